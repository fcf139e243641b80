"""Host: the extended-precision reference of tests/_fit_error_oracle.py against the exact rational fit (tests/_lsq_oracle.py:ExactFit), and
the reach of the regime generator.  The GPU tests of tests/test_gpu_fit_error.py rest on both."""
import numpy as np
import pytest

import _fit_error_oracle as fe
import _lsq_oracle as lo
import analog_oracle as ao

# 16 of the regimes at T = 2000: every ratio, every shift, both offsets, both correlations, leverage points and outliers
SUBSET = [
    # F, ratio, shift, offset, rho, on_line
    (1, 1e-2, 0, 0.0, 0.0, True), (1, 1e-4, 10, 280.0, 0.0, False), (1, 1e-6, 100, 0.0, 0.0, True), (1, 1e-8, 1000, 280.0, 0.0, True),
    (1, 3e-9, 0, 280.0, 0.0, True), (1, 1e-10, 100, 280.0, 0.0, False), (1, 0.0, 1000, 0.0, 0.0, True), (1, 0.0, 0, 280.0, 0.0, True),
    (2, 1e-2, 1000, 280.0, 0.9999, False), (2, 1e-4, 0, 0.0, 0.9999, True), (2, 1e-6, 10, 280.0, 0.0, True), (2, 1e-8, 100, 0.0, 0.9999, True),
    (2, 3e-9, 1000, 280.0, 0.9999, True), (2, 1e-10, 0, 280.0, 0.9999, True), (2, 0.0, 100, 280.0, 0.9999, False), (2, 3e-9, 0, 0.0, 0.0, True),
]
LONG_CELLS = [(1, 1e-8, 100, 280.0, 0.0, True), (2, 3e-9, 1000, 280.0, 0.9999, True)]  # T = 14600


def check_against_exact(T, F, ratio, shift, offset, rho, on_line, seed):
    X, y = fe.regime(np.random.default_rng(seed), T, F, ratio, shift, offset, rho, on_line)
    ref, exact = fe.RefFit(X, y), lo.ExactFit(X, y)
    where = f"T={T} F={F} ratio={ratio:g} shift={shift} offset={offset:g} rho={rho:g} on_line={on_line}"
    assert exact.rank == F, where
    slack = float(fe.exact_eval_slack(exact, X).max()) if ratio == 0.0 else 0.0
    err = abs(ref.rmse - exact.rmse)
    assert err <= 1e-10 * exact.rmse + slack, f"{where}: rmse {ref.rmse!r} vs exact {exact.rmse!r}"
    perr = np.abs(ref.predict(X) - exact.predict(X)).max()
    assert perr <= 1e-10 * float(np.std(y)), f"{where}: predictions at the training rows off by {perr:.3e}"
    return err / max(exact.rmse, 1e-300), perr / float(np.std(y))


@pytest.mark.parametrize("i", range(len(SUBSET)))
def test_reference_agrees_with_exact_fit(i):
    r, p = check_against_exact(2000, *SUBSET[i], seed=8000 + i)
    print(f"regime {SUBSET[i]}: rmse rel. error {r:.2e}, prediction error / std(y) {p:.2e}")


def test_reference_agrees_with_exact_fit_on_a_short_series_made_collinear_by_a_leverage_point():
    """T = 40, F = 8, exact fits with the first sample 1000 sigma out along (1, .., 1), with and without rho = 0.9999: the correlation
    matrix has a condition number of 4e5 and 2e9, the regime the refinement rows of tests/test_gpu_fit_error.py rest on"""
    for j, rho in enumerate((0.0, 0.9999)):
        for on_line in (True, False):
            X, _ = fe.regime(np.random.default_rng(8120 + j), 40, 8, 0.0, 1000, 280.0, rho, on_line)
            kappa = float(np.linalg.cond(np.corrcoef(X, rowvar=False)))
            assert kappa > 1e5
            r, p = check_against_exact(40, 8, 0.0, 1000, 280.0, rho, on_line, seed=8120 + j)
            print(f"T=40 F=8 rho={rho:g} on_line={on_line} kappa={kappa:.2g}: rmse rel. error {r:.2e}, prediction error / std(y) {p:.2e}")


@pytest.mark.parametrize("i", range(len(LONG_CELLS)))
def test_reference_agrees_with_exact_fit_at_the_workload_length(i):
    r, p = check_against_exact(14600, *LONG_CELLS[i], seed=8100 + i)
    print(f"regime {LONG_CELLS[i]}: rmse rel. error {r:.2e}, prediction error / std(y) {p:.2e}")


def test_reference_without_long_double_is_the_exact_fit(monkeypatch):
    """where numpy's long double is no wider than float64 the reference is ExactFit itself: the same numbers, slowly"""
    X, y = fe.regime(np.random.default_rng(8150), 40, 2, 1e-8, 100, 280.0, 0.9999, True)
    ref = fe.RefFit(X, y)
    monkeypatch.setattr(fe, "HAVE_LONG", False)
    slow = fe.RefFit(X, y)
    assert abs(slow.rmse - ref.rmse) <= 1e-10 * slow.rmse and np.abs(slow.predict(X) - ref.predict(X)).max() <= 1e-10 * float(np.std(y))
    assert np.array_equal(slow.eval_slack(X), fe.exact_eval_slack(lo.ExactFit(X, y), X))


@pytest.mark.parametrize("T,F", [(40, 1), (2000, 2), (14600, 1), (2000, 8)])
def test_generator_reaches_the_ratio_and_is_deterministic(T, F):
    for ratio, shift, offset, rho in fe.regimes(F):
        if shift or ratio == 0.0:
            continue
        X, y = fe.regime(np.random.default_rng(8200), T, F, ratio, shift, offset, rho, True)
        X2, y2 = fe.regime(np.random.default_rng(8200), T, F, ratio, shift, offset, rho, True)
        assert np.array_equal(X, X2) and np.array_equal(y, y2)
        ref = fe.RefFit(X, y)
        got = ref.rmse ** 2 / float(np.var(y))
        assert ratio / 3 <= got <= 3 * ratio, f"T={T} F={F} offset={offset:g} rho={rho:g}: rss / Syy = {got:.3e}, asked for {ratio:g}"
        assert abs(float(np.std(X[:, 0])) / fe.SIGMA - 1.0) < 0.35 and abs(float(np.mean(X[:, 0])) - offset) < 0.5 * fe.SIGMA
        if F >= 2:
            assert abs(float(np.corrcoef(X[:, 0], X[:, 1])[0, 1]) - rho) < (0.02 if rho else 0.45 if T < 100 else 0.1)


def test_shifted_first_sample_is_a_leverage_point_or_an_outlier():
    for shift in (10, 100, 1000):
        base = fe.RefFit(*fe.regime(np.random.default_rng(8300), 2000, 2, 1e-6, 0, 280.0, 0.0, True)).rmse
        Xl, yl = fe.regime(np.random.default_rng(8300), 2000, 2, 1e-6, shift, 280.0, 0.0, True)
        Xo, yo = fe.regime(np.random.default_rng(8300), 2000, 2, 1e-6, shift, 280.0, 0.0, False)
        assert np.allclose(Xl[0] - 280.0, shift * fe.SIGMA, atol=5 * fe.SIGMA) and np.array_equal(Xl, Xo) and np.array_equal(yl[1:], yo[1:])
        assert fe.RefFit(Xl, yl).rmse <= 1.5 * base      # on the line: rss stays small while Syy grows
        assert fe.RefFit(Xo, yo).rmse >= 10.0 * base     # off the line: rss grows


def test_exact_line_is_exact_fit_for_one_feature():
    rng = np.random.default_rng(8400)
    for k, kind in [(5, "real"), (30, "real"), (64, "offset"), (200, "real"), (5, "equal_x"), (30, "constant_y"), (30, "on_line")]:
        x, y = rng.standard_normal(k), rng.standard_normal(k)
        if kind == "offset":
            x, y = 280.0 + x, 280.0 + y
        elif kind == "equal_x":
            x[:] = 0.375
        elif kind == "constant_y":
            y[:] = 3.25
        elif kind == "on_line":
            x = np.round(x * 8) / 8
            y = 2.0 * x + 1.0
        line, exact = fe.ExactLine(x, y), lo.ExactFit(x[:, None], y)
        assert line.slope == exact.coef[0] and line.intercept == exact.intercept, (k, kind)
        assert abs(line.rmse - exact.rmse) <= 1e-15 * exact.rmse, (k, kind, line.rmse, exact.rmse)
        q = rng.standard_normal(4)
        assert np.array_equal(line.predict(q), exact.predict(q[:, None]))
        assert np.array_equal(line.eval_slack(q), fe.exact_eval_slack(exact, q[:, None]))


def test_epilogue_cells_stay_under_the_cap_of_left_out_windows():
    """tests/test_gpu_fit_error.py leaves out windows of kappa > 1e4 in its analog_regression test, at most 5 % of a cell's queries:
    the data alone must stay under that cap"""
    X, y, Xq = fe.epilogue_cells()
    nq = fe.EPI_TQ // 4
    for c in range(X.shape[2]):
        _, ii = ao.knn(X[:, :, c], Xq[:, :, c], fe.EPI_K)
        if c == X.shape[2] - 1:
            assert (ii[:nq, 0] == 7).all(), "the far leverage point is not the nearest analog of the queries beyond it"
        kap = np.array([lo.ExactFit(X[ii[t], :, c], y[ii[t], c]).kappa for t in range(fe.EPI_TQ)])
        share = float((kap > lo.KAPPA_MAX).mean())
        assert share <= fe.EPI_CAP, f"cell {c}: {share:.1%} of the windows have kappa > 1e4 (largest {kap.max():.3g})"
