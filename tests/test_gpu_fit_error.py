"""GPU: the one-pass regression sums where they cancel -- nearly exact fits and a first sample far from the series -- against an
extended-precision / exact fit (tests/_fit_error_oracle.py; pinned to ExactFit by tests/test_fit_error_host.py).

Sites: (a, b) linreg_fit_kernel without / with a threshold, (c, d) the one-feature AnalogRegression of analog_f1_mean_kernel in its
direct and prefix forms, (e) analog_regression of sd_analog_epilogue.h, (f) grouped_window_kernel.

Fit errors: |got - exact| <= 1e-6 exact + (F + 2) eps max_rows(|icpt| + |x| . |coef|) -- the project's contract plus the rounding of
one residual evaluated in float64.  Predictions: assert_close's rule at rtol = 1e-6, |got - exact| <= 1e-6 (scale + |exact|) with
scale = the standard deviation of the exact predictions without the shifted sample.  Every test prints its worst error / tolerance
per regime before it asserts (profiles/fit_error/README.md records them)."""
import numpy as np
import pytest

import _fit_error_oracle as fe
import _lsq_oracle as lo
import analog_oracle as ao

pytestmark = pytest.mark.gpu

RTOL = 1e-6


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


class Report:
    """worst error / tolerance per key; finish() prints every (selected) key, then asserts that none is above 1"""

    def __init__(self, site):
        self.site, self.rows = site, {}

    def add(self, key, err, tol, where):
        r = np.asarray(err, dtype=np.float64) / np.asarray(tol, dtype=np.float64)
        r = np.where(np.isfinite(r), r, np.inf)
        i = int(np.argmax(r)) if r.ndim else 0
        worst = float(r.max())
        if key not in self.rows or worst > self.rows[key][0]:
            self.rows[key] = (worst, f"{where} [{i}]" if r.ndim else where)

    def finish(self, select=lambda key: True):
        rows = {k: v for k, v in self.rows.items() if select(k)}
        assert rows
        for key, (worst, where) in rows.items():
            print(f"FITERR {self.site} {key}: worst error / tolerance = {worst:.3g} at {where}")
        top = max(rows.items(), key=lambda kv: kv[1][0])
        print(f"FITERR {self.site} WORST {top[1][0]:.3g} at {top[0]} {top[1][1]}")
        bad = {k: v for k, v in rows.items() if not v[0] <= 1.0}
        assert not bad, f"{self.site}: {len(bad)} of {len(rows)} regimes out of tolerance, worst {top[1][0]:.3g} x at {top[0]} {top[1][1]}"


def pred_tol(exact, scale):
    return RTOL * max(scale, 1e-300) + RTOL * np.abs(exact)


# ---------------------------------------------------------------------------------------------------------------------------
# a. linreg_fit_kernel without a threshold
# ---------------------------------------------------------------------------------------------------------------------------
def linreg_cells(T, F):
    """one cell per regime and kind of first sample: (regime, on_line, X, y, RefFit, 16 queries)"""
    cells = []
    for i, (ratio, shift, offset, rho) in enumerate(fe.regimes(F)):
        for on_line in (True, False):
            rng = np.random.default_rng([9000, T, F, i, int(on_line)])
            X, y = fe.regime(rng, T, F, ratio, shift, offset, rho, on_line)
            # nearly collinear features: training rows only (tests/_lsq_oracle.py:make_close_case on queries off the rows)
            Q = X[rng.choice(np.arange(1, T), 16, replace=False)] if rho else fe.queries_inside(rng, X)
            cells.append(((ratio, shift, offset, rho), on_line, X, y, fe.RefFit(X, y), Q))
    return cells


KAPPA_EXACT = 100.0  # exact fits: condition number of the cell's correlation matrix beyond which the fit error is asserted apart


def exact_and_collinear(key):
    """the fit error of an exact fit (ratio = 0) on nearly collinear features -- through rho, or through a far first sample along
    (1, .., 1) in a short series.  The coefficients of the normal equations carry >= eps kappa along the weak direction and the
    residuals are evaluated with them, while the tolerance of an exact fit is the (F + 2) eps of one evaluation with exact
    coefficients: at kappa = 100 that is already an order of magnitude apart."""
    return key.startswith("rmse ratio=0 ") and key.endswith(" collinear")


@pytest.fixture(scope="module")
def linreg_runs(ctx):
    """(T, F) -> Report of one fit + predict of every regime; the bit-for-bit properties are asserted while it is filled"""
    cache = {}

    def get(T, F):
        if (T, F) not in cache:
            cache[T, F] = run_linreg(ctx, T, F)
        return cache[T, F]

    return get


def run_linreg(ctx, T, F):
    cells = linreg_cells(T, F)
    C = len(cells)
    assert C > 64 and C % 64
    X = np.ascontiguousarray(np.stack([c[2] for c in cells], axis=2))
    y = np.ascontiguousarray(np.stack([c[3] for c in cells], axis=1))
    Xq = np.ascontiguousarray(np.concatenate([X, np.stack([c[5] for c in cells], axis=2)], axis=0))
    st = ctx.linreg_fit(X, y)
    e = st.export()
    out, status = ctx.linreg_predict(st, Xq)
    assert (status == 0).all() and (e["status"] == 0).all()
    rep = Report(f"a linreg T={T} F={F}")
    for c, ((ratio, shift, offset, rho), on_line, Xc, yc, ref, Q) in enumerate(cells):
        where = f"cell {c} offset={offset:g}"
        kappa = float(np.linalg.cond(np.corrcoef(Xc, rowvar=False))) if F > 1 else 1.0
        key = f"ratio={ratio:g} shift={shift} {'leverage' if on_line else 'outlier'} rho={rho:g}{' collinear' if kappa > KAPPA_EXACT else ''}"
        tol = fe.fit_error_tol(ref.rmse, float(ref.eval_slack(Xc).max()))
        rep.add("rmse " + key, abs(e["fit_error"][c] - ref.rmse), tol, where)
        assert (out[:, 2, c] == e["fit_error"][c]).all() and (out[:, 1, c] == 1.0).all(), where
        exact = ref.predict(Xq[:, :, c])
        rep.add("pred " + key, np.abs(out[:, 0, c] - exact), pred_tol(exact, float(np.std(exact[1:T]))), where)
    # resident inputs
    rst = ctx.linreg_fit(ctx.to_device(X), ctx.to_device(y))
    rout, rstatus = ctx.linreg_predict(rst, ctx.to_device(Xq))
    re = rst.export()
    assert np.array_equal(rout.to_host(), out) and np.array_equal(rstatus, status), "resident inputs differ from host inputs"
    assert all(np.array_equal(re[k], e[k]) for k in ("coef", "intercept", "fit_error"))
    # another ordering: every cell gets other neighbours in its tile, another lane and another tile
    perm = np.random.default_rng(T + F).permutation(C)
    pe = ctx.linreg_fit(np.ascontiguousarray(X[:, :, perm]), np.ascontiguousarray(y[:, perm])).export()
    for k in ("coef", "intercept", "fit_error"):
        assert np.array_equal(pe[k], e[k][..., perm]), f"{k} of a cell depends on the cells that share its tile"
    return rep


@pytest.mark.parametrize("F", [1, 2, 8])
@pytest.mark.parametrize("T", [40, 2000, 14600])
def test_pure_regression_fit_error_and_predictions(linreg_runs, T, F):
    """Every regime (ratio x shift x offset x rho) with a leverage point and with an outlier as first sample: 112 (F = 1) or 224
    cells, so several tiles of 64 and a ragged one.  fit_error_, column 2 of predict, column 0 at the training rows and at 16 queries
    inside the data range; host and resident inputs bit for bit; a second ordering of the cells bit for bit per cell.  (The fit
    error of the exact fits on nearly collinear features is asserted by the next test, on the same run.)"""
    linreg_runs(T, F).finish(lambda key: not exact_and_collinear(key))


@pytest.mark.parametrize("F", [2, 8])
@pytest.mark.parametrize("T", [40, 2000, 14600])
def test_pure_regression_fit_error_of_exact_fits_with_nearly_collinear_features(linreg_runs, T, F):
    """ratio = 0 on nearly collinear features: the fit error is the rounding of the residuals, and the tolerance is the rounding of
    evaluating one residual with exact coefficients.  The coefficients of one-pass sums and normal equations carry
    ~ eps sqrt(T kappa) of the prediction along the weak direction (condition 1e2 to 1e8 here), which put these cells 9 to 1.3e3 times
    out of tolerance; the kernel's refinement step on the residual pass (d = S^-1 Xc^T r, taken where d . Xc^T r exceeds 1e-7 of the
    residual sum) is what holds them (profiles/fit_error/README.md)."""
    linreg_runs(T, F).finish(exact_and_collinear)


# ---------------------------------------------------------------------------------------------------------------------------
# b. linreg_fit_kernel with a threshold: the shift is the cell's first sample even when the threshold excludes it
# ---------------------------------------------------------------------------------------------------------------------------
THRESH_RATIOS = (1e-2, 1e-6, 1e-10)
THRESH_DIST = (0, 100, 1000)


class ConstantSecond:
    """the fit of two features of which the second is constant over the samples: coefficient 0 (the minimum-norm solution), the rest
    is the fit on the first feature"""

    F = 2

    def __init__(self, ref):
        self.ref, self.rmse = ref, ref.rmse

    def predict(self, Q):
        return self.ref.predict(np.atleast_2d(Q)[:, :1])

    def eval_slack(self, Q):
        return (self.F + 2) * fe.EPS * (abs(self.ref.intercept) + np.abs(np.atleast_2d(Q)[:, 0]) * abs(self.ref.coef[0]))


@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("T", [2000, 14600])
def test_pure_regression_threshold_excludes_the_first_sample(ctx, T, F):
    """thresh = 0; a random half of every cell's samples exceeds it and lies on the line, the first sample does not and lies 0, 100
    or 1000 sigma from the exceeding subset.The fit error always comes from the residual pass here (the control); the coefficients come from the shifted sums.
    Columns 0 (at the exceeding rows and 16 queries inside their range) and 2 against the fit of the exceeding subset.  F = 2 adds
    three cells whose second feature is constant over the exceeding samples only: coefficient exactly 0 through the re-centred sums."""
    cells = []
    for i, (ratio, dist, offset) in enumerate((r, d, o) for r in THRESH_RATIOS for d in THRESH_DIST for o in fe.OFFSETS):
        rng = np.random.default_rng([9100, T, F, i])
        X, y = fe.regime(rng, T, F, ratio, 0, offset, 0.0, True)
        exc = rng.random(T) < 0.5  # drawn apart from X: the logistic column (not checked here) has nothing to separate
        exc[0] = False
        y -= float(y[exc].min()) - 1.0
        y[~exc] = -1.0 - np.abs(y[~exc])
        X[0] += dist * fe.SIGMA
        assert np.array_equal(exc, y > 0.0)
        cells.append((ratio, dist, offset, X, y, exc, fe.RefFit(X[exc], y[exc]), fe.queries_inside(rng, X[exc])))
    constant = []
    if F == 2:  # feature 1 constant over the exceeding subset at a decimal value, and elsewhere (the first sample too) not
        for dist in THRESH_DIST:
            rng = np.random.default_rng([9150, T, dist])
            X0, y = fe.regime(rng, T, 1, 1e-6, 0, 280.0, 0.0, True)
            X = np.column_stack([X0[:, 0], 280.0 + fe.SIGMA * rng.standard_normal(T)])
            exc = rng.random(T) < 0.5
            exc[0] = False
            y -= float(y[exc].min()) - 1.0
            y[~exc] = -1.0 - np.abs(y[~exc])
            X[exc, 1] = 280.1
            X[0] += dist * fe.SIGMA
            Q = fe.queries_inside(rng, X[exc])
            constant.append(len(cells))
            cells.append((1e-6, dist, 280.0, X, y, exc, ConstantSecond(fe.RefFit(X[exc][:, :1], y[exc])), Q))
    X = np.ascontiguousarray(np.stack([c[3] for c in cells], axis=2))
    y = np.ascontiguousarray(np.stack([c[4] for c in cells], axis=1))
    Xq = np.ascontiguousarray(np.concatenate([X, np.stack([c[7] for c in cells], axis=2)], axis=0))
    st = ctx.linreg_fit(X, y, 0.0)
    e = st.export()
    out, status = ctx.linreg_predict(st, Xq)
    assert (status == 0).all() and (e["status"] == 0).all() and not e["thresh_dropped"].any()
    assert not constant or (e["coef"][1, constant] == 0.0).all(), f"a feature constant over the exceeding samples got coefficients {e['coef'][1, constant]}"
    rep = Report(f"b linreg thresh T={T} F={F}")
    for c, (ratio, dist, offset, Xc, yc, exc, ref, Q) in enumerate(cells):
        where, key = f"cell {c} offset={offset:g}", f"ratio={ratio:g} first sample {dist} sigma out{' constant feature' if c in constant else ''}"
        assert not exc[0] and 0.4 * T < exc.sum() < 0.6 * T
        rep.add("rmse " + key, abs(e["fit_error"][c] - ref.rmse), fe.fit_error_tol(ref.rmse, float(ref.eval_slack(Xc[exc]).max())), where)
        assert (out[:, 2, c] == e["fit_error"][c]).all()
        rows = np.concatenate([exc, np.ones(16, bool)])
        exact = ref.predict(Xq[rows, :, c])
        rep.add("pred " + key, np.abs(out[rows, 0, c] - exact), pred_tol(exact, float(np.std(exact))), where)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# c, d. AnalogRegression with one feature: direct window sums (k <= 64) and prefix differences (k > 64, or the development
# library's SD_ANALOG_REG_PREFIX)
# ---------------------------------------------------------------------------------------------------------------------------
F1_T, F1_TQ = 6000, 150


def f1_cells(with_outlier):
    """-> names, X [T, 1, C], y [T, C], Xq [Tq, 1, C]: the ratio ladder at offsets 0 and 280 on both series, x rounded to 1/8 (ties
    in the distances: the exact walk), a constant y; with_outlier: one y sample 1e4 sigma out at a small x, so that every later prefix
    value carries its magnitude.  Queries: two thirds drawn like the data, a third spread evenly from 0.5 sigma below the fitted x
    to 0.5 sigma above."""
    rng = np.random.default_rng(9200)
    names, Xs, ys, Qs = [], [], [], []
    for ratio in fe.RATIOS:
        for offset in fe.OFFSETS:
            X, y = fe.regime(rng, F1_T, 1, ratio, 0, offset, 0.0, True)
            y += offset - float(np.mean(y))  # both series around the offset
            names.append(f"ratio={ratio:g} offset={offset:g}"), Xs.append(X[:, 0]), ys.append(y)
    X, y = fe.regime(rng, F1_T, 1, 1e-2, 0, 0.0, 0.0, True)
    names.append("x rounded to 1/8"), Xs.append(np.round(X[:, 0] * 8) / 8), ys.append(y)
    X, y = fe.regime(rng, F1_T, 1, 1e-2, 0, 280.0, 0.0, True)
    names.append("constant y"), Xs.append(X[:, 0]), ys.append(np.full(F1_T, 3.25))
    if with_outlier:
        X, y = fe.regime(rng, F1_T, 1, 1e-6, 0, 0.0, 0.0, True)
        y[int(np.argsort(X[:, 0])[20])] += 1e4 * float(np.std(y))
        names.append("y outlier 1e4 sigma at a small x"), Xs.append(X[:, 0]), ys.append(y)
    for x in Xs:
        n = F1_TQ // 3
        q = np.concatenate([rng.choice(x, F1_TQ - n) + 0.3 * rng.standard_normal(F1_TQ - n),
                            np.linspace(x.min() - 0.5 * fe.SIGMA, x.max() + 0.5 * fe.SIGMA, n)])
        Qs.append(np.round(q * 8) / 8 if np.array_equal(x, np.round(x * 8) / 8) else q)
    return names, np.stack(Xs, axis=1)[:, None, :].copy(), np.stack(ys, axis=1).copy(), np.stack(Qs, axis=1)[:, None, :].copy()


@pytest.fixture(scope="module")
def f1_data():
    cache = {}

    def get(with_outlier):
        if with_outlier not in cache:
            cache[with_outlier] = f1_cells(with_outlier)
        return cache[with_outlier]

    return get


def check_f1(c_, st, data, k, site):
    """every query of every cell against the exact line through its k analogs (the window from the oracle's knn)"""
    names, X, y, Xq = data
    out, status = c_.analogreg_predict(st, Xq, k)
    assert (status == 0).all()
    rep = Report(site)
    for c, name in enumerate(names):
        _, ii = ao.knn(X[:, :, c], Xq[:, :, c], k)
        lines = [fe.ExactLine(X[ii[t], 0, c], y[ii[t], c]) for t in range(F1_TQ)]
        exact = np.array([ln.predict(Xq[t, 0, c])[0] for t, ln in enumerate(lines)])
        rmse = np.array([ln.rmse for ln in lines])
        slack = np.array([ln.eval_slack(X[ii[t], 0, c]).max() for t, ln in enumerate(lines)])
        big = np.abs(y[:, c] - np.median(y[:, c])) > 1e3 * np.subtract(*np.percentile(y[:, c], [75, 25]))  # (the outlier sample, if any)
        usual = np.array([not big[ii[t]].any() for t in range(F1_TQ)]) if big.any() else np.ones(F1_TQ, bool)
        assert usual.sum() > F1_TQ // 2
        rep.add(f"pred {name}", np.abs(out[:, 0, c] - exact), pred_tol(exact, float(np.std(exact[usual]))), f"cell {c} query")
        rep.add(f"rmse {name}", np.abs(out[:, 2, c] - rmse), fe.fit_error_tol(rmse, slack), f"cell {c} query")
        assert (out[:, 1, c] == 1.0).all()
    rep.finish()


@pytest.mark.parametrize("k", [5, 30, 64])
def test_analog_regression_one_feature_direct_window_sums(ctx, f1_data, k):
    """ss = vyy - slope wxy centred on the window's first pair, gate ss > 1e-7 vyy"""
    data = f1_data(False)
    check_f1(ctx, ctx.analog_fit(data[1], data[2]), data, k, f"c analog F=1 direct k={k}")


@pytest.mark.parametrize("k", [65, 200])
def test_analog_regression_one_feature_prefix_differences(ctx, f1_data, k):
    """ss = vyy - slope vxy from prefix differences centred on the cell means, gate ss > 1e-4 k var(y): production library, k > 64"""
    data = f1_data(True)
    check_f1(ctx, ctx.analog_fit(data[1], data[2]), data, k, f"d analog F=1 prefix k={k}")


@pytest.mark.parametrize("k", [5, 30])
def test_analog_regression_one_feature_prefix_differences_short_windows(dev_ctx, monkeypatch, f1_data, k):
    """the same form at short windows, which the development library keeps behind SD_ANALOG_REG_PREFIX: a five-analog window's
    residual sum against the rounding of the cell totals"""
    data = f1_data(True)
    monkeypatch.setenv("SD_ANALOG_REG_PREFIX", "1")
    check_f1(dev_ctx, dev_ctx.analog_fit(data[1], data[2]), data, k, f"d analog F=1 prefix (dev) k={k}")


# ---------------------------------------------------------------------------------------------------------------------------
# e. analog_regression of sd_analog_epilogue.h
# ---------------------------------------------------------------------------------------------------------------------------
def test_analog_regression_epilogue_nearly_exact_fits_and_a_far_analog(ctx):
    """F = 3, k = 40, T = 2000 around 280: the per-query sums are shifted by the query's nearest analog, which for a quarter of the
    last cell's queries is a leverage point 30 sigma out.  Windows with kappa > 1e4 are left out, at most 5 % per cell (the host test
    asserts that the data stay under the cap)."""
    X, y, Xq = fe.epilogue_cells()
    st = ctx.analog_fit(X, y)
    out, status = ctx.analogreg_predict(st, Xq, fe.EPI_K)
    assert (status == 0).all()
    rep = Report("e analog epilogue F=3 k=40")
    nq = fe.EPI_TQ // 4
    for c in range(X.shape[2]):
        name = f"ratio={fe.EPI_RATIOS[c]:g}" if c < len(fe.EPI_RATIOS) else "ratio=1e-06 far analog"
        _, ii = ao.knn(X[:, :, c], Xq[:, :, c], fe.EPI_K)
        fits = [lo.ExactFit(X[ii[t], :, c], y[ii[t], c]) for t in range(fe.EPI_TQ)]
        keep = np.array([f.kappa <= lo.KAPPA_MAX for f in fits])
        assert 1.0 - keep.mean() <= fe.EPI_CAP, f"cell {c}: {1.0 - keep.mean():.1%} of the windows left out"
        exact = np.array([f.predict(Xq[t, :, c])[0] for t, f in enumerate(fits)])
        rmse = np.array([f.rmse for f in fits])
        slack = np.array([fe.exact_eval_slack(f, f.X).max() for f in fits])
        scale = float(np.std(exact[nq:] if c == X.shape[2] - 1 else exact))
        rep.add(f"pred {name}", np.abs(out[keep, 0, c] - exact[keep]), pred_tol(exact[keep], scale), f"cell {c} kept query")
        rep.add(f"rmse {name}", np.abs(out[keep, 2, c] - rmse[keep]), fe.fit_error_tol(rmse[keep], slack[keep]), f"cell {c} kept query")
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# f. grouped_window_kernel: every group's sums are shifted by the cell's first sample
# ---------------------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (24, 40, 31, 27, 36, 33)
GROUP_RATIOS = (1e-2, 1e-6, 1e-10)
GROUP_SHIFTS = (0, 100, 1000)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("window", [0, 1])
def test_grouped_regressor_with_a_far_first_sample(ctx, F, window):
    """six keys of 24 to 40 real-valued samples in no particular order in time; the cell's first sample moved 0, 100 or 1000 sigma
    along the line: a leverage point for its own group (and its neighbours' windows), a far shift for every other group.
    Predictions at the training rows of every group against the exact fit of the group's window."""
    n, T = len(GROUP_SIZES), sum(GROUP_SIZES)
    key = np.random.default_rng(9300).permutation(np.repeat(np.arange(n), GROUP_SIZES))
    cells = []
    for i, (ratio, shift, offset) in enumerate((r, s, o) for r in GROUP_RATIOS for s in GROUP_SHIFTS for o in fe.OFFSETS):
        X, y = fe.regime(np.random.default_rng([9300, F, i]), T, F, ratio, shift, offset, 0.0, True)
        cells.append((ratio, shift, offset, X, y))
    X = np.ascontiguousarray(np.stack([c[3] for c in cells], axis=2))
    y = np.ascontiguousarray(np.stack([c[4] for c in cells], axis=1))
    st = ctx.grouped_fit(X, y, key, n, window)
    out, status = ctx.grouped_predict(st, X, key)
    assert (status == 0).all() and st.export()["fitted"].all()
    st.close()
    rep = Report(f"f grouped F={F} window={window}")
    for c, (ratio, shift, offset, Xc, yc) in enumerate(cells):
        exact = np.empty(T)
        for g in range(n):
            members = np.isin(key, [(g + j) % n for j in range(-window, window + 1)])
            fit = lo.ExactFit(Xc[members], yc[members])
            assert fit.rank == F
            exact[key == g] = fit.predict(Xc[key == g])
        own = f"first sample {shift} sigma out"
        rep.add(f"pred ratio={ratio:g} {own}", np.abs(out[:, c] - exact), pred_tol(exact, float(np.std(exact[1:]))), f"cell {c} offset={offset:g} row")
    rep.finish()
