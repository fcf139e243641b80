"""GPU: sdlsq::minnorm_solve through its three call sites -- linreg_fit_kernel (PureRegression), grouped_window_kernel
(GroupedRegressor) and the per-query epilogue analog_regression (AnalogRegression) -- against the exact rational reference of
tests/_lsq_oracle.py, on rank-deficient and under-determined designs (0 <= rank <= F at every F, fewer samples than features).

Tolerance per design: tol = K eps kappa max|y - mean(y)| with K measured on the LAPACK twin (_lsq_oracle.py), plus the rounding of
evaluating icpt + q . coef in float64 where a prediction of the kernel is compared, (F + 2) eps (|icpt| + sum |q_f coef_f|).
Every test prints its largest error / (eps kappa) (profiles/lsq/README.md records them per call site)."""
import numpy as np
import pytest

import _lsq_oracle as lo
import analog_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


class Worst:
    """largest error in units of eps * kappa * yscale seen by a test"""

    def __init__(self):
        self.ratio, self.where = 0.0, ""

    def add(self, fit, err, where):
        if fit.yscale > 0 and err / (lo.EPS * fit.kappa * fit.yscale) > self.ratio:
            self.ratio, self.where = err / (lo.EPS * fit.kappa * fit.yscale), where


def eval_slack(fit, Q):
    """rounding of icpt + q . coef evaluated in float64 with the exact coefficients, per row of Q"""
    c = np.abs(fit.coef_f())
    return (fit.F + 2) * lo.EPS * (abs(float(fit.intercept)) + np.abs(np.atleast_2d(Q)) @ c)


def check_model(fit, coef, icpt, Q, worst, where):
    """the exported model of one design: constant features exactly 0, (a) queries, (b) training rows, (c) null-space component, and
    the intercept through the prediction at the feature means"""
    F = fit.F
    const = [f for f in range(F) if fit.S[f][f] == 0]
    assert all(coef[f] == 0.0 for f in const), f"{where}: constant features {const} have coefficients {coef}"
    ea, eb, ec, _ = fit.errors(coef, Q)
    tol = fit.tol()
    worst.add(fit, max(ea, eb), where)
    assert ea <= tol, f"{where}: (a) prediction at the queries off by {ea:.3e} > {tol:.3e} (kappa {fit.kappa:.3g})"
    assert eb <= tol, f"{where}: (b) prediction at the training rows off by {eb:.3e} > {tol:.3e} (kappa {fit.kappa:.3g})"
    rel = lo.K * lo.EPS * fit.kappa
    assert ec <= rel, f"{where}: (c) null-space component of the coefficients {ec:.3e} > {rel:.3e} (kappa {fit.kappa:.3g})"
    xm = np.array([float(v) for v in fit.xm])
    ei = abs(icpt + float(xm @ coef) - float(fit.ym))  # the fitted line passes through the means
    slack = tol + (F + 2) * lo.EPS * (abs(icpt) + float(np.abs(xm) @ np.abs(coef)))
    assert ei <= slack, f"{where}: intercept off by {ei:.3e} > {slack:.3e}"


def check_values(fit, got, exact, slack, worst, where, what):
    err = np.abs(np.asarray(got) - np.asarray(exact))
    assert np.isfinite(err).all(), f"{where}: {what} not finite: {got}"
    worst.add(fit, float(np.max(np.maximum(err - slack, 0.0))), where)
    bad = err > fit.tol() + slack
    assert not bad.any(), f"{where}: {what} off by {err.max():.3e} > {fit.tol():.3e} + {np.max(slack):.1e} (kappa {fit.kappa:.3g})"


# ---------------------------------------------------------------------------------------------------------------------------
# PureRegression
# ---------------------------------------------------------------------------------------------------------------------------
def linreg_designs(F, T, count, seed):
    """`count` designs of T samples, the ranks 0..min(F, T-1) in turn; in turn also the kind of design: small mixed scales, wide
    scales (2^[-17,17]: full rank, or rank deficient through constant columns only), a duplicated column"""
    rng = np.random.default_rng(seed)
    rmax = min(F, T - 1)
    out = []
    for i in range(count):
        r, kind = i % (rmax + 1), (i // (rmax + 1)) % 3
        if r == 0 or kind == 0 or (kind == 2 and (r == F or F < 2)):
            X, y, fit = lo.make_case(rng, T, F, r, 3)
        elif kind == 1:
            X, y, fit = lo.make_case(rng, T, F, r, 17, n_const=F - r)
        else:
            X, y, fit = lo.make_case(rng, T, F, r, 3, dup=True)
        out.append((X, y, fit, lo.make_queries(rng, X, 16)))
    return out


def stack(designs):
    X = np.stack([d[0] for d in designs], axis=2)
    y = np.stack([d[1] for d in designs], axis=1)
    Xq = np.stack([d[3] for d in designs], axis=2)
    return np.ascontiguousarray(X), np.ascontiguousarray(y), np.ascontiguousarray(Xq)


def check_linreg(designs, e, out, status, worst, tag):
    assert (status == 0).all() and (e["status"] == 0).all()
    for c, (X, y, fit, Q) in enumerate(designs):
        where = f"{tag} cell {c} (rank {fit.rank})"
        coef = e["coef"][:, c]
        if fit.rank == 0:
            assert (coef == 0.0).all(), f"{where}: rank 0 but coefficients {coef}"
        check_model(fit, coef, float(e["intercept"][c]), Q, worst, where)
        check_values(fit, out[:, 0, c], fit.predict(Q), eval_slack(fit, Q), worst, where, "pred")
        assert (out[:, 1, c] == 1.0).all()
        check_values(fit, out[:, 2, c], fit.rmse, float(eval_slack(fit, fit.X).max()), worst, where, "(d) fit error")
        assert e["fit_error"][c] == out[0, 2, c]


@pytest.mark.parametrize("F", range(1, 9))
def test_pure_regression_every_rank(ctx, F):
    """T = 40 (crosses the 8-slice x 4-unroll stride of 32), 65 cells (a full tile of 64 and a ragged one), every cell its own
    design, ranks 0..F; host and resident inputs; a masked and a non-finite cell do not disturb the cells that share their tile."""
    from skdownscale_amd import _lib

    worst = Worst()
    designs = linreg_designs(F, 40, 65, 1000 + F)
    assert {d[2].rank for d in designs} == set(range(F + 1))
    X, y, Xq = stack(designs)
    st = ctx.linreg_fit(X, y)
    e = st.export()
    out, status = ctx.linreg_predict(st, Xq)
    check_linreg(designs, e, out, status, worst, f"F={F} T=40")
    rst = ctx.linreg_fit(ctx.to_device(X), ctx.to_device(y))
    rout, rstatus = ctx.linreg_predict(rst, ctx.to_device(Xq))
    re = rst.export()
    assert np.array_equal(rout.to_host(), out) and np.array_equal(rstatus, status), "resident inputs differ from host inputs"
    assert all(np.array_equal(re[k], e[k]) for k in ("coef", "intercept", "fit_error"))
    # the same cells with a masked cell at 3 and a non-finite cell at 10: 67 cells, every other cell moves within its tile
    keep = np.array([c for c in range(67) if c not in (3, 10)])
    X2, y2, Xq2 = np.zeros((40, F, 67)), np.zeros((40, 67)), np.zeros((16, F, 67))
    X2[:, :, keep], y2[:, keep], Xq2[:, :, keep] = X, y, Xq
    X2[:, :, [3, 10]], y2[:, [3, 10]], Xq2[:, :, [3, 10]] = X[:, :, [0, 1]], y[:, [0, 1]], Xq[:, :, [0, 1]]
    X2[0, 0, 3] = np.nan    # masked cell
    y2[20, 10] = np.inf     # non-finite target
    st2 = ctx.linreg_fit(X2, y2)
    e2 = st2.export()
    out2, status2 = ctx.linreg_predict(st2, Xq2)
    assert status2[3] == _lib.CELL_MASKED and status2[10] == _lib.CELL_NONFINITE and (status2[keep] == 0).all()
    assert np.isnan(out2[:, :, [3, 10]]).all()
    for k in ("coef", "intercept", "fit_error"):
        assert np.array_equal(e2[k][..., keep], e[k]), f"{k} of the neighbours of a masked / non-finite cell changed"
    assert np.array_equal(out2[:, :, keep], out)
    print(f"linreg F={F}: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


@pytest.mark.parametrize("F", range(1, 9))
def test_pure_regression_fewer_samples_than_features(ctx, F):
    """T in {1, 2, F, F + 1}: at most T - 1 directions are determined, the rest is the minimum-norm part"""
    worst = Worst()
    for T in sorted({1, 2, F, F + 1}):
        designs = linreg_designs(F, T, 2 * (min(F, T - 1) + 1) + 1, 2000 + 10 * F + T)
        X, y, Xq = stack(designs)
        st = ctx.linreg_fit(X, y)
        out, status = ctx.linreg_predict(st, Xq)
        check_linreg(designs, st.export(), out, status, worst, f"F={F} T={T}")
    print(f"linreg short F={F}: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


def thresh_designs(F, seed, T=40):
    """cells whose exceeding subset (y > 0) has ne = 1..F samples: the subset design has rank ne - 1 < F"""
    rng = np.random.default_rng(seed)
    out = []
    for ne in list(range(1, F + 1)) * 2:
        for _ in range(50):
            s, o = 2.0 ** rng.integers(-3, 4, F), rng.integers(-5, 6, F)
            X = (rng.integers(-8, 9, (T, F)) + o) * s
            y = -rng.integers(1, 10, T).astype(float)
            exc = rng.choice(T, ne, replace=False)
            y[exc] = rng.integers(1, 10, ne)
            if ne > 1 and np.ptp(y[exc]) == 0:
                continue
            fit = lo.ExactFit(X[np.sort(exc)], y[np.sort(exc)])
            if fit.rank == ne - 1 and fit.kappa <= lo.KAPPA_MAX:
                break
        else:
            raise RuntimeError("no thresholded design")
        out.append((X, y, fit, lo.make_queries(rng, X, 16)))
    return out


@pytest.mark.parametrize("F", range(1, 9))
def test_pure_regression_threshold_with_an_under_determined_subset(ctx, F):
    """PureRegression(thresh): the linear model sees the exceeding samples only, here ne <= F of them.  pred and fit error against
    the exact fit of the subset (the probability column stays with tests/test_gpu_linreg.py)."""
    worst = Worst()
    designs = thresh_designs(F, 3000 + F)
    X, y, Xq = stack(designs)
    st = ctx.linreg_fit(X, y, 0.0)
    e = st.export()
    out, status = ctx.linreg_predict(st, Xq)
    assert (status == 0).all() and not e["thresh_dropped"].any()
    for c, (Xc, yc, fit, Q) in enumerate(designs):
        where = f"F={F} thresh cell {c} (ne {fit.n})"
        check_model(fit, e["coef"][:, c], float(e["intercept"][c]), Q, worst, where)
        check_values(fit, out[:, 0, c], fit.predict(Q), eval_slack(fit, Q), worst, where, "pred")
        check_values(fit, out[:, 2, c], fit.rmse, float(eval_slack(fit, fit.X).max()), worst, where, "(d) fit error")
    print(f"linreg thresh F={F}: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


def decimal_design(rng, n, F, const_value):
    """n samples of F features rounded to one decimal, feature 1 constant at a decimal value: kappa <= 1e4 by rejection"""
    for _ in range(50):
        X = np.round(rng.standard_normal((n, F)), 1)
        X[:, 1] = const_value
        y = np.round(rng.standard_normal(n), 1)
        fit = lo.ExactFit(X, y)
        if fit.rank == F - 1 and fit.kappa <= lo.KAPPA_MAX:
            return X, y, fit
    raise RuntimeError("no decimal design")


def test_pure_regression_threshold_subset_with_a_constant_decimal_feature(ctx):
    """A feature that is constant over the exceeding samples at a value that is no dyadic number (and differs from the first sample
    of the series, the shift of the one-pass sums): its centred sum of squares is pure rounding, of either sign.  It is a constant
    feature: coefficient exactly 0.0, the other coefficients as in the exact fit."""
    worst = Worst()
    rng = np.random.default_rng(3100)
    T, F, C, ne = 40, 3, 24, 12
    designs = []
    for c in range(C):
        Xs, ys, fit = decimal_design(rng, ne, F, np.round(rng.standard_normal(), 1))
        X = np.round(rng.standard_normal((T, F)), 1)
        y = -np.abs(np.round(rng.standard_normal(T), 1)) - 0.1
        exc = np.sort(rng.choice(np.arange(1, T), ne, replace=False))  # (the first sample is not among them)
        X[exc], y[exc] = Xs, np.abs(ys) + 0.1
        fit = lo.ExactFit(X[exc], y[exc])
        assert fit.S[1][1] == 0 and fit.kappa <= lo.KAPPA_MAX
        designs.append((X, y, fit, lo.make_queries(rng, X, 16)))
    X, y, Xq = stack(designs)
    st = ctx.linreg_fit(X, y, 0.0)
    e = st.export()
    out, status = ctx.linreg_predict(st, Xq)
    assert (status == 0).all()
    for c, (Xc, yc, fit, Q) in enumerate(designs):
        where = f"decimal thresh cell {c}"
        check_model(fit, e["coef"][:, c], float(e["intercept"][c]), Q, worst, where)
        check_values(fit, out[:, 0, c], fit.predict(Q), eval_slack(fit, Q), worst, where, "pred")
        check_values(fit, out[:, 2, c], fit.rmse, float(eval_slack(fit, fit.X).max()), worst, where, "(d) fit error")
    print(f"linreg decimal thresh: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


# ---------------------------------------------------------------------------------------------------------------------------
# GroupedRegressor
# ---------------------------------------------------------------------------------------------------------------------------
def test_grouped_regressor_feature_constant_within_a_group(ctx):
    """window 0, four groups of 12 samples: feature 1 is constant within each group at a decimal value of its own (a monthly
    climatology next to daily predictors).  Constant within the group: coefficient exactly 0.0 there."""
    worst = Worst()
    rng = np.random.default_rng(4100)
    F, C, n, m = 3, 24, 4, 12
    key = np.random.default_rng(1).permutation(np.repeat(np.arange(n), m))
    fits, Xs, ys, Qs = {}, [], [], []
    for c in range(C):
        X, y, Q = np.empty((n * m, F)), np.empty(n * m), np.empty((n, F))
        for g in range(n):
            X[key == g], y[key == g], fits[c, g] = decimal_design(rng, m, F, np.round(rng.standard_normal(), 1))
            Q[g] = lo.make_queries(rng, X[key == g], 1)[0]
        Xs.append(X), ys.append(y), Qs.append(Q)
    X, y, Xq = (np.ascontiguousarray(np.stack(a, axis=-1)) for a in (Xs, ys, Qs))
    st = ctx.grouped_fit(X, y, key, n, 0)
    e = st.export()
    out, status = ctx.grouped_predict(st, Xq, np.arange(n))
    assert (status == 0).all() and e["fitted"].all()
    for (c, g), fit in fits.items():
        where = f"decimal grouped cell {c} key {g}"
        check_model(fit, e["coef"][g, :, c], float(e["intercept"][g, c]), Qs[c][g:g + 1], worst, where)
        check_values(fit, out[g, c], fit.predict(Qs[c][g])[0], float(eval_slack(fit, Qs[c][g])[0]), worst, where, "pred")
    st.close()
    print(f"grouped decimal: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


GROUPED_VARIANTS = 3  # distinct designs; the 65 cells take them in turn (the exact reference is computed once per design)


def grouped_variant(F, seed):
    """One cell's series: keys 0..F+1 hold 1, 2, .., F+2 samples, keys F+2..2F+2 hold 24 samples of designed rank 0..F; one set of
    units for the whole series, so the window-1 unions stay sane.  Returns the per-key designs and the exact fits for window 0 and
    for the circular window 1 (rejection-sampled as a whole to kappa <= 1e4 for every union)."""
    rng = np.random.default_rng(seed)
    n = 2 * F + 3
    for _ in range(50):
        units = (2.0 ** rng.integers(-3, 4, F), rng.integers(-5, 6, F).astype(float))
        parts = [lo.make_case(rng, j + 1, F, min(j, F), 3, units=units) for j in range(F + 2)]
        parts += [lo.make_case(rng, 24, F, r, 3, units=units) for r in range(F + 1)]
        unions = []
        for g in range(n):
            ks = [(g - 1) % n, g, (g + 1) % n]
            unions.append(lo.ExactFit(np.vstack([parts[k][0] for k in ks]), np.concatenate([parts[k][1] for k in ks])))
        if all(u.kappa <= lo.KAPPA_MAX for u in unions):
            Q = [lo.make_queries(rng, np.vstack([parts[k][0] for k in ((g - 1) % n, g, (g + 1) % n)]), 2) for g in range(n)]
            return parts, unions, Q
    raise RuntimeError("no grouped series with kappa <= 1e4 for every window")


@pytest.fixture(scope="module")
def grouped_series():
    cache = {}

    def get(F):
        if F not in cache:
            variants = [grouped_variant(F, 4000 + 10 * F + v) for v in range(GROUPED_VARIANTS)]
            n = 2 * F + 3
            sizes = [len(p[1]) for p in variants[0][0]]
            key = np.repeat(np.arange(n), sizes)
            perm = np.random.default_rng(F).permutation(len(key))  # the keys come in no particular order in time
            series = []
            for parts, _, Q in variants:
                X = np.vstack([p[0] for p in parts])[perm]
                y = np.concatenate([p[1] for p in parts])[perm]
                series.append((X, y, np.vstack(Q)))
            cache[F] = (variants, key[perm], np.repeat(np.arange(n), 2), series)
        return cache[F]

    return get


@pytest.mark.parametrize("F", [1, 3, 8])
@pytest.mark.parametrize("window", [0, 1])
def test_grouped_regressor_every_rank_and_short_groups(ctx, grouped_series, F, window):
    """window 0: groups of 1..F+2 samples and groups of 24 samples with rank 0..F; window 1: the circular unions of the same
    keys; 65 cells"""
    worst = Worst()
    C, n = 65, 2 * F + 3
    variants, key, key_q, series = grouped_series(F)
    X = np.ascontiguousarray(np.stack([series[c % GROUPED_VARIANTS][0] for c in range(C)], axis=2))
    y = np.ascontiguousarray(np.stack([series[c % GROUPED_VARIANTS][1] for c in range(C)], axis=1))
    Xq = np.ascontiguousarray(np.stack([series[c % GROUPED_VARIANTS][2] for c in range(C)], axis=2))
    st = ctx.grouped_fit(X, y, key, n, window)
    e = st.export()
    out, status = ctx.grouped_predict(st, Xq, key_q)
    assert (status == 0).all() and (e["status"] == 0).all() and e["fitted"].all()
    if window == 0:
        assert [variants[0][0][g][2].rank for g in range(F + 2, n)] == list(range(F + 1))
    for v, (parts, unions, Q) in enumerate(variants):
        for g in range(n):
            fit = parts[g][2] if window == 0 else unions[g]
            where = f"F={F} window={window} key {g} (n {fit.n}, rank {fit.rank})"
            check_model(fit, e["coef"][g, :, v], float(e["intercept"][g, v]), Q[g], worst, where)
            check_values(fit, out[key_q == g, v], fit.predict(Q[g]), eval_slack(fit, Q[g]), worst, where, "pred")
    for c in range(GROUPED_VARIANTS, C):  # the other cells repeat the designs: bit-identical, whatever their tile and lane
        v = c % GROUPED_VARIANTS
        assert np.array_equal(e["coef"][:, :, c], e["coef"][:, :, v]) and np.array_equal(out[:, c], out[:, v]), f"cell {c} differs from cell {v}"
    st.close()
    print(f"grouped F={F} window={window}: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


# ---------------------------------------------------------------------------------------------------------------------------
# AnalogRegression
# ---------------------------------------------------------------------------------------------------------------------------
ANALOG_T, ANALOG_TQ, ANALOG_C = 96, 24, 2
MAX_LEFT_OUT = 0.25  # share of the queries of one (F, k) whose analog set has kappa > 1e4


def analog_data(F, rounded, seed=None):
    rng = np.random.default_rng((5000 if rounded else 6000) + F if seed is None else seed)
    X = rng.standard_normal((ANALOG_T, F, ANALOG_C))
    y = rng.standard_normal((ANALOG_T, ANALOG_C))
    Xq = rng.standard_normal((ANALOG_TQ, F, ANALOG_C))
    if rounded:  # one decimal: exact ties in the distances and duplicated analogs
        X, y, Xq = np.round(X, 1), np.round(y, 1), np.round(Xq, 1)
    return X, y, Xq


def analog_reference(X, y, Xq, k, thresh=None):
    """per (query, cell): (indices of the analogs, ExactFit of the analogs that enter the linear model or None)"""
    ref = {}
    for c in range(X.shape[2]):
        _, ii = ao.knn(X[:, :, c], Xq[:, :, c], k)
        for t in range(Xq.shape[0]):
            use = ii[t] if thresh is None else ii[t][y[ii[t], c] > thresh]
            ref[t, c] = (ii[t], lo.ExactFit(X[use, :, c], y[use, c]) if len(use) else None)
    return ref


def check_analog(ctx, st, X, y, Xq, k, worst, tag, thresh=None, neighbours=True):
    """-> share of the queries left out (kappa > 1e4)"""
    ref = analog_reference(X, y, Xq, k, thresh)
    if neighbours:  # the neighbour stage first, so a failure names the right stage
        _, _, inds, _ = ctx.analog_predict(st, Xq, k, ao.KIND_MEAN, want_neighbors=True)
        for (t, c), (ii, _) in ref.items():
            assert np.array_equal(inds[t, :, c], ii), f"{tag}: neighbours of query {t} cell {c} differ"
    out, status = ctx.analogreg_predict(st, Xq, k, thresh)
    left_out = 0
    for (t, c), (ii, fit) in ref.items():
        where = f"{tag} query {t} cell {c}"
        if fit is None:
            assert np.isnan(out[t, :, c]).all(), f"{where}: no exceeding analog but {out[t, :, c]}"
            continue
        if not fit.kappa <= lo.KAPPA_MAX:
            left_out += 1
            continue
        q = Xq[t, :, c]
        check_values(fit, out[t, 0, c], fit.predict(q)[0], float(eval_slack(fit, q)[0]), worst, where, f"pred (rank {fit.rank}, n {fit.n})")
        check_values(fit, out[t, 2, c], fit.rmse, float(eval_slack(fit, fit.X).max()), worst, where, f"error column (rank {fit.rank}, n {fit.n})")
        if thresh is None:
            assert out[t, 1, c] == 1.0
    return left_out / len(ref)


@pytest.mark.parametrize("F", range(2, 9))
@pytest.mark.parametrize("rounded", [False, True])
def test_analog_regression_few_analogs(ctx, F, rounded):
    """k = 2..F+2 analogs of F features: under-determined for k <= F + 1, so the prediction at the query (outside the row space of its
    analogs) rests on the null-space handling.  Candidate-list kernel for F <= 6, heap kernel for F = 7, 8."""
    worst = Worst()
    X, y, Xq = analog_data(F, rounded)
    st = ctx.analog_fit(X, y)
    for k in range(2, F + 3):
        share = check_analog(ctx, st, X, y, Xq, k, worst, f"F={F} k={k} rounded={rounded}")
        print(f"analogreg F={F} k={k} rounded={rounded}: {share:.1%} of the queries left out (kappa > 1e4)")
        assert share <= MAX_LEFT_OUT, f"F={F} k={k}: {share:.1%} of the queries left out"
    print(f"analogreg F={F} rounded={rounded}: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where} (K = {lo.K:.0f})")


def test_analog_regression_collinear_features_heap_kernel(ctx):
    """F = 3 with a duplicated feature column (in other units) and k = 40: the heap kernel at F <= 6, rank 2 through collinearity"""
    worst = Worst()
    X, y, Xq = analog_data(3, False, seed=7001)
    X[:, 2], Xq[:, 2] = 4.0 * X[:, 0], 4.0 * Xq[:, 0]
    st = ctx.analog_fit(X, y)
    share = check_analog(ctx, st, X, y, Xq, 40, worst, "F=3 k=40 collinear")
    assert share <= MAX_LEFT_OUT
    print(f"analogreg collinear: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where}, {share:.1%} left out (K = {lo.K:.0f})")


def test_analog_regression_threshold_with_few_exceeding_analogs(ctx):
    """F = 3, k = 24 and a threshold that leaves 2..4 exceeding analogs: the linear model on them is under-determined (ne <= F + 1).
    pred and the error column against the exact fit of the exceeding analogs."""
    worst = Worst()
    X, y, _ = analog_data(3, False, seed=7002)
    thresh = float(np.quantile(y, 0.875))
    # the first 24 of 400 candidate queries per cell whose 24 analogs hold 2..4 values above the threshold
    cand = np.random.default_rng(7003).standard_normal((400, 3, ANALOG_C))
    Xq = np.empty((ANALOG_TQ, 3, ANALOG_C))
    for c in range(ANALOG_C):
        ne = (y[ao.knn(X[:, :, c], cand[:, :, c], 24)[1], c] > thresh).sum(axis=1)
        Xq[:, :, c] = cand[(ne >= 2) & (ne <= 4), :, c][:ANALOG_TQ]
    st = ctx.analog_fit(X, y)
    share = check_analog(ctx, st, X, y, Xq, 24, worst, "F=3 k=24 thresh", thresh=thresh)
    assert share <= MAX_LEFT_OUT
    print(f"analogreg thresh: largest error / (eps kappa) = {worst.ratio:.1f} at {worst.where}, {share:.1%} left out (K = {lo.K:.0f})")
