"""GPU parity: GroupedRegressor (csrc/sd_grouped.hip through the C ABI, GroupedGridModel, GroupedRegressor and PointWiseDownscaler)
against goldens recorded from the reference (tests/golden/g22_grouped.npz) and the NumPy restatement (tests/_grouped_oracle.py).

Tolerance: the project's own for least squares, rtol 1e-9 of the expected field's std (tests/test_gpu_linreg.py)."""
import pickle

import numpy as np
import pandas as pd
import pytest

import _grouped_oracle as go
from _cases import assert_close, load

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


@pytest.fixture(scope="module")
def g():
    return load("g22_grouped")


def doy(x):
    return x.dayofyear


def case(g, c):
    index = pd.date_range(str(g[f"{c}_start"]), periods=len(g[f"{c}_X"]))
    if c == "c7":
        index_q = pd.date_range(str(g["c7_qstart"]), periods=len(g["c7_Xq"]))
        return index, g[f"{c}_X"], g[f"{c}_y"], int(g[f"{c}_window"]), index_q, g["c7_Xq"]
    return index, g[f"{c}_X"], g[f"{c}_y"], int(g[f"{c}_window"]), index, g[f"{c}_X"]


CASES = ["c1", "c2", "c3", "c4", "c5", "c6", "c7"]


@pytest.mark.parametrize("c", CASES)
def test_goldens_through_the_abi(ctx, g, c):
    index, X, y, w, index_q, Xq = case(g, c)
    key, n = go.doy_keys(index)
    K = y.shape[1]
    st = ctx.grouped_fit(np.repeat(X[:, :, None], K, axis=2), y, key, n, w)
    e = st.export()
    assert e["status"].tolist() == [0] * K and e["fitted"].all() and e["window"] == w
    out, status = ctx.grouped_predict(st, np.repeat(Xq[:, :, None], K, axis=2), go.doy_keys(index_q)[0])
    assert (status == 0).all()
    print(c, "pred err / std", np.abs(out - g[f"{c}_pred"]).max() / np.std(g[f"{c}_pred"]))
    assert_close(out, g[f"{c}_pred"], rtol=RTOL, what=f"{c} pred")
    assert_close(e["coef"].transpose(0, 2, 1), g[f"{c}_coef"], rtol=RTOL, scale=float(np.abs(g[f"{c}_coef"]).max()), what=f"{c} coef")
    assert_close(e["intercept"], g[f"{c}_icpt"], rtol=RTOL, scale=float(np.std(g[f"{c}_pred"])), what=f"{c} intercept")
    st.close()


@pytest.mark.parametrize("c", CASES)
@pytest.mark.parametrize("estimator", ["class", "name"])
def test_goldens_through_grouped_regressor(g, c, estimator):
    from sklearn.linear_model import LinearRegression

    from skdownscale_amd import GroupedRegressor, grouping

    index, X, y, w, index_q, Xq = case(g, c)
    cols, targets = [f"f{i}" for i in range(X.shape[1])], [f"t{i}" for i in range(y.shape[1])]
    m = GroupedRegressor(LinearRegression if estimator == "class" else "LinearRegression", grouping.PaddedDOYGrouper, doy,
                         estimator_kwargs={"fit_intercept": True, "n_jobs": 2}, fit_grouper_kwargs={"window": w})
    assert m.fit(pd.DataFrame(X, index=index, columns=cols), pd.DataFrame(y, index=index, columns=targets)) is m
    n = int(index.dayofyear.max())
    assert m.targets_ == targets and list(m.estimators_) == list(range(1, n + 1))
    assert m.estimators_[1].coef_.shape == (len(targets), len(cols)) and m.estimators_[1].intercept_.shape == (len(targets),)
    out = m.predict(pd.DataFrame(Xq, index=index_q, columns=cols))
    assert isinstance(out, np.ndarray) and out.shape == (len(Xq), len(targets))
    assert_close(out, g[f"{c}_pred"], rtol=RTOL, what=f"{c} pred")
    coef = np.stack([m.estimators_[k].coef_ for k in range(1, n + 1)])
    assert_close(coef, g[f"{c}_coef"], rtol=RTOL, scale=float(np.abs(g[f"{c}_coef"]).max()), what=f"{c} coef_")
    if c == "c6":
        assert (coef[:, :, 1] == 0.0).all()  # the constant feature: sklearn's minimum-norm answer
    m2 = pickle.loads(pickle.dumps(m))
    assert not hasattr(m2, "_grid")
    assert np.array_equal(m2.predict(pd.DataFrame(Xq, index=index_q, columns=cols)), out)


def test_key_error_of_the_reference(g):
    from sklearn.linear_model import LinearRegression

    from skdownscale_amd import GroupedRegressor, grouping

    rng = np.random.default_rng(5)
    index = pd.date_range("2019-01-01", periods=365)
    X = pd.DataFrame({"foo": rng.normal(size=365)}, index=index)
    m = GroupedRegressor(LinearRegression, grouping.PaddedDOYGrouper, doy, fit_grouper_kwargs={"window": 5}).fit(X, X + 2)
    with pytest.raises(KeyError) as ei:
        m.predict(pd.DataFrame({"foo": np.zeros(366)}, index=pd.date_range("2020-01-01", periods=366)))
    assert str(ei.value) == str(g["c7_keyerror"]) and ei.value.args[0] == 366  # (the key as pandas holds it: np.int64)


def random_grid(T, F, C, seed, start="1990-01-01"):
    rng = np.random.default_rng(seed)
    index = pd.date_range(start, periods=T)
    seas = 10 * np.sin(2 * np.pi * np.asarray(index.dayofyear) / 365.25)
    X = 280 + seas[:, None, None] + 3 * rng.standard_normal((T, F, C))
    wts = rng.standard_normal((F, C))
    y = np.einsum("tfc,fc->tc", X - 280, wts) + 275 + 1.1 * seas[:, None] + rng.standard_normal((T, C))
    return index, X, y


@pytest.mark.parametrize("F", [1, 3, 8])
@pytest.mark.parametrize("window", [0, 5, 15])
@pytest.mark.parametrize("resident", [False, True])
def test_grid_vs_oracle(ctx, F, window, resident):
    """Cell tiles with a ragged last tile, a masked and a non-finite cell; window 0 runs on month keys with a key (12) that never
    occurs, the windows 5 and 15 on the days of year of a record that starts in mid-year."""
    from skdownscale_amd import _lib

    T, Tq, C = 1500, 700, 70
    index, X, y = random_grid(T, F, C, 100 * F + window, start="1990-04-11")
    index_q, Xq, _ = random_grid(Tq, F, C, 7 + F + window, start="2001-02-03")
    X[0, 0, 2] = np.nan        # masked cell (core.py:35-37)
    y[T // 2, 4] = np.inf      # non-finite target
    X[T // 3, F - 1, 9] = np.nan
    if window == 0:
        key, n, key_q = np.asarray(index.month) - 1, 13, np.asarray(index_q.month) - 1
    else:
        (key, n), key_q = go.doy_keys(index), go.doy_keys(index_q)[0]
    if resident:
        st = ctx.grouped_fit(ctx.to_device(X), ctx.to_device(y), key, n, window)
        out, status = ctx.grouped_predict(st, ctx.to_device(Xq), key_q)
        out = out.to_host()
    else:
        st = ctx.grouped_fit(X, y, key, n, window)
        out, status = ctx.grouped_predict(st, Xq, key_q)
    expected_status = np.zeros(C, np.int32)
    expected_status[2], expected_status[4], expected_status[9] = _lib.CELL_MASKED, _lib.CELL_NONFINITE, _lib.CELL_NONFINITE
    assert np.array_equal(status, expected_status)
    e = st.export()
    assert np.array_equal(e["status"], expected_status)
    assert e["fitted"].tolist() == ([True] * 12 + [False] if window == 0 else [True] * n)
    eout, ecoef, eicpt = go.grid(X, y, key, n, window, Xq, key_q, skip=(2, 4, 9))
    print(F, window, resident, "pred err / std", np.nanmax(np.abs(out - eout)) / np.nanstd(eout))
    assert_close(out, eout, rtol=RTOL, what="pred")
    assert_close(e["coef"], ecoef, rtol=RTOL, scale=float(np.nanmax(np.abs(ecoef))), what="coef")
    assert_close(e["intercept"], eicpt, rtol=RTOL, scale=float(np.nanstd(eout)), what="intercept")
    if window == 0:
        with pytest.raises(ValueError, match="no fitted model for key 12"):
            ctx.grouped_predict(st, Xq, np.where(np.arange(Tq) % 50 == 7, 12, key_q))
    with pytest.raises(ValueError, match=f"no fitted model for key {n}"):
        ctx.grouped_predict(st, Xq, np.where(np.arange(Tq) == 3, n, key_q))
    st.close()


def test_dev_entry_with_a_row_pitch(ctx):
    """the _dev entries on column blocks of wider resident fields (leading dimension > C)"""
    T, F, C, window = 900, 2, 100, 5
    index, X, y = random_grid(T, F, C, 11)
    key, n = go.doy_keys(index)
    dX, dy = ctx.to_device(X), ctx.to_device(y)
    whole = ctx.grouped_fit(dX, dy, key, n, window)
    out_whole, _ = ctx.grouped_predict(whole, dX, key)
    out_whole = out_whole.to_host()
    block = ctx.grouped_fit(dX.cells(30, 97), dy.cells(30, 97), key, n, window)
    dout = ctx.empty((T, C))
    dout.copy_from_host(np.full((T, C), -1.0))
    ctx.grouped_predict(block, dX.cells(30, 97), key, out=dout.cells(30, 97))
    got = dout.to_host()
    assert np.array_equal(got[:, 30:97], out_whole[:, 30:97])  # a cell's result does not depend on its neighbours or its tile
    assert (got[:, :30] == -1.0).all() and (got[:, 97:] == -1.0).all()  # nothing written outside the view
    assert np.array_equal(whole.export()["coef"][:, :, 30:97], block.export()["coef"])
    host = ctx.grouped_fit(X[:, :, 30:97], y[:, 30:97], key, n, window)
    assert np.array_equal(host.export()["coef"], block.export()["coef"])


def test_window_zero_on_months_is_twelve_regressions(ctx):
    from skdownscale_amd import GroupedGridModel, RegressionGridModel
    from skdownscale_amd.groupers import MONTH_GROUPER

    T, F, C = 2200, 2, 75
    index, X, y = random_grid(T, F, C, 3)
    gm = GroupedGridModel(0, ctx=ctx, grouper=MONTH_GROUPER).fit(X, y, index)
    assert gm.labels_.tolist() == list(range(1, 13)) and gm.fitted_.all()
    out, status = gm.predict(X, index)
    e = gm.export()
    for month in range(1, 13):
        sel = np.asarray(index.month) == month
        rg = RegressionGridModel(ctx=ctx).fit(np.ascontiguousarray(X[sel]), np.ascontiguousarray(y[sel]))
        re = rg.export()
        assert_close(e["coef"][month - 1], re["coef"], rtol=RTOL, what=f"coef month {month}")
        assert_close(e["intercept"][month - 1], re["intercept"], rtol=RTOL, scale=float(np.std(y)), what=f"intercept month {month}")
        rout, _ = rg.predict(np.ascontiguousarray(X[sel]))
        assert_close(out[sel], rout[:, 0, :], rtol=RTOL, what=f"pred month {month}")


def test_export_import_and_pickle_are_bit_identical(ctx):
    from skdownscale_amd import GroupedGridModel

    T, F, C = 1200, 3, 66
    index, X, y = random_grid(T, F, C, 8)
    X[0, 0, 5] = np.nan
    gm = GroupedGridModel(7, ctx=ctx).fit(X, y, index)
    out, status = gm.predict(X, index)
    e = gm.export()
    assert e["coef"].shape == (366, F, C) and e["intercept"].shape == (366, C) and e["labels"].tolist() == list(range(1, 367))
    st2 = ctx.grouped_import(e)
    key = go.doy_keys(index)[0]
    out2, status2 = ctx.grouped_predict(st2, X, key)
    assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(status, status2)
    e2 = st2.export()
    for k in ("coef", "intercept", "fitted", "status"):
        assert np.array_equal(e[k], e2[k], equal_nan=True), k
    gm3 = pickle.loads(pickle.dumps(gm))
    out3, _ = gm3.predict(X, index)
    assert np.array_equal(out, out3, equal_nan=True)
    dout = ctx.empty((T, C))
    res, _ = gm.predict(ctx.to_device(X), index, out=dout)
    assert res is dout and np.array_equal(dout.to_host(), out, equal_nan=True)


# ---- PointWiseDownscaler ----
def c9_grid(g, chunks=None):
    from skdownscale_amd import GridArray

    index = pd.date_range(str(g["c9_start"]), periods=len(g["c9_X"]))
    coords = {"time": index, "variable": np.array(["f0", "f1"]), "cell": np.arange(6)}
    X = GridArray(g["c9_X"], ("time", "variable", "cell"), coords)
    y = GridArray(g["c9_y"], ("time", "cell"), {"time": index, "cell": np.arange(6)})
    return (X.chunk(chunks), y.chunk(chunks)) if chunks else (X, y)


def c9_model(g):
    from sklearn.linear_model import LinearRegression

    from skdownscale_amd import GroupedRegressor, PointWiseDownscaler, grouping

    return PointWiseDownscaler(GroupedRegressor(LinearRegression, grouping.PaddedDOYGrouper, doy, fit_grouper_kwargs={"window": int(g["c9_window"])}))


def test_pointwise_whole_chunked_and_the_reference(g):
    X, y = c9_grid(g)
    pw = c9_model(g)
    pw.fit(X, y)
    whole = pw.predict(X).values
    assert whole.shape == (len(g["c9_X"]), 6) and np.isnan(whole[:, 2]).all()
    assert_close(whole, g["c9_pred"], rtol=RTOL, what="c9 pred")
    Xc, yc = c9_grid(g, {"cell": 4})
    pwc = c9_model(g)
    pwc.fit(Xc, yc)
    assert np.array_equal(np.asarray(pwc.predict(Xc).values), whole, equal_nan=True)
    coef, icpt = pw.get_attr("coef_"), pw.get_attr("intercept_")
    assert coef.dims == ("group", "variable", "cell") and icpt.dims == ("group", "cell") and list(coef.coords["group"]) == list(range(1, 367))
    assert_close(coef.values, g["c9_coef"], rtol=RTOL, scale=float(np.nanmax(np.abs(g["c9_coef"]))), what="c9 coef_")
    assert_close(icpt.values, g["c9_icpt"], rtol=RTOL, scale=float(np.nanstd(g["c9_pred"])), what="c9 intercept_")
    pw2 = pickle.loads(pickle.dumps(pw))
    assert np.array_equal(pw2.predict(X).values, whole, equal_nan=True)
    est = pw._cell_model(4, {})
    assert est.estimators_[17].coef_.shape == (1, 2) and np.array_equal(est.estimators_[17].coef_[0], coef.values[16, :, 4])
    assert pw._cell_model(2, {}) is None


def test_pointwise_errors(g):
    from sklearn.linear_model import LinearRegression, Ridge

    from skdownscale_amd import GridArray, GroupedRegressor, PointWiseDownscaler, grouping

    X, y = c9_grid(g)
    w = {"window": 10}
    with pytest.raises(NotImplementedError, match="LinearRegression"):
        PointWiseDownscaler(GroupedRegressor(Ridge, grouping.PaddedDOYGrouper, doy, fit_grouper_kwargs=w)).fit(X, y)
    with pytest.raises(NotImplementedError, match="estimator_kwargs"):
        PointWiseDownscaler(GroupedRegressor(LinearRegression, grouping.PaddedDOYGrouper, doy, estimator_kwargs={"positive": True},
                                             fit_grouper_kwargs=w)).fit(X, y)
    with pytest.raises(NotImplementedError, match="overlapping"):
        PointWiseDownscaler(GroupedRegressor(LinearRegression, OverlappingHalves, doy)).fit(X, y)
    pw = c9_model(g)
    pw.fit(X, y)
    index_q = pd.date_range("2021-01-01", periods=40)
    Xq = GridArray(g["c9_X"][:40], ("time", "variable", "cell"), {"time": index_q, "variable": np.array(["f0", "f1"]), "cell": np.arange(6)})
    assert pw.predict(Xq).values.shape == (40, 6)
    bad = g["c9_X"].copy()
    bad[300, 1, 4] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        c9_model(g).fit(GridArray(bad, X.dims, X.coords), y)


# ---- other groupers and estimators on a single series ----
class MonthGroups:
    """disjoint groups: one per calendar month"""

    def __init__(self, index):
        month = np.asarray(index.month)
        self.groups = {int(m): np.nonzero(month == m)[0] for m in np.unique(month)}


class OverlappingHalves:
    """two overlapping groups keyed like the days of year 1 and 2"""

    def __init__(self, index):
        n = len(index)
        self.groups = {1: np.arange(0, 2 * n // 3), 2: np.arange(n // 3, n)}


def test_disjoint_grouper_runs_on_the_engine():
    from sklearn.linear_model import LinearRegression

    from skdownscale_amd import GroupedRegressor
    from skdownscale_amd.groupers import MONTH_GROUPER

    index, X, y = random_grid(1000, 2, 1, 4)
    Xd, yd = pd.DataFrame(X[:, :, 0], index=index, columns=["a", "b"]), pd.DataFrame(y, index=index, columns=["t"])
    m = GroupedRegressor(LinearRegression, MonthGroups, MONTH_GROUPER).fit(Xd, yd)
    assert m._engine == {"window": 0} and list(m.estimators_) == list(range(1, 13))
    out = m.predict(Xd)
    exp = np.empty_like(out)
    for month in range(1, 13):
        sel = np.asarray(index.month) == month
        lr = LinearRegression().fit(Xd[sel], yd[sel])
        exp[sel] = lr.predict(Xd[sel])
        assert_close(m.estimators_[month].coef_, lr.coef_, rtol=RTOL, what=f"coef_ month {month}")
    assert_close(out, exp, rtol=RTOL, what="monthly models")


def test_overlapping_grouper_runs_the_host_loop():
    from sklearn.linear_model import LinearRegression

    from skdownscale_amd import GroupedRegressor

    index = pd.DatetimeIndex(["2001-01-01", "2001-01-02"] * 30)  # keys 1 and 2 only
    rng = np.random.default_rng(0)
    Xd = pd.DataFrame({"a": rng.normal(size=60)}, index=index)
    yd = 3 * Xd.rename(columns={"a": "t"}) + 1
    m = GroupedRegressor(LinearRegression, OverlappingHalves, doy).fit(Xd, yd)
    assert isinstance(m.estimators_[1], LinearRegression) and not hasattr(m, "_engine")
    assert_close(m.predict(Xd), yd.values, rtol=RTOL, what="host loop")


def test_quantile_mapping_estimator_fails_like_the_reference(g):
    """QuantileMappingReressor predicts (k,) into the (k, 1) slot of grouping.py:101: the reference's ValueError is kept"""
    from skdownscale_amd import GroupedRegressor, QuantileMappingReressor, grouping

    index, X, y, w, _, _ = case(g, "c1")
    Xd, yd = pd.DataFrame(X, index=index, columns=["foo"]), pd.DataFrame(y, index=index, columns=["bar"])
    m = GroupedRegressor(QuantileMappingReressor, grouping.PaddedDOYGrouper, doy, fit_grouper_kwargs={"window": w}).fit(Xd, yd)
    with pytest.raises(ValueError, match="shape mismatch"):
        m.predict(Xd)
