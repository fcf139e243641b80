"""ZScoreRegressor on the MI355X (csrc/sd_zscore.hip) against the NumPy + pandas oracle (tests/_zscore_oracle.py).

Tolerances: the fit statistics and the predict output to rtol 1e-9.  pandas' own sliding variance drifts from the exact
window std by up to ~6e-9 relative on a 14 600-step series, and by ~3e-8 absolute on narrow windows, so the predict std fields
are compared to 1e-7 (the output does not carry that drift: the std enters it once as a divisor and once as a factor).  Where
the drift has collapsed pandas' variance to exactly 0 on a window that is not constant (pandas_collapse: at most one sample in
a thousand), pandas' output is NaN and the engine's is the finite value of the true std; those positions are left out."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _zscore_oracle as zo  # noqa: E402

pytestmark = pytest.mark.gpu

REF_TIME = pd.date_range(start="2018-01-01", end="2020-01-01")
CALENDARS = {
    "ref_2018_2020": REF_TIME,
    "daily_40y_leap": pd.date_range("1980-01-01", periods=40 * 365 + 10, freq="D"),
    "monthly_480": pd.date_range(periods=480, start="1950", freq="MS"),
    "days_100": pd.date_range("2001-03-01", periods=100, freq="D"),
}


def close(got, exp, rtol=1e-9, atol_rel=1e-12):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), "NaN positions differ"
    assert np.array_equal(np.isinf(got), np.isinf(exp)), "inf positions differ"
    f = np.isfinite(exp)
    scale = np.max(np.abs(exp[f])) if f.any() else 1.0
    np.testing.assert_allclose(got[f], exp[f], rtol=rtol, atol=atol_rel * scale)


def pandas_collapse(values, w, stdi):
    """positions where pandas' sliding variance has collapsed to exactly 0 on a window that is not constant (its running
    Welford sums carry more rounding than the window's spread); the engine returns the window's true small std there"""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    lo, hi = w // 2, (w - 1) // 2
    out = np.zeros(n, dtype=bool)
    for t in np.flatnonzero(np.asarray(stdi) == 0.0):
        win = v[t - lo:t + hi + 1]
        out[t] = np.ptp(win) != 0.0
    assert out.sum() <= max(2, n // 1000), "more pandas collapses than rounding explains"
    return out


def close_predict(out, eout, Xp, w, stdi):
    keep = ~pandas_collapse(Xp, w, stdi)
    close(np.asarray(out)[keep], np.asarray(eout)[keep])


def check_fit(model, exp):
    for attr, key in (("shift_", "shift"), ("scale_", "scale")):
        s = getattr(model, attr)
        assert s.index.name == "day" and np.array_equal(s.index.values, exp[key].index.values)
        close(s.values, exp[key].values)
    for key in ("X_mean", "X_std", "y_mean", "y_std"):
        close(model.fit_stats_dict_[key].values, exp[key].values)


def frame(values, index, name="foo"):
    return pd.DataFrame({name: values}, index=index)


@pytest.mark.parametrize("cal", sorted(CALENDARS))
@pytest.mark.parametrize("w", [1, 2, 30, 31, 61])
def test_single_estimator_against_oracle(cal, w):
    from skdownscale_amd import ZScoreRegressor

    index = CALENDARS[cal]
    rng = np.random.default_rng(len(index) * 100 + w)
    doy = np.asarray(index.dayofyear, dtype=float)
    X = 10 + 5 * np.sin(2 * np.pi * doy / 365.25) + rng.normal(0, 1, len(index))
    y = 12 + 6 * np.sin(2 * np.pi * doy / 365.25) + rng.normal(0, 1.5, len(index))
    exp = zo.fit(X, y, index, w)
    if len(exp["shift"]) == 0:
        with pytest.raises(NotImplementedError):
            ZScoreRegressor(w).fit(frame(X, index), frame(y, index))
        return
    m = ZScoreRegressor(w).fit(frame(X, index), frame(y, index))
    check_fit(m, exp)
    n = len(index) if min(len(index), 364) <= len(exp["shift"]) else len(exp["shift"])
    Xp = X[:n] + 0.5
    out = m.predict(frame(Xp, index[:n]))
    eout, estats = zo.predict(Xp, index[:n], exp["shift"], exp["scale"], w)
    assert list(out.columns) == ["foo"] and out.index.equals(index[:n])
    keep = ~pandas_collapse(Xp, w, estats["stdi"].values)
    close(out["foo"].values[keep], eout.values[keep])
    for k in ("meani", "meanf"):
        close(m.predict_stats_dict_[k].values, estats[k].values)
    for k in ("stdi", "stdf"):
        close(m.predict_stats_dict_[k].values[keep], estats[k].values[keep], rtol=1e-7, atol_rel=1e-7)


def test_expansion_past_the_fit_raises():
    from skdownscale_amd import ZScoreRegressor

    idx = pd.date_range("2001-01-01", periods=400)
    m = ZScoreRegressor().fit(frame(np.arange(100.0) ** 0.5, idx[:100]), frame(np.arange(100.0), idx[:100]))
    with pytest.raises(IndexError):
        m.predict(frame(np.arange(400.0), idx))


def test_duplicate_days_raise():
    from skdownscale_amd import ZScoreRegressor

    idx = pd.date_range("2001-01-01", periods=200, freq="12h")
    with pytest.raises(ValueError, match="at most one sample per day"):
        ZScoreRegressor().fit(frame(np.arange(200.0), idx), frame(np.arange(200.0), idx))


# ---- the reference's own tests (test/test_pointwise_models.py:236-299), on the engine ----
def test_reference_scale():
    from skdownscale_amd import ZScoreRegressor

    X = np.linspace(0, 1, len(REF_TIME))
    m = ZScoreRegressor().fit(frame(X, REF_TIME.rename("index")), frame(2 * X, REF_TIME.rename("index")))
    assert list(m.scale_.index) == list(range(1, 365))
    np.testing.assert_allclose(m.scale_, np.full(364, 2.0))


def test_reference_shift():
    from skdownscale_amd import ZScoreRegressor

    n = len(REF_TIME)
    m = ZScoreRegressor().fit(frame(np.zeros(n), REF_TIME), frame(np.ones(n), REF_TIME))
    np.testing.assert_allclose(m.shift_, np.ones(364))


def test_reference_predict():
    from skdownscale_amd import ZScoreRegressor

    X = np.linspace(0, 1, len(REF_TIME))
    m = ZScoreRegressor()
    days = pd.Index(np.arange(1, 365), name="day")
    m.shift_ = pd.Series(np.zeros(364), index=days, name="foo")
    m.scale_ = pd.Series(np.ones(364), index=days, name="foo")
    out = m.predict(frame(X, REF_TIME))
    exp = X.copy()
    exp[:15] = np.nan
    exp[-15:] = np.nan
    np.testing.assert_allclose(out["foo"].values, exp)


def test_ndarray_input_fabricates_an_index():
    from skdownscale_amd import ZScoreRegressor

    rng = np.random.default_rng(3)
    X, y = rng.normal(size=(480, 1)), rng.normal(size=(480, 1))
    with pytest.warns(UserWarning, match="making one up"):
        m = ZScoreRegressor().fit(X, y)
    exp = zo.fit(X[:, 0], y[:, 0], pd.date_range(periods=480, start="1950", freq="MS"))
    assert len(m.shift_) == 21
    check_fit(m, exp)


# ---- numerics ----
@pytest.mark.parametrize("field", ["seasonal", "offset"])
def test_numerics_against_plain_sums(field):
    from skdownscale_amd import ZScoreRegressor

    index = pd.date_range("1980-01-01", periods=14600)
    rng = np.random.default_rng(11)
    doy = np.asarray(index.dayofyear, dtype=float)
    if field == "seasonal":
        X = 280 + 15 * np.sin(2 * np.pi * doy / 365.25) + rng.normal(0, 1e-3, len(index))
    else:
        X = 1e4 + rng.normal(0, 1e-2, len(index))
    y = X * 1.01 + rng.normal(0, 1e-3, len(index))
    exp = zo.fit(X, y, index)
    m = ZScoreRegressor().fit(frame(X, index), frame(y, index))
    close(m.fit_stats_dict_["X_std"].values, exp["X_std"].values)
    close(m.scale_.values, exp["scale"].values)
    if field == "seasonal":
        return
    # on the offset field a kernel that summed x and x^2 would miss this tolerance on the same windows
    lab, _, std = zo.fit_stats(X, index, 31)
    days, day_idx = np.unique(doy, return_inverse=True)
    sums = np.array([[X[day_idx == d].sum(), (X[day_idx == d] ** 2).sum(), (day_idx == d).sum()] for d in range(len(days))])
    ext = np.concatenate([sums[-16:], sums, sums[:15]])
    win = np.array([ext[p - 15:p + 16].sum(axis=0) for p in range(16, len(ext) - 16)])
    plain = np.sqrt(np.maximum(win[:, 1] / win[:, 2] - (win[:, 0] / win[:, 2]) ** 2, 0))
    assert np.max(np.abs(plain - std) / std) > 1e-9


def test_constant_windows_match_pandas():
    from skdownscale_amd import ZScoreRegressor

    index = pd.date_range("1980-01-01", periods=14600)
    rng = np.random.default_rng(5)
    X = np.where(rng.random(len(index)) < 0.4, rng.gamma(2.0, 3.0, len(index)), 0.0)
    y = np.where(rng.random(len(index)) < 0.5, rng.gamma(2.0, 4.0, len(index)), 0.0)
    for s in range(100, 14000, 1500):  # dry spells of 31 .. 80 days
        X[s:s + 31 + s % 50] = 0.0
    X[7000:7040] = 2.5  # and a constant wet one
    X[np.asarray(index.dayofyear) == 40] = 0.0  # the same day dry in every year ...
    y[np.asarray(index.dayofyear) == 40] = 0.0
    X[(np.asarray(index.dayofyear) >= 200) & (np.asarray(index.dayofyear) <= 240)] = 0.0  # ... and whole all-zero day windows
    exp = zo.fit(X, y, index)
    m = ZScoreRegressor().fit(frame(X, index), frame(y, index))
    assert np.array_equal(np.isnan(m.scale_.values), np.isnan(exp["scale"].values))
    assert np.array_equal(np.isinf(m.scale_.values), np.isinf(exp["scale"].values))
    assert np.isnan(exp["scale"].values).any() or np.isinf(exp["scale"].values).any()
    out = m.predict(frame(X, index))
    eout, estats = zo.predict(X, index, m.shift_, m.scale_)
    keep = ~pandas_collapse(X, 31, estats["stdi"].values)
    assert np.array_equal(np.isnan(out["foo"].values[keep]), np.isnan(eout.values[keep]))
    assert np.array_equal(m.predict_stats_dict_["stdi"].values[keep] == 0.0, estats["stdi"].values[keep] == 0.0)
    close(out["foo"].values[keep], eout.values[keep])


# ---- PointWiseDownscaler ----
@pytest.fixture(scope="module")
def grid():
    from skdownscale_amd import GridArray

    index = pd.date_range("1980-01-01", periods=14600)
    rng = np.random.default_rng(21)
    doy = np.asarray(index.dayofyear, dtype=float)
    base = 15 + 10 * np.sin(2 * np.pi * doy / 365.25)
    X = base[:, None, None] + rng.normal(0, 3, (len(index), 16, 16))
    y = 1.1 * base[:, None, None] - 1 + rng.normal(0, 4, (len(index), 16, 16))
    Xp = base[:, None, None] + 0.7 + rng.normal(0, 3.5, (len(index), 16, 16))
    X[:, 3, 5] = np.nan
    X[:, 11, 0] = np.nan
    coords = {"time": index, "lat": np.arange(16.0), "lon": np.arange(16.0)}

    def ga(v):
        return GridArray(v, ("time", "lat", "lon"), coords)

    return dict(index=index, X=X, y=y, Xp=Xp, ga=ga)


def fitted(grid, dtype=np.float64, chunks=None):
    from skdownscale_amd import PointWiseDownscaler, ZScoreRegressor

    X, y = grid["ga"](grid["X"].astype(dtype)), grid["ga"](grid["y"].astype(dtype))
    if chunks:
        X, y = X.chunk(chunks), y.chunk(chunks)
    pw = PointWiseDownscaler(ZScoreRegressor())
    pw.fit(X, y)
    return pw


def test_pointwise_against_oracle(grid):
    pw = fitted(grid)
    out = pw.predict(grid["ga"](grid["Xp"])).values
    scale = pw.get_attr("scale_").values
    idx = grid["index"]
    for i, j in [(0, 0), (3, 5), (7, 9), (11, 0), (15, 15), (2, 13)]:
        if np.isnan(grid["X"][0, i, j]):
            assert np.isnan(out[:, i, j]).all() and np.isnan(scale[:, i, j]).all()
            continue
        exp = zo.fit(grid["X"][:, i, j], grid["y"][:, i, j], idx)
        close(scale[:, i, j], exp["scale"].values)
        eout, est = zo.predict(grid["Xp"][:, i, j], idx, exp["shift"], exp["scale"])
        close_predict(out[:, i, j], eout.values, grid["Xp"][:, i, j], 31, est["stdi"].values)


def test_pointwise_float32(grid):
    pw = fitted(grid, np.float32)
    res = pw.predict(grid["ga"](grid["Xp"].astype(np.float32)))
    assert res.values.dtype == np.float32
    idx = grid["index"]
    X, y, Xp = (grid[k][:, 4, 4].astype(np.float32).astype(np.float64) for k in ("X", "y", "Xp"))
    exp = zo.fit(X, y, idx)
    eout, est = zo.predict(Xp, idx, exp["shift"], exp["scale"])
    keep = ~pandas_collapse(Xp, 31, est["stdi"].values)
    close(res.values[:, 4, 4][keep], eout.values.astype(np.float32)[keep], rtol=1e-6, atol_rel=1e-6)


def test_pointwise_nan_in_live_cell(grid):
    from skdownscale_amd import PointWiseDownscaler, ZScoreRegressor

    X = grid["X"].copy()
    X[500, 2, 2] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        PointWiseDownscaler(ZScoreRegressor()).fit(grid["ga"](X), grid["ga"](grid["y"]))


def test_pointwise_chunked_is_bit_identical(grid):
    whole = fitted(grid).predict(grid["ga"](grid["Xp"])).values
    chunked = fitted(grid, chunks={"lat": 5, "lon": 7}).predict(grid["ga"](grid["Xp"]).chunk({"lat": 5, "lon": 7})).values
    assert np.array_equal(whole, chunked, equal_nan=True)


def test_pointwise_pickle_and_get_attr(grid):
    from skdownscale_amd import GridArray

    pw = fitted(grid)
    out = pw.predict(grid["ga"](grid["Xp"])).values
    pw2 = pickle.loads(pickle.dumps(pw))
    assert np.array_equal(pw2.predict(grid["ga"](grid["Xp"])).values, out, equal_nan=True)
    shift = pw.get_attr("shift_")
    assert shift.dims == ("day", "lat", "lon") and list(shift.coords["day"]) == list(range(1, 366))
    K = shift.shape[0]
    tmpl = GridArray(np.zeros((K, 16, 16)), ("day", "lat", "lon"), {"day": np.arange(1, K + 1), "lat": np.arange(16.0), "lon": np.arange(16.0)})
    with_t = pw.get_attr("scale_", template_output=tmpl)
    assert np.array_equal(with_t.values, pw.get_attr("scale_").values, equal_nan=True)
    est = pw._cell_model(16 * 4 + 4, {})
    exp = zo.fit(grid["X"][:, 4, 4], grid["y"][:, 4, 4], grid["index"])
    check_fit(est, exp)


# ---- 100 000 resident cells ----
def test_resident_grid_and_cell_alone_bit_identical():
    from skdownscale_amd import synth
    from skdownscale_amd.engine import Context
    from skdownscale_amd.zscore import ZScoreGridModel

    ctx = Context(0)
    T, C = 14600, 100_000
    index = synth.daily_calendar(T)
    tabs = synth.tas_tables(index)
    fields = {}
    for name in ("X_hist", "y_obs", "X_fut"):
        d = ctx.empty((T, C))
        t = tabs[name]
        ctx.synth_fill(d, synth.GAUSS, 7, t["stream"], c_full=C, base=t["base"], amp=t["amp"], cell_scale=t["cell_scale"])
        fields[name] = d
    gm = ZScoreGridModel(31, ctx=ctx).fit(fields["X_hist"], fields["y_obs"], index)
    assert (gm.status_ == 0).all()
    out, status, _ = gm.predict(fields["X_fut"])
    rows = 800
    head = np.empty((rows, C))
    ctx.lib.sd_memcpy_d2h(ctx.handle, head.ctypes.data_as(ctypes.c_void_p), out.vptr, head.nbytes)
    e = gm.export()
    cells = np.array([0, 1, 63, 64, 12345, 65536, 99999])
    X, y, Xp = (synth.tas_field(n, 7, index, cells, C) for n in ("X_hist", "y_obs", "X_fut"))
    alone = ZScoreGridModel(31, ctx=ctx)
    alone.fit(np.ascontiguousarray(X), np.ascontiguousarray(y), index)
    a_out, _, _ = alone.predict(np.ascontiguousarray(Xp))
    a_e = alone.export()
    assert np.array_equal(a_e["scale"], e["scale"][:, cells]) and np.array_equal(a_e["shift"], e["shift"][:, cells])
    assert np.array_equal(a_out[:rows], head[:, cells], equal_nan=True)
    for i, c in enumerate(cells[:3]):
        exp = zo.fit(X[:, i], y[:, i], index)
        close(e["scale"][:, c], exp["scale"].values)
        close(e["shift"][:, c], exp["shift"].values, atol_rel=1e-9)
        eout, est = zo.predict(Xp[:, i], index, exp["shift"], exp["scale"])
        close_predict(a_out[:, i], eout.values, Xp[:, i], 31, est["stdi"].values)
    for d in fields.values():
        d.free()
    out.free()
