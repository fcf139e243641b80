"""CPU: the constructed-analog rule restated in tests/_constructed_oracle.py against independent formulations (``np.lexsort`` on a
broadcast distance, ``np.linalg.solve`` on the same Gram matrix), and the Python layer (``ConstructedAnalogs``, ``ConstructedGridArray``,
the engine wrappers) on the stand-in library of tests/_recording_lib.py: what is called with which sizes, keys and exclusion ids, every
refusal and its words, and what stays lazy."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import _constructed_oracle as co
from _recording_lib import RecordingLib, context


def coarse_case(seed=0, Tl=120, Tq=9, Cc=12):
    """the coarse side of the base shape of tests/test_gpu_constructed.py: 280 K fields, column 5 NaN in the library, column 8 weighs 0"""
    rng = np.random.default_rng(seed)
    L = 280.0 + 8.0 * rng.standard_normal((Tl, Cc))
    Q = 280.0 + 8.0 * rng.standard_normal((Tq, Cc))
    wc = np.cos(np.deg2rad(np.linspace(30.0, 60.0, Cc)))
    L[Tl // 3, 5] = np.nan
    wc[8] = 0.0
    return L, Q, wc


def all_days(L, Q):
    z, zq = np.zeros(len(L), np.int32), np.zeros(len(Q), np.int32)
    return dict(key_l=z, key_q=zq, period=366, window=-1, excl_l=z - 1, excl_q=zq - 1)


# ---- the oracle against independent formulations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_selection_equals_lexsort_on_a_broadcast_distance(seed):
    L, Q, wc = coarse_case(seed)
    L[[17, 41, 119]] = L[5]  # four identical days, and a target equal to them: ties
    Q[2] = L[5]
    cols = co.used_columns(L, wc)
    assert cols == [0, 1, 2, 3, 4, 6, 7, 9, 10, 11]
    d = (wc[cols] * (Q[:, None, cols] - L[None, :, cols]) ** 2).sum(axis=-1)  # (pairwise sums: the last bits differ)
    keys = (np.arange(120) * 7) % 366
    cand = co.candidates(keys, keys[:9] + 1, 366, 60, np.arange(120) // 40, np.array([0, 1, 2, -1, 0, 1, 2, -1, 5]))
    for k in (1, 5, 30):
        idx, dist, status = co.select(L, Q, wc, k, keys, keys[:9] + 1, 366, 60, np.arange(120) // 40, np.array([0, 1, 2, -1, 0, 1, 2, -1, 5]))
        for q in range(9):
            t = np.flatnonzero(cand[q])
            assert status[q] == (co.OK if len(t) >= k else co.FEW_CANDIDATES)
            if len(t) < k:
                assert (idx[q] == -1).all() and np.isnan(dist[q]).all()
                continue
            order = t[np.lexsort((t, d[q, t]))][:k]  # by distance, then by day
            assert np.array_equal(idx[q], order)
            assert np.allclose(dist[q], d[q, order], rtol=1e-13, atol=0)
    idx, dist, _ = co.select(L, Q, wc, 5, **all_days(L, Q))
    assert list(idx[2, :4]) == [5, 17, 41, 119] and (dist[2, :4] == 0).all()


def test_candidates_wrap_across_the_year_end():
    key_l, key_q = np.array([364, 2, 100, 366, 1]), np.array([1, 365, 183])
    got = co.candidates(key_l, key_q, 366, 3, [-1] * 5, [-1] * 3)
    want = np.array([[min(abs(a - b), 366 - abs(a - b)) <= 3 for b in key_l] for a in key_q])
    assert np.array_equal(got, want) and got.tolist() == [[True, True, False, True, True], [True, True, False, True, True], [False] * 5]
    assert co.candidates(key_l, key_q, 366, -1, [-1] * 5, [-1] * 3).all()
    assert co.candidates(key_l, key_q, 366, -1, [7, 8, 7, 8, 9], [7, -1, 9]).tolist() == [[False, True, False, True, True], [True] * 5,
                                                                                          [True, True, True, True, False]]


@pytest.mark.parametrize("ridge", [1e-6, 1e-9])
@pytest.mark.parametrize("k", [1, 5, 30, 32])
def test_weights_equal_numpy_solve_within_the_measured_margin(k, ridge):
    worst = 0.0
    for seed in (0, 1, 2):
        L, Q, wc = coarse_case(seed)
        idx, dist, status = co.select(L, Q, wc, k, **all_days(L, Q))
        w, _, _, status = co.weights(L, Q, wc, idx, dist, status, co.REGRESSION, ridge)
        assert (status == co.OK).all()  # k > Cc: the ridge alone makes the Gram matrix definite
        cols = co.used_columns(L, wc)
        for q in range(len(Q)):
            G, b = co.gram(L, Q[q], wc, cols, idx[q])
            assert np.allclose(G, (L[idx[q]][:, cols] * wc[cols]) @ L[idx[q]][:, cols].T, rtol=1e-13)
            ref = np.linalg.solve(co.add_ridge(G, ridge), b)
            worst = max(worst, np.abs(w[q] - ref).max() / np.abs(ref).max())
    print(f"k={k} ridge={ridge:g}: largest relative difference {worst:.3e}, margin {co.SOLVE_RTOL[ridge]:.1e}")
    assert worst <= co.SOLVE_RTOL[ridge]


def test_duplicate_days_solve_with_a_ridge_and_are_singular_without():
    L, Q, wc = coarse_case(1)
    L[[17, 41, 119]] = L[5]
    Q[2] = L[5]
    idx, dist, status = co.select(L, Q, wc, 5, **all_days(L, Q))
    w, _, _, st = co.weights(L, Q, wc, idx, dist, status, co.REGRESSION, 1e-6)
    assert (st == co.OK).all() and np.isfinite(w).all()
    # integers: G[0][0] = 25 has an exact root, the second pivot is exactly 25 - 5 * 5 = 0
    Li = np.round(coarse_case(2, 30, 3, 12)[0][:, :4] - 270.0)
    Li[[3, 11, 20]] = [3.0, 4.0, 0.0, 0.0]
    Qi = np.array([[9.0, 1.0, 4.0, 2.0], [3.0, 4.0, 0.0, 0.0]])
    idx, dist, status = co.select(Li, Qi, np.ones(4), 3, **all_days(Li, Qi))
    assert list(idx[1]) == [3, 11, 20]
    w, idx, dist, st = co.weights(Li, Qi, np.ones(4), idx, dist, status, co.REGRESSION, 0.0)
    assert st[1] == co.SINGULAR and np.isnan(w[1]).all() and (idx[1] == -1).all() and np.isnan(dist[1]).all() and st[0] == co.OK
    assert co.weights(Li, Qi, np.ones(4), *co.select(Li, Qi, np.ones(4), 3, **all_days(Li, Qi)), co.REGRESSION, 1e-6)[3][1] == co.OK


def test_mean_of_one_analog_copies_the_row_and_bad_targets_are_nan_rows():
    L, Q, wc = coarse_case(3)
    Q[4, 0] = np.inf
    Q[5, 5] = np.nan  # an unused column
    F = np.random.default_rng(0).standard_normal((120, 7)).astype(np.float32)
    F[:, 0] = -0.0
    idx, dist, w, status, out = co.constructed(L, Q, wc, F, 1, co.MEAN, 0.0, **all_days(L, Q))
    assert list(status) == [0, 0, 0, 0, co.QUERY_NONFINITE, 0, 0, 0, 0] and np.isnan(out[4]).all() and (idx[4] == -1).all()
    ok = status == co.OK
    assert np.array_equal(out[ok], F[idx[ok, 0]].astype(np.float64)) and not np.signbit(out[ok][:, 0]).any() and (w[ok] == 1.0).all()
    with pytest.raises(ValueError, match="no column is used"):
        co.select(L, Q, np.zeros(12), 1, **all_days(L, Q))


# ---- the Python layer on the stand-in library ---------------------------------------------------------------------------------------
class ScriptedLib(RecordingLib):
    """a RecordingLib whose device-to-host copies deliver ``downloads`` one after the other (zeros once they are used up), and which keeps
    the small host tables handed to sd_ca_select_dev"""

    def __init__(self):
        super().__init__()
        self.downloads, self.tables = [], []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name == "sd_memcpy_d2h":
            def copy(ctx, dst, src, nbytes):
                data = np.ascontiguousarray(self.downloads.pop(0)).tobytes() if self.downloads else bytes(int(nbytes))
                assert len(data) == int(nbytes), (len(data), int(nbytes))
                C.memmove(dst, data, len(data))
                return call(ctx, dst, src, nbytes)
            return copy
        if name == "sd_ca_select_dev":
            def select(*a):
                Tl, Tq, Cc = int(a[3]), int(a[6]), int(a[7])
                read = lambda p, n, t: np.ctypeslib.as_array((t * n).from_address(p.value)).copy()  # noqa: E731
                self.tables.append(dict(wc=read(a[8], Cc, C.c_double), key_l=read(a[10], Tl, C.c_int32), key_q=read(a[11], Tq, C.c_int32),
                                        excl_l=read(a[14], Tl, C.c_int32), excl_q=read(a[15], Tq, C.c_int32)))
                return call(*a)
            return select
        return call


TL, TQ, K = 400, 6, 4
LAT_C, LON_C = np.array([35.0, 40.0, 45.0]), np.array([-110.0, -105.0])
LAT_F, LON_F = np.linspace(33.0, 47.0, 5), np.linspace(-112.0, -103.0, 4)
TIME_L = pd.date_range("1990-12-01", periods=TL, freq="D")
TIME_Q = pd.date_range("2000-12-29", periods=TQ, freq="D")


def arrays(f32=True):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(0)
    coarse = GridArray(280.0 + rng.standard_normal((TL, 3, 2)), ("time", "lat", "lon"), {"time": TIME_L, "lat": LAT_C, "lon": LON_C})
    fine = GridArray((280.0 + rng.standard_normal((TL, 5, 4))).astype(np.float32 if f32 else np.float64), ("time", "lat", "lon"),
                     {"time": TIME_L, "lat": LAT_F, "lon": LON_F})
    target = GridArray(280.0 + rng.standard_normal((TQ, 3, 2)), ("time", "lat", "lon"), {"time": TIME_Q, "lat": LAT_C, "lon": LON_C}, name="tas")
    return coarse, fine, target


def tables(status=None):
    idx = (np.arange(TQ * K, dtype=np.int32).reshape(TQ, K) * 7) % TL
    return [idx, np.ones((TQ, K)), np.zeros(TQ, np.int32) if status is None else np.asarray(status, np.int32), np.full((TQ, K), 0.25)]


def predicted(f32=True, **kw):
    from skdownscale_amd import ConstructedAnalogs

    ctx = context(ScriptedLib())
    coarse, fine, target = arrays(f32)
    ca = ConstructedAnalogs(n_analogs=K, ctx=ctx, **kw).fit(coarse, fine)
    ctx.lib.downloads = tables()
    return ctx, ca, ca.predict(target)


def test_exports():
    import skdownscale_amd
    from skdownscale_amd import _lib
    from skdownscale_amd.timesource import TAKEN_WHOLE

    assert {"ConstructedAnalogs", "ConstructedGridArray"} <= set(skdownscale_amd.__all__)
    assert {"sd_ca_select_dev", "sd_ca_weights_dev", "sd_ca_apply_dev"} <= set(_lib.SIGNATURES)
    assert "constructed" in TAKEN_WHOLE["any"] and "constructed" not in TAKEN_WHOLE["resample"]
    assert (_lib.CA_OK, _lib.CA_QUERY_NONFINITE, _lib.CA_FEW_CANDIDATES, _lib.CA_SINGULAR) == (co.OK, co.QUERY_NONFINITE, co.FEW_CANDIDATES,
                                                                                              co.SINGULAR)
    assert _lib.CA_KINDS == {"regression": co.REGRESSION, "mean": co.MEAN}


def test_predict_calls_select_and_weights_and_stays_lazy():
    from skdownscale_amd import ConstructedGridArray

    ctx, ca, pred = predicted()
    names = [n for n, _ in ctx.lib.log]
    assert names == ["sd_ca_select_dev", "sd_ca_weights_dev"]  # nothing of the fine library is touched
    sel, wgt = ctx.lib.log[0][1], ctx.lib.log[1][1]
    # ctx, L, ld_l, Tl, Q, ld_q, Tq, Cc, wc, k, key_l, key_q, period, window, excl_l, excl_q, idx, dist, status
    assert sel[2:4] == [6, TL] and sel[5:8] == [6, TQ, 6] and sel[9] == K and sel[12:14] == [366, 45]
    assert wgt[2:4] == [6, TL] and wgt[5:8] == [6, TQ, 6] and wgt[9:12] == [K, co.REGRESSION, 1e-6]
    assert wgt[1] == sel[1] and wgt[4] == sel[4] and wgt[12] == sel[16] and wgt[13] == sel[17] and wgt[15] == sel[18]  # one upload each
    t = ctx.lib.tables[0]
    assert np.array_equal(t["key_l"], TIME_L.dayofyear) and np.array_equal(t["key_q"], [364, 365, 366, 1, 2, 3])
    assert (t["excl_l"] == -1).all() and (t["excl_q"] == -1).all()
    assert np.array_equal(t["wc"], np.repeat(np.cos(np.deg2rad(LAT_C)), 2))
    assert isinstance(pred, ConstructedGridArray) and not pred.computed and pred.shape == (TQ, 5, 4) and pred.name == "tas"
    assert pred.dims == ("time", "lat", "lon") and pred.coords["time"] is not None and len(pred.coords["lat"]) == 5
    want = tables()
    assert np.array_equal(ca.analog_index_, want[0]) and np.array_equal(ca.weights_, want[3]) and np.array_equal(ca.status_, want[2])
    assert np.array_equal(ca.analog_distance_, want[1]) and ca.analog_index_.dtype == np.int32
    assert sum(n == "sd_dev_alloc" for n, _ in ctx.lib.traffic) == sum(n == "sd_dev_free" for n, _ in ctx.lib.traffic) == 6  # all freed


def test_keys_exclusions_kind_and_weights():
    ctx, _, _ = predicted(window=None, exclude_same_year=True, kind="mean", ridge=0.5, weights="plain")
    sel, wgt = ctx.lib.log[0][1], ctx.lib.log[1][1]
    assert sel[12:14] == [366, -1] and wgt[10:12] == [co.MEAN, 0.5]
    t = ctx.lib.tables[0]
    assert np.array_equal(t["excl_l"], TIME_L.year) and np.array_equal(t["excl_q"], [2000, 2000, 2000, 2001, 2001, 2001])
    assert (t["wc"] == 1.0).all()
    given = np.arange(6.0).reshape(3, 2)
    ctx, _, _ = predicted(weights=given, window=0)
    assert np.array_equal(ctx.lib.tables[0]["wc"], given.reshape(-1)) and ctx.lib.log[0][1][13] == 0
    ctx, _, _ = predicted(latitude="lon")  # a dim named as the latitude
    assert np.array_equal(ctx.lib.tables[0]["wc"], np.tile(np.cos(np.deg2rad(np.clip(LON_C, -90, 90))), 3))
    ctx, _, _ = predicted(latitude=None)
    assert (ctx.lib.tables[0]["wc"] == 1.0).all()


def test_status_of_a_target_raises_like_the_issue_says():
    from skdownscale_amd import ConstructedAnalogs

    coarse, fine, target = arrays()
    ctx = context(ScriptedLib())
    ca = ConstructedAnalogs(n_analogs=K, window=2, ctx=ctx).fit(coarse, fine)
    ctx.lib.downloads = tables([0, 0, co.FEW_CANDIDATES, co.SINGULAR, co.FEW_CANDIDATES, 0])
    with pytest.raises(ValueError, match=r"step 2 of the target \(2000-12-31 00:00:00\) has fewer than n_analogs=4 candidate days .*window=2"):
        ca.predict(target)
    assert list(ca.status_) == [0, 0, 2, 3, 2, 0]  # the tables of the failed predict stay readable
    ctx.lib.downloads = tables([0, co.QUERY_NONFINITE, 0, co.SINGULAR, 0, 0])
    with pytest.raises(ArithmeticError, match=r"step 3 of the target \(2001-01-01 00:00:00\).*not positive definite with ridge=1e-06"):
        ca.predict(target)
    ctx.lib.downloads = tables([0, co.QUERY_NONFINITE, 0, 0, 0, 0])
    assert not ca.predict(target).computed  # a non-finite target day is a NaN row, not an error


def test_constructor_and_fit_refusals():
    from skdownscale_amd import ConstructedAnalogs, GridArray

    for kw, words in ((dict(n_analogs=0), "n_analogs=0: expected 1 to 32"), (dict(n_analogs=33), "n_analogs=33"), (dict(window=-1), "window=-1"),
                      (dict(window=2.5), "window=2.5"), (dict(kind="best"), "kind='best': expected one of 'regression', 'mean'"),
                      (dict(ridge=-1e-3), "ridge=-0.001"), (dict(ridge=float("nan")), "ridge=nan"), (dict(weights="volume"), "weights='volume'")):
        with pytest.raises(ValueError, match=words):
            ConstructedAnalogs(**kw)
    coarse, fine, target = arrays()
    ca = ConstructedAnalogs(n_analogs=K, ctx=context(ScriptedLib()))
    with pytest.raises(ValueError, match="not fitted"):
        ca.predict(target)
    with pytest.raises(ValueError, match="the fine library: expected a GridArray, got ndarray"):
        ca.fit(coarse, fine.values)
    with pytest.raises(ValueError, match="dim 'time' is not a dim of the coarse library"):
        ca.fit(GridArray(coarse.values, ("t", "lat", "lon"), {}), fine)
    with pytest.raises(ValueError, match="the libraries differ: 400 coarse and 399 fine steps of 'time'"):
        ca.fit(coarse, fine.isel(time=slice(0, 399)))
    shifted = GridArray(fine.values, fine.dims, dict(fine.coords, time=TIME_L[:7].append(TIME_L[7:] + pd.Timedelta(days=1))))
    with pytest.raises(ValueError, match=r"the time coordinates of the libraries differ at step 7: 1990-12-08 00:00:00 and 1990-12-09 00:00:00"):
        ca.fit(coarse, shifted)
    with pytest.raises(ValueError, match="the time coordinate of the coarse library must be a DatetimeIndex, got .* of int64"):
        ca.fit(GridArray(coarse.values, coarse.dims, dict(coarse.coords, time=np.arange(TL))), fine)
    with pytest.raises(ValueError, match="the fine library has no coordinate for dim 'time'"):
        ca.fit(coarse, GridArray(fine.values, fine.dims, {}))
    with pytest.raises(ValueError, match=r"weights: expected an array of the coarse grid's shape \(3, 2\), got shape \(2, 3\)"):
        ConstructedAnalogs(weights=np.ones((2, 3))).fit(coarse, fine)
    with pytest.raises(ValueError, match="latitude='y' is not one of the spatial dims"):
        ConstructedAnalogs(latitude="y").fit(coarse, fine)
    ca.fit(coarse, fine)
    with pytest.raises(ValueError, match=r"the target has dims \('time', 'y', 'x'\); expected \('time', 'lat', 'lon'\) in any order"):
        ca.predict(GridArray(target.values, ("time", "y", "x"), target.coords))
    with pytest.raises(ValueError, match=r"the target has sizes \{'lat': 2, 'lon': 2\} on the coarse grid; the coarse library has \{'lat': 3, 'lon': 2\}"):
        ca.predict(target.isel(lat=slice(0, 2)))
    with pytest.raises(ValueError, match="the time coordinate of the target must be a DatetimeIndex"):
        ca.predict(GridArray(target.values, target.dims, dict(target.coords, time=np.arange(TQ))))
    assert ca._ctx.lib.log == [] and ca._ctx.lib.traffic == []  # nothing reached the library


def test_a_transposed_target_and_a_lazy_coarse_library():
    from skdownscale_amd import ConstructedAnalogs, GridArray

    coarse, fine, target = arrays()
    ctx = context(ScriptedLib())
    flipped = GridArray(np.ascontiguousarray(coarse.values.transpose(2, 0, 1)), ("lon", "time", "lat"), coarse.coords)
    ca = ConstructedAnalogs(n_analogs=K, ctx=ctx).fit(flipped, fine)
    assert ca._coarse["dims"] == ("lon", "lat") and np.array_equal(ca._L, coarse.values.transpose(0, 2, 1).reshape(TL, 6))
    ctx.lib.downloads = tables()
    ca.predict(target)  # dims (time, lat, lon): brought into the library's order
    assert np.array_equal(ctx.lib.tables[0]["wc"], np.tile(np.cos(np.deg2rad(LAT_C)), 2))


@pytest.mark.parametrize("f32", [True, False])
def test_values_apply_the_whole_field_once(f32):
    ctx, ca, pred = predicted(f32)
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    values = pred.values
    assert values.shape == (TQ, 5, 4) and pred.computed
    (name, a), = ctx.lib.log
    # ctx, F, f_is_f32, ld_f, Tl, Cf, idx, weights, Tq, k, q0, q1, out, ld_out
    assert name == "sd_ca_apply_dev" and a[2:6] == [int(f32), 20, TL, 20] and a[8:12] == [TQ, K, 0, TQ] and a[13] == 20
    up = [args[3] for n, args in ctx.lib.traffic if n == "sd_memcpy_h2d"]
    assert up == [TL * 20 * (4 if f32 else 8), TQ * K * 4, TQ * K * 8]  # the fine library as it is stored, and the two tables


def test_isel_stays_lazy_and_selects_cells_of_the_fine_library():
    from skdownscale_amd import ConstructedGridArray

    ctx, ca, pred = predicted()
    win = pred.isel(lat=slice(1, 4), lon=slice(0, 2), time=slice(2, 5))
    assert isinstance(win, ConstructedGridArray) and not win.computed and not pred.computed and win.shape == (3, 3, 2)
    assert np.array_equal(win.analog_index, ca.analog_index_[2:5]) and list(win.coords["time"]) == list(TIME_Q[2:5])
    assert np.array_equal(win.coords["lat"], LAT_F[1:4])
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    win.values
    (name, a), = ctx.lib.log
    assert name == "sd_ca_apply_dev" and a[3:6] == [6, TL, 6] and a[8:12] == [3, K, 0, 3]
    assert [args[3] for n, args in ctx.lib.traffic if n == "sd_memcpy_h2d"][0] == TL * 6 * 4  # only the cells of the window go up
    with pytest.raises(ValueError, match="dim 'x' is not a dim"):
        pred.isel(x=slice(0, 1))
    picked = pred.isel(lat=[0, 2])  # anything but slices is answered on the computed field
    assert not isinstance(picked, ConstructedGridArray) and picked.shape == (TQ, 2, 4) and pred.computed


def test_block_producer_keeps_the_fine_library_resident():
    from skdownscale_amd.timesource import takes_whole

    ctx, ca, pred = predicted()
    assert takes_whole(pred, "any", "time") and not takes_whole(pred, "resample", "time") and not takes_whole(pred, "any", "lat")
    assert pred._block_producer(ctx, "lat") is None
    p = pred._block_producer(ctx, "time")
    assert (p.rows, p.cells, p.dtype, p.uploads) == (TQ, 20, np.float64, False)
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    out = ctx.lib.resident(ctx, "OUT", (TQ, 20))
    for r0, r1 in ((0, 2), (2, 4), (4, 6)):
        p.produce(r0, r1, out=out.rows(r0, r1))
    calls = [a for n, a in ctx.lib.log]
    assert [n for n, _ in ctx.lib.log] == ["sd_ca_apply_dev"] * 3 and [a[10:12] for a in calls] == [[0, 2], [2, 4], [4, 6]]
    assert [a[12] for a in calls] == [("OUT", 0), ("OUT", 40), ("OUT", 80)] and len({a[1] for a in calls}) == 1
    assert sum(n == "sd_memcpy_h2d" for n, _ in ctx.lib.traffic) == 3  # the library and the two tables, once
    pred.values
    assert pred._block_producer(ctx, "time") is None  # computed: its rows are uploaded like any host array's


def test_engine_wrappers_refuse_before_the_library():
    ctx = context(ScriptedLib())
    L, Q, wc = coarse_case()
    for call, words in ((lambda: ctx.ca_select(L, Q[:, :5], wc, 3), r"Q: expected a \[Tq, 12\] field like L"),
                        (lambda: ctx.ca_select(L, Q, wc[:3], 3), "wc: expected 12 column weights"),
                        (lambda: ctx.ca_select(L, Q, wc, 0), r"sd_ca_select: k = 0 lies outside \[1, 32\]"),
                        (lambda: ctx.ca_select(L, Q, wc, 3, key_l=np.zeros(5)), r"key_l: expected one id per day \(120\)"),
                        (lambda: ctx.ca_select(L, Q, wc, 3, excl_q=np.zeros(5)), r"excl_q: expected one id per day \(9\)"),
                        (lambda: ctx.ca_select(L[:0], Q, wc, 3), r"sd_ca_select: bad sizes \(Tl=0, Tq=9, Cc=12\)"),
                        (lambda: ctx.ca_weights(L, Q, wc, np.zeros((9, 3), np.int32), None, None), "idx: expected the int32"),
                        (lambda: ctx.ca_apply(np.zeros((4, 4)), None, None), "F: expected a float32 or float64"),
                        (lambda: ctx.ca_apply(L, None, None), "F: expected")):
        with pytest.raises(ValueError, match=words):
            call()
    assert ctx.lib.log == [] and ctx.lib.traffic == []
    idx, dist, status = ctx.ca_select(L, Q, wc, 3)
    assert (idx.shape, idx.dtype, dist.shape, status.shape, status.dtype) == ((9, 3), np.int32, (9, 3), (9,), np.int32)
    for call, words in ((lambda: ctx.ca_weights(L, Q, wc, idx, dist, status, kind="median"), "kind='median'"),
                        (lambda: ctx.ca_weights(L, Q, wc, idx, dist, status, ridge=-1.0), "ridge = -1, expected a finite factor >= 0"),
                        (lambda: ctx.ca_weights(L, Q, wc, idx, status, status), r"dist: expected a contiguous float64 DeviceArray of shape \(9, 3\)"),
                        (lambda: ctx.ca_weights(L, Q[:4], wc, idx, dist, status), r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)")):
        with pytest.raises(ValueError, match=words):
            call()
    w = ctx.ca_weights(L, Q, wc, idx, dist, status)
    F = ctx.lib.resident(ctx, "F", (120, 7), np.float32)
    with pytest.raises(ValueError, match=r"sd_ca_apply: rows \[3, 3\) lie outside the 9 targets"):
        ctx.ca_apply(F, idx, w, 3, 3)
    with pytest.raises(ValueError, match=r"out: expected a float64 DeviceArray of shape \(2, 7\)"):
        ctx.ca_apply(F, idx, w, 0, 2, out=ctx.lib.resident(ctx, "O", (3, 7)))
    other = context(ScriptedLib())
    with pytest.raises(ValueError, match="sd_ca_apply: `F` belongs to another context"):
        ctx.ca_apply(other.lib.resident(other, "F2", (120, 7)), idx, w)
    assert [n for n, _ in ctx.lib.log] == ["sd_ca_select_dev", "sd_ca_weights_dev"]
