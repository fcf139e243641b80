"""CPU: properties of the localized-analog rule as tests/_localized_oracle.py restates it (full-cover radii reproduce the regional
distance bit for bit, ties, unused cells, rows without analogs), and the Python layer (``LocalizedAnalogs``, ``LocalizedGridArray``, the
engine wrappers) on the stand-in library of tests/_recording_lib.py: ``cell_of``, what is called with which arguments, every refusal and
its words, and what stays lazy."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

import _constructed_oracle as co
import _localized_oracle as lo
from _recording_lib import RecordingLib, context


def coarse_case(seed=0, Tl=120, Tq=9, ny=3, nx=4):
    """the coarse side of the base shape of tests/test_gpu_localized.py: 280 K fields, column 5 NaN once in the library, column 8 weighs 0"""
    rng = np.random.default_rng(seed)
    Cc = ny * nx
    L = 280.0 + 8.0 * rng.standard_normal((Tl, Cc))
    Q = 280.0 + 8.0 * rng.standard_normal((Tq, Cc))
    wc = np.cos(np.deg2rad(np.linspace(30.0, 60.0, Cc)))
    L[Tl // 3, 5] = np.nan
    wc[8] = 0.0
    return L, Q, wc


def regional(L, Q, wc, k):
    z, zq = np.zeros(len(L), np.int32), np.zeros(len(Q), np.int32)
    return lo.select(L, Q, wc, k, z, zq, 366, -1, z - 1, zq - 1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", [(3, 4), (9, 17)])
def test_radii_that_cover_the_grid_give_slot_0_and_the_regional_distance_bit_for_bit(ny, nx):
    L, Q, wc = coarse_case(0, Tq=9 if ny == 3 else 3, ny=ny, nx=nx)
    idx, dist, status = regional(L, Q, wc, 5)
    for radius in ((ny - 1, nx - 1), (ny + 3, nx + 9)):
        slot, lidx, ldist = lo.local(L, Q, wc, idx, ny, nx, *radius)
        assert (slot == 0).all() and (lidx == idx[:, :1]).all()
        assert same_bits(ldist, np.repeat(dist[:, :1], ny * nx, axis=1))  # the local sum is the regional sum in the same order


def test_one_analog_gives_slot_0_and_five_give_at_least_three_distinct_slots_per_target():
    L, Q, wc = coarse_case()
    idx, _, _ = regional(L, Q, wc, 1)
    assert (lo.local(L, Q, wc, idx, 3, 4, 1, 1)[0] == 0).all()
    idx, _, _ = regional(L, Q, wc, 5)
    slot, lidx, ldist = lo.local(L, Q, wc, idx, 3, 4, 1, 1)
    assert all(len(set(row)) >= 3 for row in slot)  # an implementation that always answers slot 0 cannot pass
    assert np.array_equal(lidx, np.take_along_axis(idx, slot, axis=1)) and lidx.dtype == np.int32
    # against an independent formulation: the windowed sum of a broadcast term array (pairwise sums: the last bits differ)
    cols = co.used_columns(L, wc)
    term = np.zeros((9, 5, 12))
    term[:, :, cols] = wc[cols] * (Q[:, None, cols] - L[idx][:, :, cols]) ** 2
    term = term.reshape(9, 5, 3, 4)
    for i in range(3):
        for j in range(4):
            box = term[:, :, max(0, i - 1):i + 2, max(0, j - 1):j + 2].sum(axis=(2, 3))
            assert np.array_equal(box.argmin(axis=1), slot[:, i * 4 + j])
            assert np.allclose(box.min(axis=1), ldist[:, i * 4 + j], rtol=1e-13, atol=0)


def test_ties_go_to_the_lower_slot():
    L, Q, wc = coarse_case(3)
    L[[17, 41, 119]] = L[5]  # four identical days, and a target equal to them
    Q[2] = L[5]
    idx, dist, _ = regional(L, Q, wc, 5)
    assert list(idx[2, :4]) == [5, 17, 41, 119]
    slot, lidx, ldist = lo.local(L, Q, wc, idx, 3, 4, 1, 1)
    assert (slot[2] == 0).all() and (lidx[2] == 5).all() and same_bits(ldist[2], np.zeros(12))
    swapped = idx.copy()
    swapped[2, :4] = [119, 41, 17, 5]  # the slot decides, not the day
    assert (lo.local(L, Q, wc, swapped, 3, 4, 1, 1)[1][2] == 119).all()


def test_a_row_without_analogs_and_an_unused_cell_alone():
    L, Q, wc = coarse_case(4)
    Q[4, 0] = np.inf
    Q[5, 5] = np.nan  # an unused column: no effect
    idx, dist, status = regional(L, Q, wc, 5)
    assert status[4] == co.QUERY_NONFINITE and status[5] == co.OK
    slot, lidx, ldist = lo.local(L, Q, wc, idx, 3, 4, 0, 0)
    assert (lidx[4] == -1).all() and np.isnan(ldist[4]).all() and (slot[4] == -1).all()
    ok = status == co.OK
    assert (slot[ok][:, [5, 8]] == 0).all() and same_bits(ldist[ok][:, [5, 8]], np.zeros((8, 2)))  # +0.0 for every slot, hence slot 0
    assert np.isfinite(ldist[ok]).all() and (lidx[ok] >= 0).all()
    around = lo.local(L, Q, wc, idx, 3, 4, 1, 1)[2]
    assert (around[ok][:, [5, 8]] > 0).all()  # the neighbourhood of an unused cell holds used ones
    with pytest.raises(ValueError, match="no column is used"):
        lo.local(L, Q, np.zeros(12), idx, 3, 4, 1, 1)


def test_synthesis_of_the_oracle():
    rng = np.random.default_rng(0)
    F = rng.standard_normal((6, 5)).astype(np.float32)
    F[:, 0] = -0.0
    L, Q = np.array([[2.0, 0.0]] * 6), np.array([[3.0, 5.0], [8.0, 1.0]])
    lidx = np.array([[4, 1], [2, -1]], np.int32)
    cell_of = np.array([0, 1, -1, 2, 0], np.int32)
    none = lo.local_apply(F, cell_of, lidx)
    assert np.signbit(none[0, 0]) and none[0, 1] == F[1, 1] and none[1, 4] == F[2, 4]  # a copy: -0.0 stays -0.0
    assert np.isnan(none[:, 2:4]).all() and np.isnan(none[1, 1])  # cells outside the coarse grid, a cell without a day
    shift = lo.local_apply(F, cell_of, lidx, L, Q, lo.ADJUST_SHIFT)
    assert shift[0, 4] == np.float64(F[4, 4]) + 1.0 and shift[0, 1] == np.float64(F[1, 1]) + 5.0 and shift[1, 4] == np.float64(F[2, 4]) + 6.0
    scale = lo.local_apply(F, cell_of, lidx, L, Q, lo.ADJUST_SCALE)
    assert scale[0, 4] == np.float64(F[4, 4]) * 1.5 and scale[0, 1] == np.float64(F[1, 1]) and scale[1, 4] == np.float64(F[2, 4]) * 4.0
    cut = lo.local_apply(F, cell_of, lidx, L, Q, lo.ADJUST_SCALE, max_scale=2.0)
    assert cut[0, 4] == scale[0, 4] and cut[1, 4] == np.float64(F[2, 4]) * 2.0
    assert same_bits(lo.local_apply(F, cell_of, lidx, L, Q, lo.ADJUST_SHIFT, q0=1, q1=2), shift[1:2])


# ---- the Python layer on the stand-in library -----------------------------------------------------------------------------------------
class ScriptedLib(RecordingLib):
    """a RecordingLib whose device-to-host copies deliver ``downloads`` one after the other (zeros once they are used up), and which keeps
    the column weights handed to sd_ca_local_dev"""

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
        if name == "sd_ca_local_dev":
            def local(*a):
                n = int(a[7]) * int(a[8])
                self.tables.append(np.ctypeslib.as_array((C.c_double * n).from_address(a[9].value)).copy())
                return call(*a)
            return local
        return call


TL, TQ, K = 400, 6, 4
LAT_C, LON_C = np.array([35.0, 40.0, 45.0]), np.array([-110.0, -105.0])
LAT_F, LON_F = np.linspace(33.0, 47.0, 5), np.linspace(-112.0, -103.0, 4)  # 33, 36.5, 40, 43.5, 47 and -112, -109, -106, -103
TIME_L = pd.date_range("1990-12-01", periods=TL, freq="D")
TIME_Q = pd.date_range("2000-12-29", periods=TQ, freq="D")
CELL_OF = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [4, 4, 5, 5], [4, 4, 5, 5]], np.int32)  # bounds 32.5, 37.5, 42.5, 47.5 / -112.5, -107.5, -102.5


def arrays(f32=True):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(0)
    coarse = GridArray(280.0 + rng.standard_normal((TL, 3, 2)), ("time", "lat", "lon"), {"time": TIME_L, "lat": LAT_C, "lon": LON_C})
    fine = GridArray((280.0 + rng.standard_normal((TL, 5, 4))).astype(np.float32 if f32 else np.float64), ("time", "lat", "lon"),
                     {"time": TIME_L, "lat": LAT_F, "lon": LON_F})
    target = GridArray(280.0 + rng.standard_normal((TQ, 3, 2)), ("time", "lat", "lon"), {"time": TIME_Q, "lat": LAT_C, "lon": LON_C}, name="pr")
    return coarse, fine, target


def tables(status=None):
    idx = (np.arange(TQ * K, dtype=np.int32).reshape(TQ, K) * 7) % TL
    lidx = (np.arange(TQ * 6, dtype=np.int32).reshape(TQ, 6) * 11) % TL
    return [idx, np.ones((TQ, K)), np.zeros(TQ, np.int32) if status is None else np.asarray(status, np.int32), lidx, np.full((TQ, 6), 0.5)]


def predicted(f32=True, **kw):
    from skdownscale_amd import LocalizedAnalogs

    ctx = context(ScriptedLib())
    coarse, fine, target = arrays(f32)
    la = LocalizedAnalogs(n_analogs=K, ctx=ctx, **kw).fit(coarse, fine)
    ctx.lib.downloads = tables()
    return ctx, la, la.predict(target)


def test_exports():
    import skdownscale_amd
    from skdownscale_amd import _lib
    from skdownscale_amd.timesource import TAKEN_WHOLE

    assert {"LocalizedAnalogs", "LocalizedGridArray"} <= set(skdownscale_amd.__all__)
    assert {"sd_ca_local_dev", "sd_ca_local_apply_dev"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["sd_ca_local_dev"]) == 16 and len(_lib.SIGNATURES["sd_ca_local_apply_dev"]) == 20
    assert "localized" in TAKEN_WHOLE["any"] and "localized" not in TAKEN_WHOLE["resample"] and "constructed" in TAKEN_WHOLE["any"]
    assert _lib.CA_ADJUST == {"none": lo.ADJUST_NONE, "shift": lo.ADJUST_SHIFT, "scale": lo.ADJUST_SCALE}
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sd_downscale.h")).read()
    assert f"#define SD_CA_LOCAL_MAX_CELLS {_lib.CA_LOCAL_MAX_CELLS}\n" in header and "int sd_ca_local_apply_dev(sd_ctx* ctx" in header


def test_cell_of_for_ascending_and_descending_coordinates_bounds_and_the_hull():
    from skdownscale_amd.localized import coarse_index

    c = np.array([35.0, 40.0, 45.0])  # bounds 32.5, 37.5, 42.5, 47.5
    x = np.array([32.4, 32.5, 35.0, 37.5, 42.4999, 42.5, 47.5, 47.6, np.nan])
    want = [-1, 0, 0, 1, 1, 2, 2, -1, -1]  # the lower bound belongs to the cell, so does the outermost upper bound
    assert list(coarse_index(c, x)) == want and coarse_index(c, x).dtype == np.int32
    assert list(coarse_index(c[::-1], x)) == [-1 if m < 0 else 2 - m for m in want]  # descending coarse centres: the same cells, counted back
    assert list(coarse_index(c, x[::-1])) == want[::-1]
    assert list(coarse_index(np.array([0.0, 1.0, 3.0]), np.array([-0.5, 0.5, 1.9, 2.0, 4.0]))) == [0, 1, 1, 2, 2]  # uneven spacing
    with pytest.raises(ValueError, match="the coarse coordinate 'lat' has 1 centre"):
        coarse_index(np.array([1.0]), x, "lat")
    with pytest.raises(ValueError, match="the fine coordinate 'lat' must be one-dimensional and numeric"):
        coarse_index(c, np.array(["a", "b"]), "lat")
    ctx, la, pred = predicted()
    assert np.array_equal(la._cell_of, CELL_OF) and la._cell_of.dtype == np.int32 and np.array_equal(pred.cell_of, CELL_OF)


def test_cell_of_follows_the_fine_dims_and_marks_cells_outside_the_hull():
    from skdownscale_amd import GridArray, LocalizedAnalogs

    coarse, fine, _ = arrays()
    lat = np.array([47.0, 43.5, 40.0, 36.5, 20.0])  # descending, the last centre outside the hull
    flipped = GridArray(np.ascontiguousarray(fine.values.transpose(0, 2, 1)), ("time", "lon", "lat"), {"time": TIME_L, "lat": lat, "lon": LON_F})
    la = LocalizedAnalogs(n_analogs=K, ctx=context(ScriptedLib())).fit(coarse, flipped)
    want = np.array([[4, 4, 2, 0, -1], [4, 4, 2, 0, -1], [5, 5, 3, 1, -1], [5, 5, 3, 1, -1]])  # [lon, lat]: coarse column i_lat * 2 + j_lon
    assert np.array_equal(la._cell_of, want)


def test_predict_calls_select_and_local_and_stays_lazy():
    from skdownscale_amd import LocalizedGridArray

    ctx, la, pred = predicted(radius=(1, 2))
    assert [n for n, _ in ctx.lib.log] == ["sd_ca_select_dev", "sd_ca_local_dev"]  # no weights stage, nothing of the fine library
    sel, loc = ctx.lib.log[0][1], ctx.lib.log[1][1]
    assert sel[2:4] == [6, TL] and sel[5:8] == [6, TQ, 6] and sel[9] == K and sel[12:14] == [366, 45]
    # ctx, L, ld_l, Tl, Q, ld_q, Tq, ny, nx, wc, k, ry, rx, idx, local_idx, local_dist
    assert loc[2:4] == [6, TL] and loc[5:9] == [6, TQ, 3, 2] and loc[10:13] == [K, 1, 2]
    assert loc[1] == sel[1] and loc[4] == sel[4] and loc[13] == sel[16]  # one upload each; the table of select
    assert np.array_equal(ctx.lib.tables[0], np.repeat(np.cos(np.deg2rad(LAT_C)), 2))
    assert isinstance(pred, LocalizedGridArray) and not pred.computed and pred.shape == (TQ, 5, 4) and pred.name == "pr"
    assert pred.dims == ("time", "lat", "lon") and len(pred.coords["lat"]) == 5 and list(pred.coords["time"]) == list(TIME_Q)
    want = tables()
    assert np.array_equal(la.analog_index_, want[0]) and np.array_equal(la.analog_distance_, want[1]) and np.array_equal(la.status_, want[2])
    assert np.array_equal(la.local_index_, want[3].reshape(TQ, 3, 2)) and la.local_index_.dtype == np.int32
    assert np.array_equal(la.local_distance_, want[4].reshape(TQ, 3, 2)) and not hasattr(la, "weights_")
    assert sum(n == "sd_dev_alloc" for n, _ in ctx.lib.traffic) == sum(n == "sd_dev_free" for n, _ in ctx.lib.traffic) == 7  # all freed
    assert predicted(radius=3)[0].lib.log[1][1][11:13] == [3, 3]


def test_too_few_candidates_raise_and_a_non_finite_day_does_not():
    from skdownscale_amd import LocalizedAnalogs

    coarse, fine, target = arrays()
    ctx = context(ScriptedLib())
    la = LocalizedAnalogs(n_analogs=K, window=2, ctx=ctx).fit(coarse, fine)
    ctx.lib.downloads = tables([0, 0, co.FEW_CANDIDATES, 0, co.FEW_CANDIDATES, 0])
    with pytest.raises(ValueError, match=r"step 2 of the target \(2000-12-31 00:00:00\) has fewer than n_analogs=4 candidate days .*window=2"):
        la.predict(target)
    assert list(la.status_) == [0, 0, 2, 0, 2, 0] and la.local_index_.shape == (TQ, 3, 2)  # the tables of the failed predict stay readable
    ctx.lib.downloads = tables([0, co.QUERY_NONFINITE, 0, 0, 0, 0])
    assert not la.predict(target).computed  # a non-finite target day is a NaN row, not an error


def test_constructor_fit_and_predict_refusals():
    from skdownscale_amd import GridArray, LocalizedAnalogs

    for kw, words in ((dict(n_analogs=0), "n_analogs=0: expected 1 to 32"), (dict(n_analogs=33), "n_analogs=33"), (dict(window=-1), "window=-1"),
                      (dict(radius=-1), "radius=-1: expected a number of coarse cells >= 0 or a pair"), (dict(radius=1.5), "radius=1.5"),
                      (dict(radius=(1, 2, 3)), r"radius=\(1, 2, 3\)"), (dict(radius=(1, -2)), r"radius=\(1, -2\)"), (dict(radius="a"), "radius='a'"),
                      (dict(adjust="add"), "adjust='add': expected one of 'none', 'shift', 'scale'"), (dict(max_scale=0), "max_scale=0: expected None or a limit > 0"),
                      (dict(max_scale=-2.0), "max_scale=-2.0"), (dict(max_scale=float("nan")), "max_scale=nan"), (dict(weights="volume"), "weights='volume'")):
        with pytest.raises(ValueError, match=words):
            LocalizedAnalogs(**kw)
    assert LocalizedAnalogs(radius=0).radius == (0, 0) and LocalizedAnalogs(radius=(2, 1)).radius == (2, 1) and LocalizedAnalogs().max_scale is None
    coarse, fine, target = arrays()
    la = LocalizedAnalogs(n_analogs=K, ctx=context(ScriptedLib()))
    with pytest.raises(ValueError, match="this LocalizedAnalogs is not fitted"):
        la.predict(target)
    # what ConstructedAnalogs.fit checks
    with pytest.raises(ValueError, match="the fine library: expected a GridArray, got ndarray"):
        la.fit(coarse, fine.values)
    with pytest.raises(ValueError, match="the libraries differ: 400 coarse and 399 fine steps of 'time'"):
        la.fit(coarse, fine.isel(time=slice(0, 399)))
    with pytest.raises(ValueError, match="the time coordinate of the coarse library must be a DatetimeIndex"):
        la.fit(GridArray(coarse.values, coarse.dims, dict(coarse.coords, time=np.arange(TL))), fine)
    # the two grids
    with pytest.raises(ValueError, match=r"the coarse library needs exactly two spatial dims beside 'time', got \('cell',\)"):
        la.fit(GridArray(coarse.values.reshape(TL, 6), ("time", "cell"), {"time": TIME_L}), fine)
    with pytest.raises(ValueError, match=r"the fine library has spatial dims \('y', 'x'\); expected \('lat', 'lon'\) in any order"):
        la.fit(coarse, GridArray(fine.values, ("time", "y", "x"), {"time": TIME_L, "y": LAT_F, "x": LON_F}))
    with pytest.raises(ValueError, match="the fine library has no coordinate for dim 'lon'"):
        la.fit(coarse, GridArray(fine.values, fine.dims, {"time": TIME_L, "lat": LAT_F}))
    with pytest.raises(ValueError, match="the coarse library has no coordinate for dim 'lat'"):
        LocalizedAnalogs(weights="plain").fit(GridArray(coarse.values, coarse.dims, {"time": TIME_L, "lon": LON_C}), fine)
    with pytest.raises(ValueError, match="the coarse coordinate 'lat' is not strictly monotonic"):
        la.fit(GridArray(coarse.values, coarse.dims, dict(coarse.coords, lat=np.array([35.0, 45.0, 40.0]))), fine)
    with pytest.raises(ValueError, match="the fine coordinate 'lon' must be one-dimensional and numeric"):
        la.fit(coarse, GridArray(fine.values, fine.dims, dict(fine.coords, lon=np.array(["a", "b", "c", "d"]))))
    with pytest.raises(ValueError, match="not fitted"):  # a failed fit leaves nothing half fitted
        la.predict(target)
    la.fit(coarse, fine)
    with pytest.raises(ValueError, match=r"the target has dims \('time', 'y', 'x'\); expected \('time', 'lat', 'lon'\) in any order"):
        la.predict(GridArray(target.values, ("time", "y", "x"), target.coords))
    with pytest.raises(ValueError, match=r"the target has sizes \{'lat': 2, 'lon': 2\} on the coarse grid"):
        la.predict(target.isel(lat=slice(0, 2)))
    with pytest.raises(ValueError, match="the time coordinate of the target must be a DatetimeIndex"):
        la.predict(GridArray(target.values, target.dims, dict(target.coords, time=np.arange(TQ))))
    assert la._ctx.lib.log == [] and la._ctx.lib.traffic == []  # nothing reached the library


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("adjust,max_scale", [("none", None), ("shift", None), ("scale", 3.0)])
def test_values_apply_the_whole_field_once(f32, adjust, max_scale):
    ctx, la, pred = predicted(f32, adjust=adjust, max_scale=max_scale)
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    values = pred.values
    assert values.shape == (TQ, 5, 4) and pred.computed
    (name, a), = ctx.lib.log
    # ctx, F, f_is_f32, ld_f, Tl, Cf, cell_of, local_idx, Cc, L, ld_l, Q, ld_q, adjust, max_scale, Tq, q0, q1, out, ld_out
    assert name == "sd_ca_local_apply_dev" and a[2:6] == [int(f32), 20, TL, 20] and a[8] == 6 and a[15:18] == [TQ, 0, TQ] and a[19] == 20
    assert a[13:15] == [getattr(lo, "ADJUST_" + adjust.upper()), 0.0 if max_scale is None else max_scale]
    up = [args[3] for n, args in ctx.lib.traffic if n == "sd_memcpy_h2d"]
    fine_bytes = TL * 20 * (4 if f32 else 8)
    if adjust == "none":  # the coarse fields are neither uploaded nor handed over
        assert up == [fine_bytes, 20 * 4, TQ * 6 * 4] and a[9:13] == [None, 0, None, 0]
    else:
        assert up == [fine_bytes, 20 * 4, TQ * 6 * 4, TL * 6 * 8, TQ * 6 * 8] and a[9] is not None and a[11] is not None and a[10] == a[12] == 6
    assert sum(n == "sd_dev_alloc" for n, _ in ctx.lib.traffic) == sum(n == "sd_dev_free" for n, _ in ctx.lib.traffic)


def test_isel_stays_lazy_and_slices_the_library_the_cells_and_the_rows():
    from skdownscale_amd import LocalizedGridArray

    ctx, la, pred = predicted()
    win = pred.isel(lat=slice(1, 4), lon=slice(0, 2), time=slice(2, 5))
    assert isinstance(win, LocalizedGridArray) and not win.computed and not pred.computed and win.shape == (3, 3, 2)
    assert np.array_equal(win.local_index, la.local_index_.reshape(TQ, 6)[2:5]) and list(win.coords["time"]) == list(TIME_Q[2:5])
    assert np.array_equal(win.cell_of, CELL_OF[1:4, 0:2]) and np.array_equal(win.coords["lat"], LAT_F[1:4]) and win._Q.shape == (3, 6)
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    win.values
    (name, a), = ctx.lib.log
    assert name == "sd_ca_local_apply_dev" and a[3:6] == [6, TL, 6] and a[8] == 6 and a[15:18] == [3, 0, 3]
    up = [args[3] for n, args in ctx.lib.traffic if n == "sd_memcpy_h2d"]
    assert up == [TL * 6 * 4, 6 * 4, 3 * 6 * 4, TL * 6 * 8, 3 * 6 * 8]  # the cells and the rows of the window only; the coarse library whole
    with pytest.raises(ValueError, match="dim 'x' is not a dim"):
        pred.isel(x=slice(0, 1))
    picked = pred.isel(lat=[0, 2])  # anything but slices is answered on the computed field
    assert not isinstance(picked, LocalizedGridArray) and picked.shape == (TQ, 2, 4) and pred.computed


def test_block_producer_keeps_the_libraries_resident():
    from skdownscale_amd.timesource import takes_whole

    ctx, la, pred = predicted()
    assert takes_whole(pred, "any", "time") and not takes_whole(pred, "resample", "time") and not takes_whole(pred, "any", "lat")
    assert pred._block_producer(ctx, "lat") is None
    p = pred._block_producer(ctx, "time")
    assert (p.rows, p.cells, p.dtype, p.uploads) == (TQ, 20, np.float64, False)
    ctx.lib.log.clear(), ctx.lib.traffic.clear()
    out = ctx.lib.resident(ctx, "OUT", (TQ, 20))
    for r0, r1 in ((0, 2), (2, 4), (4, 6)):
        p.produce(r0, r1, out=out.rows(r0, r1))
    calls = [a for n, a in ctx.lib.log]
    assert [n for n, _ in ctx.lib.log] == ["sd_ca_local_apply_dev"] * 3 and [a[15:18] for a in calls] == [[TQ, 0, 2], [TQ, 2, 4], [TQ, 4, 6]]
    assert [a[18] for a in calls] == [("OUT", 0), ("OUT", 40), ("OUT", 80)]
    assert all(len({a[i] for a in calls}) == 1 for i in (1, 6, 7, 9, 11))  # the same five resident arrays in every call
    assert sum(n == "sd_memcpy_h2d" for n, _ in ctx.lib.traffic) == 5  # the fine library, cell_of, the table and the two coarse fields, once
    pred.values
    assert pred._block_producer(ctx, "time") is None  # computed: its rows are uploaded like any host array's


def test_engine_wrappers_refuse_before_the_library():
    ctx = context(ScriptedLib())
    L, Q, wc = coarse_case()
    idx = ctx.lib.resident(ctx, "IDX", (9, 3), np.int32)
    for call, words in ((lambda: ctx.ca_local(L, Q, wc, (3, 4), (1, 1), np.zeros((9, 3), np.int32)), "idx: expected the int32"),
                        (lambda: ctx.ca_local(L, Q[:, :5], wc, (3, 4), (1, 1), idx), r"Q: expected a \[Tq, 12\] field like L"),
                        (lambda: ctx.ca_local(L, Q, wc[:3], (3, 4), (1, 1), idx), "wc: expected 12 column weights"),
                        (lambda: ctx.ca_local(L, Q, wc, (3, 5), (1, 1), idx), r"grid: expected \(ny, nx\) with ny \* nx = 12 columns, got \(3, 5\)"),
                        (lambda: ctx.ca_local(L, Q, wc, 12, (1, 1), idx), r"grid=12, radius=\(1, 1\): expected \(ny, nx\) and \(ry, rx\)"),
                        (lambda: ctx.ca_local(L, Q, wc, (3, 4), (1, -1), idx), r"sd_ca_local: radii \(1, -1\), expected two numbers of coarse cells >= 0"),
                        (lambda: ctx.ca_local(L, Q[:4], wc, (3, 4), (1, 1), idx), r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)"),
                        (lambda: ctx.ca_local(L[:0], Q, wc, (3, 4), (1, 1), idx), r"sd_ca_local: bad sizes \(Tl=0, Tq=9, Cc=12\)"),
                        (lambda: ctx.ca_local(L, Q, wc, (3, 4), (1, 1), ctx.lib.resident(ctx, "I33", (9, 33), np.int32)), r"k = 33 lies outside \[1, 32\]")):
        with pytest.raises(ValueError, match=words):
            call()
    assert ctx.lib.log == [] and ctx.lib.traffic == []
    lidx, ldist = ctx.ca_local(L, Q, wc, (3, 4), (1, 2), idx)
    assert (lidx.shape, lidx.dtype, ldist.shape, ldist.dtype) == ((9, 12), np.int32, (9, 12), np.float64)
    F, cell_of = ctx.lib.resident(ctx, "F", (120, 7), np.float32), ctx.lib.resident(ctx, "CELL", (7,), np.int32)
    Ld, Qd = ctx.lib.resident(ctx, "L", (120, 12)), ctx.lib.resident(ctx, "Q", (9, 12))
    n = len(ctx.lib.log)
    for call, words in ((lambda: ctx.ca_local_apply(np.zeros((4, 4)), cell_of, lidx), "F: expected a float32 or float64"),
                        (lambda: ctx.ca_local_apply(F, np.zeros(7, np.int32), lidx), r"cell_of: expected an int32 DeviceArray of shape \(7,\)"),
                        (lambda: ctx.ca_local_apply(F, ctx.lib.resident(ctx, "C8", (8,), np.int32), lidx), "cell_of: expected"),
                        (lambda: ctx.ca_local_apply(F, cell_of, None), "local_idx: expected the int32"),
                        (lambda: ctx.ca_local_apply(F, cell_of, ldist), r"local_idx: expected a contiguous int32 DeviceArray of shape \(9, 12\)"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, adjust="add"), "adjust='add': expected one of 'none', 'shift', 'scale'"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, max_scale=-1.0), "sd_ca_local_apply: max_scale = -1, expected 0"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, max_scale=float("nan")), "max_scale = nan"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, adjust="shift"), r"L: adjust='shift' needs a float64 DeviceArray of shape \(120, 12\)"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, Ld, Qd.rows(0, 4), adjust="scale"), r"Q: adjust='scale' needs a float64 DeviceArray of shape \(9, 12\)"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, q0=3, q1=3), r"sd_ca_local_apply: rows \[3, 3\) lie outside the 9 targets"),
                        (lambda: ctx.ca_local_apply(F, cell_of, lidx, q0=0, q1=2, out=ctx.lib.resident(ctx, "O", (3, 7))),
                         r"out: expected a float64 DeviceArray of shape \(2, 7\)")):
        with pytest.raises(ValueError, match=words):
            call()
    other = context(ScriptedLib())
    with pytest.raises(ValueError, match="sd_ca_local_apply: `cell_of` belongs to another context"):
        ctx.ca_local_apply(F, other.lib.resident(other, "C2", (7,), np.int32), lidx)
    assert len(ctx.lib.log) == n
    ctx.ca_local_apply(F, cell_of, lidx, Ld, Qd, adjust="scale", max_scale=4.0, q0=2, q1=5)
    a = ctx.lib.log[-1][1]
    assert ctx.lib.log[-1][0] == "sd_ca_local_apply_dev" and a[1:9] == [("F", 0), 1, 7, 120, 7, ("CELL", 0), a[7], 12]
    assert a[9:18] == [("L", 0), 12, ("Q", 0), 12, lo.ADJUST_SCALE, 4.0, 9, 2, 5] and a[19] == 7
