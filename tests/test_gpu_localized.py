"""GPU: the localized-analog kernels (csrc/sd_localized.hip) against the rule restated in tests/_localized_oracle.py, bit for bit: the
chosen days and their local distances at every radius and grid shape where ca_local_kernel takes another path (tile constants from
csrc/sd_localized_plan.h), with ties, non-finite targets and padded rows, the synthesised field under every adjustment, and through
``LocalizedAnalogs`` / ``LocalizedGridArray``."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import _localized_oracle as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "scikit-downscale_amd", "csrc", "sd_localized_plan.h")).read()


def plan_const(name):
    value = re.search(rf"constexpr int {name} = (\w+);", PLAN).group(1)  # a number, or the name of another constant
    return int(value) if value.isdigit() else plan_const(value)


LOC_BLOCK, LAP_ROWS, LAP_BATCH = (plan_const(n) for n in ("kLocBlock", "kLapRows", "kLapBatch"))
LAP_CELLS = 64 * plan_const("kLapWaves")  # kLapCells = kLapBlock = kLanes * kLapWaves


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def make_case(seed=0, Tl=120, Tq=9, ny=3, nx=4):
    """fields near 280 K; column 5 of the library holds a NaN, column 8 weighs 0 (where the grid has them)"""
    rng = np.random.default_rng(seed)
    Cc = ny * nx
    L = 280.0 + 8.0 * rng.standard_normal((Tl, Cc))
    Q = 280.0 + 8.0 * rng.standard_normal((Tq, Cc))
    wc = np.cos(np.deg2rad(np.linspace(30.0, 60.0, Cc)))
    if Cc > 8:
        L[Tl // 3, 5] = np.nan
        wc[8] = 0.0
    return dict(L=L, Q=Q, wc=wc, ny=ny, nx=nx)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def nan_equal_bits(a, b):
    """bit equality, any NaN equal to any NaN (the payload of a propagated NaN is not part of the rule)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0.0, a), np.where(nan, 0.0, b))


def padded(ctx, a, pad, fill=1e30):
    """``a`` [T, C] on the device with rows ``C + pad`` apart and ``fill`` between them"""
    if not pad:
        return ctx.to_device(a, a.dtype)
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    wide[:, :a.shape[1]] = a
    return ctx.to_device(wide, a.dtype).cells(0, a.shape[1])


def choose(ctx, case, k, radius, pad_l=0, pad_q=0):
    """sd_ca_select_dev and sd_ca_local_dev -> idx, dist, local_idx, local_dist as host arrays"""
    Ld, Qd = padded(ctx, case["L"], pad_l), padded(ctx, case["Q"], pad_q)
    idx, dist, status = ctx.ca_select(Ld, Qd, case["wc"], k)
    lidx, ldist = ctx.ca_local(Ld, Qd, case["wc"], (case["ny"], case["nx"]), radius, idx)
    return idx.to_host(), dist.to_host(), lidx.to_host(), ldist.to_host()


def check_choice(case, got, radius):
    """the GPU's choice against the oracle's on the GPU's own regional table -> the oracle's slots"""
    idx, _, lidx, ldist = got
    slot, elidx, eldist = lo.local(case["L"], case["Q"], case["wc"], idx, case["ny"], case["nx"], *radius)
    assert lidx.dtype == np.int32 and np.array_equal(lidx, elidx)
    assert nan_equal_bits(ldist, eldist), np.nanmax(np.abs(ldist - eldist))
    return slot


# ---- the choice -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("radius", [(0, 0), (1, 1), (1, 2), (5, 5)])
def test_base_grid_equals_the_oracle_bit_for_bit(ctx, k, radius):
    case = make_case()
    got = choose(ctx, case, k, radius)
    slot = check_choice(case, got, radius)
    assert (got[2] >= 0).all()
    if k == 1:
        assert (slot == 0).all()
    if k == 5 and radius == (1, 1):  # a kernel that always answers slot 0 cannot pass
        assert all(len(set(row)) >= 3 for row in slot)
    if radius == (0, 0):  # an unused cell alone: +0.0 for every slot, hence slot 0
        assert (slot[:, [5, 8]] == 0).all() and same_bits(got[3][:, [5, 8]], np.zeros((9, 2)))


@pytest.mark.parametrize("k", [5, 32])
def test_radii_that_cover_the_grid_give_the_regional_distance(ctx, k):
    """the local sum is then the regional sum in the same order: slot 0 everywhere, and local_dist == dist[:, 0] bit for bit"""
    case = make_case(seed=1)
    idx, dist, lidx, ldist = choose(ctx, case, k, (2, 3))
    assert (lidx == idx[:, :1]).all()
    assert same_bits(ldist, np.repeat(dist[:, :1], 12, axis=1))
    far = choose(ctx, case, k, (1 << 40, 1 << 40))  # radii past the grid
    assert same_bits(far[2], lidx) and same_bits(far[3], ldist)


@pytest.mark.parametrize("ny,nx", [(9, 17), (1, 7), (7, 1), (LOC_BLOCK // 16, 16 + 1)])
def test_grids_beside_a_workgroups_share(ctx, ny, nx):
    """9 x 17, one row and one column of cells, and one column more than the cells that one pass of a workgroup's threads covers"""
    case = make_case(seed=2, Tl=60, Tq=3, ny=ny, nx=nx)
    for radius in ((1, 1), (2, 0)):
        check_choice(case, choose(ctx, case, 4, radius), radius)
    assert (ny, nx) != (LOC_BLOCK // 16, 17) or LOC_BLOCK < ny * nx < 2 * LOC_BLOCK  # a second, partly filled pass over the cells


def test_ties_go_to_the_lower_slot(ctx):
    case = make_case(seed=3)
    for t in (17, 41, 119):
        case["L"][t] = case["L"][5]  # three more copies of day 5: four identical rows
    case["Q"][2] = case["L"][5]      # a target equal to them
    got = choose(ctx, case, 5, (1, 1))
    slot = check_choice(case, got, (1, 1))
    assert list(got[0][2, :4]) == [5, 17, 41, 119]
    assert (slot[2] == 0).all() and (got[2][2] == 5).all() and same_bits(got[3][2], np.zeros(12))


def test_a_non_finite_target_row_has_no_choice(ctx):
    case = make_case(seed=4, Tq=6)
    clean = choose(ctx, case, 5, (1, 1))
    case["Q"][1, 2] = np.nan
    case["Q"][3, 11] = np.inf
    case["Q"][4, 5] = np.nan  # column 5 is not used: no effect
    got = choose(ctx, case, 5, (1, 1))
    check_choice(case, got, (1, 1))
    assert (got[2][[1, 3]] == -1).all() and np.isnan(got[3][[1, 3]]).all()
    for g, c in zip(got, clean):
        assert same_bits(g[[0, 2, 4, 5]], c[[0, 2, 4, 5]])


def test_padded_leading_dimensions_of_the_coarse_fields(ctx):
    case = make_case(seed=5, ny=9, nx=17)
    plain = choose(ctx, case, 6, (1, 2))
    wide = choose(ctx, case, 6, (1, 2), pad_l=3, pad_q=5)
    check_choice(case, plain, (1, 2))
    for p, w in zip(plain, wide):
        assert nan_equal_bits(p, w) if p.dtype == np.float64 else np.array_equal(p, w)


# ---- the synthesis --------------------------------------------------------------------------------------------------------------------
def apply_case(seed, Tl, Tq, Cc, Cf, f32):
    """a table of chosen days (row 1 without analogs), cell_of with a -1 and a value >= Cc, positive coarse fields with column 2 of the
    library <= 0 in places"""
    rng = np.random.default_rng(seed)
    L = 3.0 + rng.random((Tl, Cc))
    Q = 1.0 + 9.0 * rng.random((Tq, Cc))
    L[::2, 2 % Cc] = 0.0
    L[1::4, 2 % Cc] = -1.5
    F = 280.0 + 10.0 * rng.standard_normal((Tl, Cf))
    F = F.astype(np.float32) if f32 else F
    lidx = rng.integers(0, Tl, (Tq, Cc)).astype(np.int32)
    if Tq > 1:
        lidx[1] = -1
    cell_of = rng.integers(0, Cc, Cf).astype(np.int32)
    if Cf > 2:
        cell_of[Cf // 2], cell_of[Cf - 1] = -1, Cc
    return dict(L=L, Q=Q, F=F, lidx=lidx, cell_of=cell_of)


def synthesise(ctx, case, adjust, max_scale=0.0, rows=None, pad_f=0, pad_out=0, pad_c=0):
    F, lidx = case["F"], case["lidx"]
    Tq, Cf = lidx.shape[0], F.shape[1]
    q0, q1 = (0, Tq) if rows is None else rows
    Fd = padded(ctx, F, pad_f)
    outd = ctx.to_device(np.full((q1 - q0, Cf + pad_out), -7.0))
    view = outd.cells(0, Cf) if pad_out else outd
    coarse = {} if adjust == "none" else dict(L=padded(ctx, case["L"], pad_c, np.nan), Q=padded(ctx, case["Q"], pad_c, np.nan))
    ctx.ca_local_apply(Fd, ctx.to_device(case["cell_of"], np.int32), ctx.to_device(lidx, np.int32), adjust=adjust, max_scale=max_scale, q0=q0,
                       q1=q1, out=view, **coarse)
    if pad_out:
        assert (outd.to_host()[:, Cf:] == -7.0).all()  # nothing is written between the rows
    return view.to_host()


def expected(case, adjust, max_scale=0.0, q0=0, q1=None):
    return lo.local_apply(case["F"], case["cell_of"], case["lidx"], case["L"], case["Q"], getattr(lo, "ADJUST_" + adjust.upper()), max_scale, q0, q1)


@pytest.mark.parametrize("Cf", [1, 130, LAP_CELLS + 1])
@pytest.mark.parametrize("f32", [False, True])
def test_every_adjustment_equals_the_oracle_bit_for_bit(ctx, Cf, f32):
    case = apply_case(10 + Cf, Tl=40, Tq=LAP_ROWS + LAP_BATCH + 1, Cc=12, Cf=Cf, f32=f32)  # more rows than one row group, a cut batch
    for adjust, max_scale in (("none", 0.0), ("shift", 0.0), ("scale", 0.0), ("scale", 2.0), ("scale", 50.0)):
        got, exp = synthesise(ctx, case, adjust, max_scale), expected(case, adjust, max_scale)
        assert nan_equal_bits(got, exp), (adjust, max_scale, np.nanmax(np.abs(got - exp)))
        assert np.isnan(got[1]).all() and np.isfinite(got[0, 0])
    if Cf > 2:
        assert np.isnan(got[:, [Cf // 2, Cf - 1]]).all()
    rows = case["lidx"][:, case["cell_of"][0]]
    assert same_bits(synthesise(ctx, case, "none")[[0, 2], 0], case["F"][rows[[0, 2]], 0].astype(np.float64))  # a plain copy


def test_scale_limits_and_library_cells_that_are_not_positive(ctx):
    case = apply_case(20, Tl=40, Tq=9, Cc=12, Cf=130, f32=True)
    L, Q, lidx, cell_of = case["L"], case["Q"], case["lidx"], case["cell_of"]
    free, cut, loose = (synthesise(ctx, case, "scale", m) for m in (0.0, 2.0, 50.0))
    valid = ((cell_of >= 0) & (cell_of < 12))[None, :] & (lidx[:, np.clip(cell_of, 0, 11)] >= 0)  # [Tq, Cf]: a day and a coarse cell
    c = np.broadcast_to(np.clip(cell_of, 0, 11), valid.shape)
    t = np.maximum(lidx[:, np.clip(cell_of, 0, 11)], 0)
    Fv, Lv, Qv = case["F"][t, np.arange(130)[None, :]].astype(np.float64), L[t, c], Q[np.arange(9)[:, None], c]
    keep = valid & (Lv <= 0.0)
    assert keep.sum() > 20 and same_bits(free[keep], Fv[keep])  # r = 1 where the library is not > 0
    with np.errstate(all="ignore"):
        ratio = Qv / Lv
    hit, below = valid & (Lv > 0.0) & (ratio > 2.0), valid & (Lv > 0.0) & (ratio <= 2.0)
    assert hit.sum() > 20 and below.sum() > 20  # max_scale = 2 is hit and not hit
    assert same_bits(cut[hit], Fv[hit] * 2.0) and not same_bits(cut[hit], free[hit]) and same_bits(cut[below], free[below])
    assert (ratio[hit] < 50.0).all() and nan_equal_bits(loose, free)


def test_row_cuts_and_leading_dimensions_with_sentinels(ctx):
    case = apply_case(30, Tl=50, Tq=2 * LAP_ROWS + 5, Cc=12, Cf=130, f32=True)
    whole = synthesise(ctx, case, "shift")
    assert nan_equal_bits(whole, expected(case, "shift"))
    for rows in ((0, 1), (3, LAP_ROWS + 4), (LAP_ROWS, 2 * LAP_ROWS + 5)):
        assert nan_equal_bits(synthesise(ctx, case, "shift", rows=rows), whole[rows[0]:rows[1]])
    # what lies between the rows of F (1e30) and of L / Q (NaN) must not be read, what lies between the rows of out not written
    assert nan_equal_bits(synthesise(ctx, case, "shift", pad_f=3, pad_out=5, pad_c=2), whole)


def test_engine_refusals(ctx):
    case = make_case(Tl=20, Tq=3)
    L, Q, wc = case["L"], case["Q"], case["wc"]
    idx, dist, status = ctx.ca_select(L, Q, wc, 3)
    with pytest.raises(ValueError, match=r"grid: expected \(ny, nx\) with ny \* nx = 12"):
        ctx.ca_local(L, Q, wc, (3, 5), (1, 1), idx)
    with pytest.raises(ValueError, match=r"radii \(-1, 0\)"):
        ctx.ca_local(L, Q, wc, (3, 4), (-1, 0), idx)
    with pytest.raises(ValueError, match=r"wc\[1\] = -1"):
        ctx.ca_local(L, Q, np.where(np.arange(12) == 1, -1.0, wc), (3, 4), (1, 1), idx)
    with pytest.raises(ValueError, match="no column is used"):
        ctx.ca_local(L, Q, np.zeros(12), (3, 4), (1, 1), idx)
    lidx, _ = ctx.ca_local(L, Q, wc, (3, 4), (1, 1), idx)
    F, cell_of = ctx.to_device(np.zeros((20, 4), np.float32), np.float32), ctx.to_device(np.zeros(4, np.int32), np.int32)
    with pytest.raises(ValueError, match=r"rows \[2, 9\)"):
        ctx.ca_local_apply(F, cell_of, lidx, q0=2, q1=9)
    with pytest.raises(ValueError, match="adjust='shift' needs a float64 DeviceArray"):
        ctx.ca_local_apply(F, cell_of, lidx, adjust="shift")


# ---- through Python -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids(ctx):
    from skdownscale_amd import GridArray, LocalizedAnalogs

    rng = np.random.default_rng(11)
    time_l = pd.date_range("1990-01-01", periods=3 * 365 + 1, freq="D")
    time_q = pd.date_range("2001-01-01", periods=90, freq="D")
    lat_c, lon_c = np.array([35.0, 40.0, 45.0]), np.array([-110.0, -105.0, -100.0, -95.0])
    lat_f, lon_f = np.linspace(33.0, 47.0, 10), np.linspace(-112.0, -93.0, 13)
    season = 8.0 * np.cos(2 * np.pi * (time_l.dayofyear.to_numpy() - 200) / 365.25)
    coarse = (280.0 + season[:, None, None] + 3.0 * rng.standard_normal((len(time_l), 3, 4)))
    coarse[:, 1, 2] = np.nan  # a masked coarse cell
    fine = (280.0 + season[:, None, None] + 4.0 * rng.standard_normal((len(time_l), 10, 13))).astype(np.float32)
    fine[:, 0, 0] = np.nan    # a masked fine cell
    target = 281.0 + 8.0 * np.cos(2 * np.pi * (time_q.dayofyear.to_numpy() - 200) / 365.25)[:, None, None] + 3.0 * rng.standard_normal((90, 3, 4))
    target[:, 1, 2] = np.nan
    obs = 280.0 + 4.0 * rng.standard_normal((90, 10, 13))
    c = GridArray(coarse, ("time", "lat", "lon"), {"time": time_l, "lat": lat_c, "lon": lon_c})
    f = GridArray(fine, ("time", "lat", "lon"), {"time": time_l, "lat": lat_f, "lon": lon_f})
    t = GridArray(target, ("time", "lat", "lon"), {"time": time_q, "lat": lat_c, "lon": lon_c})
    o = GridArray(obs, ("time", "lat", "lon"), {"time": time_q, "lat": lat_f, "lon": lon_f})
    la = LocalizedAnalogs(n_analogs=8, window=20, radius=1, adjust="shift", ctx=ctx).fit(c, f)
    pred = la.predict(t)
    wc = np.repeat(np.cos(np.deg2rad(lat_c)), 4)
    L, Q = coarse.reshape(len(time_l), 12), target.reshape(90, 12)
    idx, dist, status = lo.select(L, Q, wc, 8, time_l.dayofyear.to_numpy(), time_q.dayofyear.to_numpy(), 366, 20, np.full(len(time_l), -1),
                                  np.full(90, -1))
    _, lidx, ldist = lo.local(L, Q, wc, idx, 3, 4, 1, 1)
    i = np.searchsorted([37.5, 42.5], lat_f, side="right")  # bounds 32.5, 37.5, 42.5, 47.5 and -112.5 .. -92.5: every centre inside
    j = np.searchsorted([-107.5, -102.5, -97.5], lon_f, side="right")
    cell_of = (i[:, None] * 4 + j[None, :]).astype(np.int32)
    out = lo.local_apply(fine.reshape(len(time_l), 130), cell_of.reshape(-1), lidx, L, Q, lo.ADJUST_SHIFT)
    return dict(la=la, pred=pred, exp=(idx, dist, status, lidx, ldist, out), cell_of=cell_of, obs=o, target=t)


def test_predict_values(grids):
    from skdownscale_amd import LocalizedGridArray

    la, pred, exp = grids["la"], grids["pred"], grids["exp"]
    assert isinstance(pred, LocalizedGridArray) and not pred.computed and pred.dims == ("time", "lat", "lon") and pred.shape == (90, 10, 13)
    assert np.array_equal(la.analog_index_, exp[0]) and nan_equal_bits(la.analog_distance_, exp[1]) and np.array_equal(la.status_, exp[2])
    assert np.array_equal(la.local_index_, exp[3].reshape(90, 3, 4)) and nan_equal_bits(la.local_distance_, exp[4].reshape(90, 3, 4))
    assert np.array_equal(pred.cell_of, grids["cell_of"])
    assert len(np.unique(la.local_index_[0])) > 1  # more than one library day in one field
    values = pred.values
    assert nan_equal_bits(values, exp[5].reshape(90, 10, 13))
    masked = grids["cell_of"] == 1 * 4 + 2  # the fine cells of the masked coarse cell: NaN under 'shift'
    assert np.isnan(values[:, 0, 0]).all() and np.isnan(values[:, masked]).all() and np.isfinite(values[:, ~masked][:, 1:]).all()


def test_device_field_and_compare_from_hbm(grids):
    from skdownscale_amd.timesource import takes_whole

    la, obs = grids["la"], grids["obs"]
    fresh = la.predict(grids["target"])
    field = fresh.device_field()
    assert tuple(field.shape) == (90, 130) and nan_equal_bits(field.to_host(), grids["exp"][5]) and not fresh.computed
    field.free()
    assert takes_whole(fresh, "any", "time")
    got = fresh.compare(obs).rmse().values
    assert not fresh.computed
    assert nan_equal_bits(got, fresh.compute().compare(obs).rmse().values)
    d = grids["exp"][5].reshape(90, 10, 13) - obs.values
    ok = np.isfinite(d).all(axis=0)
    assert ok.sum() > 100 and np.allclose(got[ok], np.sqrt((d * d).mean(axis=0))[ok], rtol=1e-12)


def test_resample_through_the_block_producer(grids):
    fresh = grids["la"].predict(grids["target"])
    whole = fresh.resample(time="MS").mean().values
    assert not fresh.computed
    blocked = fresh.resample(time="MS", scratch_bytes=31 * 130 * 8).mean().values  # 31 rows per block: January, February, March
    assert whole.shape == (3, 10, 13) and nan_equal_bits(blocked, whole)
    v = grids["exp"][5].reshape(90, 10, 13)
    field = grids["la"].predict(grids["target"]).compute().resample(time="MS").mean().values  # the same on the computed field
    assert nan_equal_bits(whole, field)
    ok = np.isfinite(v).all(axis=0)
    assert np.allclose(whole[:, ok], np.stack([v[:31].mean(0), v[31:59].mean(0), v[59:].mean(0)])[:, ok], rtol=1e-12)


def test_isel_of_a_cell_window_stays_lazy(grids):
    from skdownscale_amd import LocalizedGridArray

    fresh = grids["la"].predict(grids["target"])
    win = fresh.isel(lat=slice(2, 7), lon=slice(4, 13), time=slice(10, 50))
    assert isinstance(win, LocalizedGridArray) and not win.computed and not fresh.computed and win.shape == (40, 5, 9)
    assert nan_equal_bits(win.values, grids["exp"][5].reshape(90, 10, 13)[10:50, 2:7, 4:13])
