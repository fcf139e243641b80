"""GPU: the constructed-analog kernels (csrc/sd_constructed.hip) against the rule restated in tests/_constructed_oracle.py, bit for bit:
indices, distances, weights, status and the synthesised field, at every shape where the kernels take another path (tile edges from
csrc/sd_constructed_plan.h), with ties, too few candidates, non-finite targets and singular Gram matrices, and through
``ConstructedAnalogs`` / ``ConstructedGridArray``."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import _constructed_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "scikit-downscale_amd", "csrc", "sd_constructed_plan.h")).read()


def plan_const(name):
    value = re.search(rf"constexpr int {name} = (\w+);", PLAN).group(1)  # a number, or the name of another constant
    return int(value) if value.isdigit() else plan_const(value)


SEL_Q, SEL_L, SEL_COLS, APP_CELLS, APP_ROWS = (plan_const(n) for n in ("kSelQ", "kSelL", "kSelCols", "kAppCells", "kAppRows"))


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def make_case(seed=0, Tl=120, Tq=9, Cc=12, Cf=130, f32=False):
    """fields near 280 K; column 5 of the library holds a NaN, column 8 weighs 0"""
    rng = np.random.default_rng(seed)
    L = 280.0 + 8.0 * rng.standard_normal((Tl, Cc))
    Q = 280.0 + 8.0 * rng.standard_normal((Tq, Cc))
    wc = np.cos(np.deg2rad(np.linspace(30.0, 60.0, Cc)))
    if Cc > 8:
        L[Tl // 3, 5] = np.nan
        wc[8] = 0.0
    F = 280.0 + 10.0 * rng.standard_normal((Tl, Cf))
    F = F.astype(np.float32) if f32 else F
    return dict(L=L, Q=Q, wc=wc, F=F, key_l=np.zeros(Tl, np.int32), key_q=np.zeros(Tq, np.int32), period=366, window=-1,
                excl_l=np.full(Tl, -1, np.int32), excl_q=np.full(Tq, -1, np.int32))


def gpu(ctx, case, k, kind="regression", ridge=1e-6, ld_f=None, ld_out=None, rows=None):
    """the three calls -> idx, dist, weights, status, out as host arrays"""
    L, Q, F = case["L"], case["Q"], case["F"]
    idx, dist, status = ctx.ca_select(L, Q, case["wc"], k, case["key_l"], case["key_q"], case["period"], case["window"], case["excl_l"],
                                      case["excl_q"])
    w = ctx.ca_weights(L, Q, case["wc"], idx, dist, status, kind=kind, ridge=ridge)
    Tl, Cf = F.shape
    Fd = ctx.empty((Tl, Cf if ld_f is None else ld_f), F.dtype)
    if ld_f is not None:
        wide = np.full((Tl, ld_f), 1e30, F.dtype)  # (what lies between the rows must not be read)
        wide[:, :Cf] = F
        Fd.copy_from_host(wide)
        Fd = Fd.cells(0, Cf)
    else:
        Fd.copy_from_host(F)
    q0, q1 = (0, Q.shape[0]) if rows is None else rows
    outd = ctx.empty((q1 - q0, Cf if ld_out is None else ld_out))
    outd.copy_from_host(np.full(outd.shape, -7.0))
    view = outd if ld_out is None else outd.cells(0, Cf)
    ctx.ca_apply(Fd, idx, w, q0, q1, out=view)
    got = idx.to_host(), dist.to_host(), w.to_host(), status.to_host(), view.to_host()
    if ld_out is not None:
        assert (outd.to_host()[:, Cf:] == -7.0).all()  # nothing is written between the rows
    return got


def oracle(case, k, kind="regression", ridge=1e-6):
    return co.constructed(case["L"], case["Q"], case["wc"], case["F"], k, co.REGRESSION if kind == "regression" else co.MEAN, ridge,
                          case["key_l"], case["key_q"], case["period"], case["window"], case["excl_l"], case["excl_q"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def nan_equal_bits(a, b):
    """bit equality, any NaN equal to any NaN (the payload of a propagated NaN is not part of the rule)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0.0, a), np.where(nan, 0.0, b))


def check(got, exp):
    for name, g, e in zip(("idx", "dist", "weights", "status", "out"), got, exp):
        if name in ("idx", "status"):
            assert np.array_equal(g, e) and g.dtype == np.int32, name
        else:
            assert nan_equal_bits(g, e), (name, np.nanmax(np.abs(g - e)))


# ---- base shape ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_oracles():
    return {}


@pytest.mark.parametrize("k", [1, 5, 30, 32])
@pytest.mark.parametrize("kind", ["regression", "mean"])
@pytest.mark.parametrize("f32", [False, True])
def test_base_shape_equals_the_oracle_bit_for_bit(ctx, base_oracles, k, kind, f32):
    case = make_case(f32=f32)
    got = gpu(ctx, case, k, kind)
    key = (k, kind)
    if key not in base_oracles:  # the coarse side does not depend on the fine library's dtype
        base_oracles[key] = oracle(case, k, kind)[:4]
    exp = base_oracles[key]
    check(got, exp + (co.apply(case["F"], exp[0], exp[2]),))
    assert (got[3] == co.OK).all() and (got[0] >= 0).all()
    assert len(co.used_columns(case["L"], case["wc"])) == 10


def test_more_columns_than_one_staged_step(ctx):
    case = make_case(seed=3, Tl=70, Tq=5, Cc=2 * SEL_COLS + 3, Cf=7)
    check(gpu(ctx, case, 4), oracle(case, 4))
    wide = make_case(seed=4, Tl=40, Tq=3, Cc=2 * 64 + 1, Cf=3)  # more than one staged step of the weights kernel
    check(gpu(ctx, wide, 6), oracle(wide, 6))


# ---- ties and tiling ------------------------------------------------------------------------------------------------------------------
def tied_case(Tl=120, Tq=9):
    case = make_case(seed=1, Tl=Tl, Tq=Tq)
    for t in (17, 41, Tl - 1):
        case["L"][t] = case["L"][5]  # three more copies of day 5: four identical rows
    case["Q"][2] = case["L"][5]      # a target equal to them
    return case


def test_ties_go_to_the_earlier_day(ctx):
    case = tied_case()
    got = gpu(ctx, case, 5)
    check(got, oracle(case, 5))
    assert list(got[0][2, :4]) == [5, 17, 41, 119] and (got[1][2, :4] == 0.0).all()
    assert (got[3] == co.OK).all()  # the ridge keeps the duplicate rows solvable


@pytest.mark.parametrize("Tl,Tq", [(SEL_L + 1, 9), (120, SEL_Q + 1), (2 * SEL_L + 1, 2 * SEL_Q + 1)])
def test_results_do_not_depend_on_the_tiling(ctx, Tl, Tq):
    case = tied_case(Tl, Tq)
    got = gpu(ctx, case, 30)
    check(got, oracle(case, 30))
    # the same targets in a call of their own, and the same library days with the tile edge elsewhere
    few = dict(case, Q=case["Q"][3:8], key_q=case["key_q"][3:8], excl_q=case["excl_q"][3:8])
    alone = gpu(ctx, few, 30)
    for g, a in zip(got, alone):
        assert nan_equal_bits(g[3:8], a)


def test_ridge_zero_with_duplicate_analogs_is_singular(ctx):
    # integers: G[0][0] = 25 has an exact root, so the second pivot is exactly 25 - 5 * 5 = 0 in the rule's order
    case = make_case(seed=2, Tl=30, Tq=3, Cc=4, Cf=9)
    case["L"] = np.round(case["L"] - 270.0)
    case["wc"] = np.ones(4)
    case["L"][[3, 11, 20]] = [3.0, 4.0, 0.0, 0.0]
    case["Q"] = np.round(case["Q"] - 270.0)
    case["Q"][1] = [3.0, 4.0, 0.0, 0.0]
    got = gpu(ctx, case, 3, ridge=0.0)
    exp = oracle(case, 3, ridge=0.0)
    check(got, exp)
    assert got[3][1] == co.SINGULAR and (got[0][1] == -1).all() and np.isnan(got[1][1]).all() and np.isnan(got[2][1]).all()
    assert np.isnan(got[4][1]).all() and got[3][0] == co.OK and got[3][2] == co.OK and np.isfinite(got[4][[0, 2]]).all()


# ---- candidates -----------------------------------------------------------------------------------------------------------------------
def test_window_wraps_and_too_few_candidates(ctx):
    k = 6
    case = make_case(seed=5, Tl=60, Tq=4, Cf=11)
    key_l = np.full(60, 100, np.int32)
    key_l[[4, 9, 50]] = 364
    key_l[[7, 30, 59]] = 2       # with window 3 the target of day 1 has these six: exactly k
    key_l[10:15] = 200           # k - 1 days near day 200
    case.update(key_l=key_l, key_q=np.array([1, 100, 200, 365], np.int32), window=3)
    got = gpu(ctx, case, k)
    check(got, oracle(case, k))
    assert sorted(got[0][0]) == [4, 7, 9, 30, 50, 59]
    assert list(got[3]) == [co.OK, co.OK, co.FEW_CANDIDATES, co.OK]  # |365 - 2| = 363, 366 - 363 = 3: day 365 reaches 364 and 2 as well
    assert sorted(got[0][3]) == [4, 7, 9, 30, 50, 59]
    assert np.isnan(got[4][2]).all() and (got[0][2] == -1).all() and np.isfinite(got[4][[0, 1, 3]]).all()
    narrow = dict(case, window=2)  # day 1 loses the days of 364, day 365 those of 2: three candidates each
    got = gpu(ctx, narrow, k)
    check(got, oracle(narrow, k))
    assert list(got[3]) == [co.FEW_CANDIDATES, co.OK, co.FEW_CANDIDATES, co.FEW_CANDIDATES]


def test_same_year_exclusion_and_no_window(ctx):
    case = make_case(seed=6, Tl=90, Tq=5, Cf=5)
    case["excl_l"] = (1990 + np.arange(90) // 30).astype(np.int32)
    case["excl_q"] = np.array([1990, 1991, 1992, -1, 2000], np.int32)
    case["Q"][0] = case["L"][3]  # its own day is the nearest, but it lies in the excluded year
    got = gpu(ctx, case, 8)
    check(got, oracle(case, 8))
    assert (got[0][0] >= 30).all() and ((got[0][1] < 30) | (got[0][1] >= 60)).all() and (got[0][2] < 60).all()
    free = dict(case, excl_q=np.full(5, -1, np.int32))
    assert gpu(ctx, free, 8)[0][0, 0] == 3


# ---- status ---------------------------------------------------------------------------------------------------------------------------
def test_non_finite_targets(ctx):
    case = make_case(seed=7, Tl=50, Tq=6, Cf=8)
    clean = gpu(ctx, case, 5)
    case["Q"][1, 2] = np.nan
    case["Q"][3, 11] = np.inf
    case["Q"][4, 5] = np.nan   # column 5 is not used (NaN in the library): no effect
    case["Q"][5, 8] = -np.inf  # column 8 is not used (weight 0): no effect
    got = gpu(ctx, case, 5)
    check(got, oracle(case, 5))
    assert list(got[3]) == [co.OK, co.QUERY_NONFINITE, co.OK, co.QUERY_NONFINITE, co.OK, co.OK]
    assert np.isnan(got[4][[1, 3]]).all() and (got[0][[1, 3]] == -1).all()
    for g, c in zip(got, clean):
        assert same_bits(g[[0, 2, 4, 5]], c[[0, 2, 4, 5]])


# ---- synthesis ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cf", [1, 63, 64, 65, APP_CELLS + 1, 2 * APP_CELLS + 1])
@pytest.mark.parametrize("f32", [False, True])
def test_mean_of_one_analog_copies_the_library_row(ctx, Cf, f32):
    case = make_case(seed=8, Tl=40, Tq=APP_ROWS + 3, Cf=Cf, f32=f32)
    case["F"][:, 0] = -0.0
    got = gpu(ctx, case, 1, kind="mean")
    check(got, oracle(case, 1, kind="mean"))
    rows = case["F"][got[0][:, 0]].astype(np.float64)
    assert np.array_equal(got[4], rows) and not np.signbit(got[4][:, 0]).any()  # -0.0 becomes +0.0
    assert same_bits(got[4][:, 1:], rows[:, 1:])


def test_nan_fine_cells_and_row_ranges_and_leading_dimensions(ctx):
    case = make_case(seed=9, Tl=80, Tq=2 * APP_ROWS + 5, Cf=130, f32=True)
    clean = gpu(ctx, case, 7)
    case["F"][:, 17] = np.nan  # a masked fine cell
    got = gpu(ctx, case, 7)
    exp = oracle(case, 7)
    check(got, exp)
    keep = np.arange(130) != 17
    assert np.isnan(got[4][:, 17]).all() and same_bits(got[4][:, keep], clean[4][:, keep])
    for rows in ((0, 1), (3, APP_ROWS + 4), (APP_ROWS, 2 * APP_ROWS + 5)):
        part = gpu(ctx, case, 7, rows=rows)
        assert nan_equal_bits(part[4], got[4][rows[0]:rows[1]])
    padded = gpu(ctx, case, 7, ld_f=130 + 3, ld_out=130 + 5)
    assert nan_equal_bits(padded[4], got[4])


def test_engine_refusals(ctx):
    case = make_case(Tl=20, Tq=3, Cf=4)
    L, Q, wc = case["L"], case["Q"], case["wc"]
    with pytest.raises(ValueError, match="k = 33"):
        ctx.ca_select(L, Q, wc, 33)
    with pytest.raises(ValueError, match=r"wc\[1\] = -1"):
        ctx.ca_select(L, Q, np.where(np.arange(12) == 1, -1.0, wc), 3)
    with pytest.raises(ValueError, match="no column is used"):
        ctx.ca_select(L, Q, np.zeros(12), 3)
    with pytest.raises(ValueError, match="period = 0 with window = 2"):
        ctx.ca_select(L, Q, wc, 3, period=0, window=2)
    idx, dist, status = ctx.ca_select(L, Q, wc, 3)
    with pytest.raises(ValueError, match="ridge"):
        ctx.ca_weights(L, Q, wc, idx, dist, status, ridge=-1.0)
    with pytest.raises(ValueError, match="kind="):
        ctx.ca_weights(L, Q, wc, idx, dist, status, kind="median")
    w = ctx.ca_weights(L, Q, wc, idx, dist, status)
    with pytest.raises(ValueError, match=r"rows \[2, 9\)"):
        ctx.ca_apply(ctx.to_device(case["F"]), idx, w, 2, 9)


# ---- through Python -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids(ctx):
    from skdownscale_amd import ConstructedAnalogs, GridArray

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
    ca = ConstructedAnalogs(n_analogs=8, window=20, ctx=ctx).fit(c, f)
    pred = ca.predict(t)
    wc = np.repeat(np.cos(np.deg2rad(lat_c)), 4)
    exp = co.constructed(coarse.reshape(len(time_l), 12), target.reshape(90, 12), wc, fine.reshape(len(time_l), 130), 8, co.REGRESSION, 1e-6,
                         time_l.dayofyear.to_numpy(), time_q.dayofyear.to_numpy(), 366, 20, np.full(len(time_l), -1), np.full(90, -1))
    return dict(ca=ca, pred=pred, exp=exp, obs=o, fine=f, target=t)


def test_predict_values(grids):
    from skdownscale_amd import ConstructedGridArray

    ca, pred, exp = grids["ca"], grids["pred"], grids["exp"]
    assert isinstance(pred, ConstructedGridArray) and not pred.computed and pred.dims == ("time", "lat", "lon") and pred.shape == (90, 10, 13)
    assert np.array_equal(ca.analog_index_, exp[0]) and nan_equal_bits(ca.analog_distance_, exp[1])
    assert nan_equal_bits(ca.weights_, exp[2]) and np.array_equal(ca.status_, exp[3]) and (ca.status_ == co.OK).all()
    assert nan_equal_bits(pred.values, exp[4].reshape(90, 10, 13))
    assert np.isnan(pred.values[:, 0, 0]).all() and np.isfinite(pred.values[:, 1:, :]).all()


def test_compare_takes_the_field_from_hbm(grids):
    from skdownscale_amd.timesource import takes_whole

    ca, obs = grids["ca"], grids["obs"]
    fresh = ca.predict(grids["target"])
    assert takes_whole(fresh, "any", "time")
    got = fresh.compare(obs).rmse().values
    assert not fresh.computed
    host = fresh.compute().compare(obs).rmse().values
    assert nan_equal_bits(got, host)
    d = grids["exp"][4].reshape(90, 10, 13) - obs.values
    assert np.allclose(got[1:, :], np.sqrt((d * d).mean(axis=0))[1:, :], rtol=1e-12)


def test_resample_through_the_block_producer(grids):
    fresh = grids["ca"].predict(grids["target"])
    whole = fresh.resample(time="MS").mean().values
    assert not fresh.computed
    blocked = fresh.resample(time="MS", scratch_bytes=31 * 130 * 8).mean().values  # 31 rows per block: January, February, March
    assert whole.shape == (3, 10, 13) and nan_equal_bits(blocked, whole)
    v = grids["exp"][4].reshape(90, 10, 13)
    assert np.allclose(whole[:, 1:], np.stack([v[:31].mean(0), v[31:59].mean(0), v[59:].mean(0)])[:, 1:], rtol=1e-12)


def test_isel_of_a_cell_window_stays_lazy(grids):
    from skdownscale_amd import ConstructedGridArray

    fresh = grids["ca"].predict(grids["target"])
    win = fresh.isel(lat=slice(2, 7), lon=slice(4, 13), time=slice(10, 50))
    assert isinstance(win, ConstructedGridArray) and not win.computed and not fresh.computed and win.shape == (40, 5, 9)
    assert nan_equal_bits(win.values, grids["exp"][4].reshape(90, 10, 13)[10:50, 2:7, 4:13])
    assert len(win.coords["lat"]) == 5 and len(win.coords["time"]) == 40
