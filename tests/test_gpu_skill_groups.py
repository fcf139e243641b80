"""GPU: skill_groups_kernel (csrc/sd_skill.hip) through Context.skill_groups / sd_skill_groups, and the lazy
GridArray.compare(...).groupby(...) surface for both statistic families.

The defining property: group g is evaluated exactly as sd_skill evaluates one bin whose steps are the rows with group == g in ascending
order.  So everything is compared bit for bit (``same``): with the grouped oracle (tests/_grouped_pair_oracle.py) and with
``ctx.skill`` on the fields gathered on the host, ``(a[rows], b[rows], offsets)``."""
import numpy as np
import pandas as pd
import pytest

import _grouped_pair_oracle as gp
import _skill_oracle as sk
import _twosample_oracle as ts

pytestmark = pytest.mark.gpu

FEW = 16  # sdgb::kFewGroups (pinned by tests/test_skill_groups_plan.py): up to here a wave takes one group, beyond it two
# T = 97 in G = 11 groups dealt out of order: an id that never occurs first, in the middle and last; one row; a partial, a whole and a
# whole + 1 batch of 8 rows; two whole and two whole + 1; 31
SIZES = [0, 1, 7, 8, 9, 16, 17, 0, 31, 8, 0]
CELLS = [1, 2, 63, 64, 65, 130, 256, 260]
PAIRS = [(np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32)]
STATS = list(sk.STATS)


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def deal(rng, sizes):
    """group ids with ``sizes[g]`` rows of group g, in a shuffled order"""
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def fields(rng, shape, nan_share=0.05):
    """a pair of fields in multiples of 1 / 8 (exact in float32 too) with NaN in both, partly at the same places"""
    a = np.round(rng.normal(size=shape) * 16.0) / 8.0
    b = a + np.round(rng.normal(size=shape) * 4.0) / 8.0
    a[rng.random(shape) < nan_share] = np.nan
    b[rng.random(shape) < nan_share] = np.nan
    return a, b


def inside(ctx, host, ld, lead):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart"""
    T, C = host.shape
    if (ld, lead) == (C, 0):
        return ctx.to_device(host, host.dtype)
    parent = np.full((T, ld), 7.0, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    return ctx.to_device(parent, host.dtype).cells(lead, lead + C)


def run(ctx, a, b, group, G, stats, layout=None, what=""):
    """Context.skill_groups in a layout (ld and lead of a, of b, of the output, rows between the planes beyond G) -> host
    [nstat * G, C]; everything of the output's parent outside the result must stay untouched"""
    T, C = a.shape
    n = len(stats)
    ld_a, lead_a, ld_b, lead_b, ld_out, lead_out, extra = layout or (C, 0, C, 0, C, 0, 0)
    da, db = inside(ctx, a, ld_a, lead_a), inside(ctx, b, ld_b, lead_b)
    plane = G + extra
    parent = ctx.to_device(np.full((n * plane, ld_out), 7.0))
    view = parent if (ld_out, lead_out) == (C, 0) else parent.cells(lead_out, lead_out + C)
    if extra == 0:
        out = ctx.skill_groups(da, db, group, G, stats, out=view)
        assert out is view
    else:
        ctx.skill_groups(da, db, group, G, stats, out=view.rows(0, G), plane_rows=plane)
    back = parent.to_host().reshape(n, plane, ld_out)
    untouched = np.ones(back.shape, dtype=bool)
    untouched[:, :G, lead_out:lead_out + C] = False
    assert (back[untouched] == 7.0).all(), f"{what}: padding written"
    return back[:, :G, lead_out:lead_out + C].reshape(n * G, C).copy()


def gathered(ctx, a, b, group, G, stats):
    """the binned call on the fields gathered group by group on the host"""
    rows, offsets = gp.tables(group, G)
    return ctx.skill(np.ascontiguousarray(a[rows]), np.ascontiguousarray(b[rows]), offsets, stats).to_host()


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} want {want[bad][0]!r}"


@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C):
    rng = np.random.default_rng(7000 + C)
    group = deal(rng, SIZES)
    G = len(SIZES)
    assert len(group) == 97 and G < FEW and (np.diff(np.flatnonzero(group == 8)) > 1).any()  # no run of consecutive rows
    a64, b64 = fields(rng, (97, C))
    a64[group == 8, 0] = np.nan  # a group without a valid pair in cell 0
    for ta, tb in PAIRS:
        a, b = a64.astype(ta), b64.astype(tb)
        what = f"C={C} {np.dtype(ta).name} {np.dtype(tb).name}"
        want = gp.skill(a, b, group, G, STATS)
        got = run(ctx, a, b, group, G, STATS, what=what)
        same(got, want, what)
        same(got, gathered(ctx, a, b, group, G, STATS), what + " against ctx.skill on the gathered fields")
        for s, stat in enumerate(STATS):  # one by one: the same rows as in the call for all seven
            same(run(ctx, a, b, group, G, [stat]), want[s * G:(s + 1) * G], f"{what} {stat} alone")
    got = got.reshape(len(STATS), G, C)
    empty = np.array(SIZES) == 0
    assert (got[0][empty] == 0.0).all() and np.isnan(got[1:][:, empty]).all()  # ids that never occur
    assert got[0, 8, 0] == 0.0 and np.isnan(got[1:, 8, 0]).all()  # the all-invalid group
    t = int(np.flatnonzero(group == 1)[0])  # the group of one row: one pair where both are there
    full = ~np.isnan(a64[t]) & ~np.isnan(b64[t])
    assert np.isnan(got[5:, 1][:, full]).all() and np.isfinite(got[4, 1][full]).all() and (got[0, 1][full] == 1.0).all()


@pytest.mark.parametrize("G", [1, 4, FEW - 1, FEW, FEW + 1, FEW + 9, 2 * FEW + 1])
def test_group_counts_on_both_sides_of_the_few_groups_edge(ctx, G):
    """G <= 16: one group per wave; beyond: two, and an odd G ends inside a wave's pair of groups (the g >= G break)"""
    rng = np.random.default_rng(G)
    sizes = rng.integers(0, 12, G)
    sizes[rng.integers(0, G)] += 3
    group = deal(rng, sizes)
    for C in (65, 130):
        a, b = fields(rng, (len(group), C))
        got = ctx.skill_groups(a, b, group, G, STATS)
        assert got.shape == (len(STATS) * G, C)
        same(got.to_host(), gp.skill(a, b, group, G, STATS), f"G={G} C={C}")
        same(got.to_host(), gathered(ctx, a, b, group, G, STATS), f"G={G} C={C} gathered")


@pytest.mark.parametrize("lengths", [[97], SIZES, [5] * FEW, [3, 0] * FEW + [3]], ids=["G=1", "G=11", "G=16", "G=33"])
def test_groups_that_are_runs_of_rows_equal_the_binned_call(ctx, lengths):
    rng = np.random.default_rng(len(lengths))
    group = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for C, (ta, tb) in zip((63, 130, 260, 64), PAIRS):
        a64, b64 = fields(rng, (len(group), C))
        a, b = a64.astype(ta), b64.astype(tb)
        same(ctx.skill_groups(a, b, group, len(lengths), STATS).to_host(), ctx.skill(a, b, offsets, STATS).to_host(), f"G={len(lengths)} C={C}")


def test_constructed_cells(ctx):
    nan, inf = np.nan, np.inf
    sizes = [20, 17, 1, 24]
    rng = np.random.default_rng(9)
    group = deal(rng, sizes)
    T, C = len(group), 8
    a, b = fields(rng, (T, C), 0.0)
    first = [int(np.flatnonzero(group == g)[0]) for g in range(4)]
    last = [int(np.flatnonzero(group == g)[-1]) for g in range(4)]
    a[(group == 0) & (np.arange(T) != last[0]), 0] = nan   # 0: group 0 with one valid pair, its last row
    a[:, 1] = 2.5                                           # 1: a constant series
    a[first[1], 2] = inf                                    # 2: an inf sample in a
    b[first[3], 3] = -inf                                   # 3: one in b
    a[last[3], 4] = b[last[3], 4] = inf                     # 4: inf in both at the same step: inf - inf
    b[group == 1, 5] = nan                                  # 5: a group with NaN only in b: no valid pair
    b[first[0], 6] = b[last[3], 6] = nan                    # 6: isolated NaN only in b
    b[:, 7] = a[:, 7] + 0.5                                 # 7: a constant offset
    for ta, tb in PAIRS:
        what = f"{np.dtype(ta).name} {np.dtype(tb).name}"
        x, y = a.astype(ta), b.astype(tb)
        got = run(ctx, x, y, group, 4, STATS, what=what)
        same(got, gp.skill(x, y, group, 4, STATS), what)
        same(got, gathered(ctx, x, y, group, 4, STATS), what + " gathered")
    count, bias, ratio, mae, rmse, corr, std_ratio = run(ctx, a, b, group, 4, STATS).reshape(7, 4, C)
    assert count[0, 0] == 1 and np.isnan(corr[0, 0]) and np.isnan(std_ratio[0, 0]) and rmse[0, 0] == abs(a[last[0], 0] - b[last[0], 0])
    assert np.isnan(corr[2]).all() and np.isnan(std_ratio[2]).all() and np.isfinite(rmse[2, [0, 1, 2, 3, 4, 6, 7]]).all()  # the group of one row
    assert np.isnan(corr[[0, 1, 3], 1]).all() and (std_ratio[[0, 1, 3], 1] == 0.0).all()  # a constant: no correlation, no spread
    assert bias[1, 2] == inf and rmse[1, 2] == inf and np.isnan(corr[1, 2]) and np.isfinite(bias[[0, 2, 3], 2]).all()
    assert bias[3, 3] == inf and mae[3, 3] == inf and np.isnan(corr[3, 3])
    assert np.isnan(bias[3, 4]) and np.isnan(rmse[3, 4]) and count[3, 4] == 24  # inf - inf is NaN, the pair is valid
    assert count[1, 5] == 0 and np.isnan([bias[1, 5], ratio[1, 5], mae[1, 5], rmse[1, 5], corr[1, 5], std_ratio[1, 5]]).all()
    assert list(count[:, 5]) == [20, 0, 1, 24] and list(count[:, 6]) == [19, 17, 1, 23]
    assert (bias[:, 7] == -0.5).all() and (mae[:, 7] == 0.5).all() and (rmse[:, 7] == 0.5).all()
    d = ctx.to_device(a)  # a == b through the same pointer
    twice = ctx.skill_groups(d, d, group, 4, ["bias", "mae", "ratio"]).to_host()
    same(twice, gp.skill(a, a, group, 4, ["bias", "mae", "ratio"]), "the same pointer")


@pytest.mark.parametrize("C", [63, 130, 260])
def test_views_give_the_bits_of_the_contiguous_call(ctx, C):
    rng = np.random.default_rng(50 + C)
    group = deal(rng, SIZES)
    G = len(SIZES)
    a64, b64 = fields(rng, (97, C))
    even = C + 6 if C % 2 == 0 else C + 5
    odd = C + 5 - C % 2
    # (name, ld and lead of a, of b, of the output, rows between two planes beyond G)
    layouts = [("padded by fours", (C + 8, 4, C + 12, 8, C + 4, 4, 2)), ("padded even", (even + 2, 4, even + 4, 2, even, 2, 2)),
               ("padded odd", (odd, 4, odd + 2, 1, odd - 2, 2, 1)), ("a off by one element", (C + 4, 1, C, 0, C, 0, 0)),
               ("b off by one element", (C, 0, C + 4, 1, C, 0, 0)), ("output off by one double", (C, 0, C, 0, C + 2, 1, 1))]
    for ta, tb in PAIRS:
        a, b = a64.astype(ta), b64.astype(tb)
        tight = run(ctx, a, b, group, G, STATS)
        same(tight, gp.skill(a, b, group, G, STATS), "tight")
        for name, layout in layouts:
            what = f"C={C} {np.dtype(ta).name} {np.dtype(tb).name} {name}"
            same(run(ctx, a, b, group, G, STATS, layout, what), tight, what)


def test_the_host_twin(ctx):
    rng = np.random.default_rng(6)
    group = deal(rng, SIZES)
    G = len(SIZES)
    for C in (63, 130, 260):
        a64, b64 = fields(rng, (97, C))
        for ta, tb in PAIRS:
            a, b = a64.astype(ta), b64.astype(tb)
            got = ctx.skill_groups(a, b, group, G, STATS).to_host()
            same(ctx.skill_groups_host(a, b, group, G, STATS), got, "sd_skill_groups")
            same(ctx.skill_groups(ctx.to_device(a, ta), ctx.to_device(b, tb), group, G, STATS).to_host(), got, "resident sources")
            same(ctx.skill_groups(a.astype(np.float64), b.astype(np.float64), group, G, STATS).to_host(), got, "the widened sources")


def test_refusals_through_the_c_abi_launch_nothing(ctx):
    from skdownscale_amd._lib import check, ptr

    x = np.zeros((10, 4))
    a, b, out = ctx.to_device(x), ctx.to_device(x + 1.0), ctx.empty((6, 4))
    ids = np.array([1, 0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=np.int32)
    codes = np.array([1, 4, 0, 0, 0, 0, 0], dtype=np.intc)

    def call(ld_a=4, ld_b=4, T=10, C=4, group=ids, G=2, stats=codes, nstat=3, ld_out=4, stride=8):
        check(ctx.lib.sd_skill_groups_dev(ctx.handle, a.vptr, 0, ld_a, b.vptr, 0, ld_b, T, C, ptr(group), G, ptr(stats), nstat, out.vptr, ld_out, stride))

    ctx.prof_reset()
    ctx.prof_enable(True)
    who = "sd_skill_groups: "
    bad = ids.copy()
    bad[3] = 2
    for kw, msg in ((dict(stats=np.array([1, 7, 0, 0, 0, 0, 0], dtype=np.intc)), who + r"unknown statistic code 7 \(stats\[1\]\)"),
                    (dict(nstat=0), who + "nstat = 0, expected 1 to 7 statistics"), (dict(nstat=8), who + "nstat = 8"),
                    (dict(T=0), who + r"bad sizes \(T=0, C=4\)"), (dict(C=-1), who + "bad sizes"),
                    (dict(ld_a=3), who + "ld_a = 3 is less than the 4 cells of a row"),
                    (dict(ld_b=3), who + "ld_b = 3 is less than the 4 cells of a row"),
                    (dict(ld_out=3), who + "ld_out = 3 is less than the 4 cells of a row"),
                    (dict(stride=7), who + r"stride_out = 7 is less than the 8 elements of one statistic \(G \* ld_out\)"),
                    (dict(ld_a=1 << 61), who + "field too large"),
                    (dict(G=0, stride=0), who + r"bad sizes \(G=0\)"), (dict(G=-2, stride=0), who + r"bad sizes \(G=-2\)"),
                    (dict(group=bad), who + r"group\[3\] = 2 lies outside the 2 groups"),
                    (dict(G=1, group=ids), who + r"group\[0\] = 1 lies outside the 1 groups"),
                    (dict(group=bad, ld_b=3), who + "ld_b = 3"), (dict(group=bad, G=0, stride=0), who + r"bad sizes \(G=0\)")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match=who + r"group\[1\] = 5 lies outside the 3 groups"):
        ctx.skill_groups_host(x, x, [0, 5, 1, 2, 0, 0, 0, 0, 0, 0], 3, ["bias"])
    with pytest.raises(ValueError, match=who + r"group\[9\] = -1 lies outside the 3 groups"):
        ctx.skill_groups(x, x, [0, 1, 1, 2, 0, 0, 0, 0, 0, -1], 3, ["bias"])
    assert "skill_groups_kernel" not in ctx.prof() and "skill_kernel" not in ctx.prof()  # nothing was launched
    call()
    assert ctx.prof()["skill_groups_kernel"]["launches"] == 1 and "skill_kernel" not in ctx.prof()
    ctx.prof_enable(False)
    assert np.array_equal(out.to_host(), np.array([[-1.0] * 4] * 2 + [[1.0] * 4] * 2 + [[4.0] * 4, [6.0] * 4]))  # bias, rmse, count
    # the Python wrapper
    with pytest.raises(ValueError, match="skill statistic 'kge'"):
        ctx.skill_groups(x, x, ids, 2, ["kge"])
    with pytest.raises(ValueError, match=r"group: expected one group id per row \(10\), got shape \(9,\)"):
        ctx.skill_groups(x, x, ids[:9], 2, ["bias"])
    with pytest.raises(ValueError, match=r"sd_skill_groups: bad sizes \(G=0\)"):
        ctx.skill_groups(x, x, ids, 0, ["bias"])
    with pytest.raises(ValueError, match="b: expected a \\[T, C\\] field of shape \\(10, 4\\)"):
        ctx.skill_groups(x, x[:, :3], ids, 2, ["bias"])


# ---- the lazy surface: two years of daily data over 6 x 7 cells -------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2002-12-31", freq="D")
MONTH = (np.asarray(TIME.month) - 1).astype(np.int32)
SEASON = np.array([0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 3, 0], dtype=np.int32)[MONTH]  # ids of the sorted labels DJF, JJA, MAM, SON
LAT, LON = np.linspace(42.0, 38.0, 6), np.linspace(-110.0, -106.0, 7)
NAMES = ["bias", "rmse", "corr"]
CELLS_E2E = 42


def grid(values, time=TIME):
    from skdownscale_amd import GridArray

    return GridArray(values, ("time", "lat", "lon"), dict(time=time, lat=LAT, lon=LON))


@pytest.fixture(scope="module")
def obs():
    rng = np.random.default_rng(21)
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(len(TIME)) / 365.25)
    v = 285.0 + season[:, None, None] + 4.0 * rng.normal(size=(len(TIME), 6, 7))
    v[rng.random(v.shape) < 0.01] = np.nan
    return grid(v)


@pytest.fixture(scope="module")
def model(obs):
    rng = np.random.default_rng(22)
    v = obs.values + 0.5 + rng.normal(size=obs.shape)
    v[rng.random(v.shape) < 0.01] = np.nan
    v[np.isnan(obs.values) & (rng.random(v.shape) < 0.5)] = 1.0  # (NaN only in the observations at some steps)
    return grid(v)


def test_host_against_host_by_month_and_by_season(ctx, obs, model):
    fa, fb = model.values.reshape(730, CELLS_E2E), obs.values.reshape(730, CELLS_E2E)
    want = gp.skill(fa, fb, MONTH, 12, NAMES)
    for scratch_bytes in (None, 1):  # both sources come whole whatever the room
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = model.compare(obs, **kw).groupby("time.month").indices(NAMES)
        assert not lazy.computed and lazy.dims == ("index", "month", "lat", "lon") and lazy.shape == (3, 12, 6, 7)
        same(lazy.values.reshape(36, CELLS_E2E), want, f"by month scratch_bytes={scratch_bytes}")
    assert list(lazy.coords["month"]) == list(range(1, 13))
    ks = model.compare(obs).groupby("time.season").ks()
    assert ks.dims == ("season", "lat", "lon") and list(ks.coords["season"]) == ["DJF", "JJA", "MAM", "SON"]
    same(ks.values.reshape(4, CELLS_E2E), gp.twosample(fa, fb, SEASON, 4, "ks"), "ks by season")
    dist = model.compare(obs).groupby("time.month").distribution(["ks", "perkins", "na", "nb"], width=0.5, origin=0.25)
    same(dist.values.reshape(48, CELLS_E2E), gp.twosample(fa, fb, MONTH, 12, ts.STATS, 0.5, 0.25), "distribution by month")
    # one statistic, a selection along the other dims, float32 against float64 with the other array in another order of dims
    cut = model.compare(obs).groupby("time.month").corr().isel(lat=slice(2, 5))
    assert not cut.computed and np.array_equal(cut.values, want.reshape(3, 12, 6, 7)[2][:, 2:5], equal_nan=True)
    a32 = grid(model.values.astype(np.float32))
    got = a32.compare(obs.transpose("lon", "time", "lat")).groupby("time.season").indices(NAMES)
    same(got.values.reshape(12, CELLS_E2E), gp.skill(a32.values.reshape(730, CELLS_E2E), fb, SEASON, 4, NAMES), "float32 a")
    mid = model.transpose("lat", "time", "lon").compare(obs).groupby("time.month").rmse()
    assert mid.dims == ("lat", "month", "lon")
    same(np.ascontiguousarray(mid.values.transpose(1, 0, 2)).reshape(12, CELLS_E2E), want[12:24], "time in the middle")
    doy = model.compare(obs).groupby("time.dayofyear").bias()  # 365 groups of two rows: two groups per wave
    same(doy.values.reshape(365, CELLS_E2E), gp.skill(fa, fb, np.asarray(TIME.dayofyear) - 1, 365, "bias"), "by day of year")


def test_a_lazy_disaggregate_result_against_a_host_array(ctx, obs, model):
    labels = pd.date_range("2001-01-01", periods=24, freq="MS")
    clean = grid(np.nan_to_num(obs.values, nan=285.0))
    target = np.asarray(model.resample(time="MS").mean().values)
    want_field = grid(target, labels).disaggregate(clean, years="same").values.reshape(730, CELLS_E2E)
    fb = obs.values.reshape(730, CELLS_E2E)
    for scratch_bytes in (None, 1):
        daily = grid(target, labels).disaggregate(clean, years="same")
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        got = daily.compare(obs, **kw).groupby("time.month").indices(NAMES).values
        assert not daily.computed  # taken whole from HBM
        same(got.reshape(36, CELLS_E2E), gp.skill(want_field, fb, MONTH, 12, NAMES), f"disaggregated scratch_bytes={scratch_bytes}")
    daily = grid(target, labels).disaggregate(clean, years="same")
    same(daily.compare(obs).groupby("time.season").ks().values.reshape(4, CELLS_E2E), gp.twosample(want_field, fb, SEASON, 4, "ks"), "ks of the lazy field")
    assert not daily.computed


def test_an_unchunked_interp_like_source(ctx, obs):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(5)
    coarse = GridArray(285.0 + 5.0 * rng.normal(size=(730, 3, 3)), ("time", "lat", "lon"),
                       dict(time=TIME, lat=np.array([42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0])))
    fine_host = coarse.interp_like(obs).compute().values.reshape(730, CELLS_E2E)
    fb = obs.values.reshape(730, CELLS_E2E)
    for scratch_bytes in (None, 1):
        fine = coarse.interp_like(obs)
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        same(fine.compare(obs, **kw).groupby("time.month").indices(NAMES).values.reshape(36, CELLS_E2E), gp.skill(fine_host, fb, MONTH, 12, NAMES),
             f"interp_like scratch_bytes={scratch_bytes}")
        same(fine.compare(obs, **kw).groupby("time.season").ks().values.reshape(4, CELLS_E2E), gp.twosample(fine_host, fb, SEASON, 4, "ks"), "ks")
        assert not fine.computed  # the fine field never came to the host
