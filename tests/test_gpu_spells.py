"""GPU: spells_kernel (csrc/sd_spells.hip) through Context.spells / sd_spells against tests/_spells_oracle.py, and the lazy
GridArray.where surface on host, interp_like and lazy HBM sources.

Every statistic is an integer or one division of two integers, so everything here is compared bit for bit (np.array_equal with
equal_nan): with the oracle, and between layouts, cells per lane, block sizes and the host-buffer twin."""
import warnings

import numpy as np
import pandas as pd
import pytest

import _spells_oracle as sp

pytestmark = pytest.mark.gpu

GROUP = 8  # bins of a workgroup (sdbn::kBinsPerGroup, pinned by tests/test_spells_plan.py); 8 rows are in flight per batch
# T = 120: an empty first, middle and last bin; lengths 1, 7, 8, 9 (one row, a partial, a whole and a whole + partial batch), 16, 31;
# M = 12 is more than one workgroup's run of bins
LENGTHS = [0, 1, 7, 8, 9, 31, 0, 31, 8, 16, 9, 0]
CELLS = [1, 63, 64, 65, 130, 257]
OPS = [">", ">=", "<", "<="]
STATS = list(sp.STATS)


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def table(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def quarters(rng, shape, nan_share):
    """multiples of 0.25 (exact in float32 too, so samples tie with thresholds) with a share of NaN"""
    x = np.round(rng.normal(size=shape) * 4.0) / 4.0
    x[rng.random(shape) < nan_share] = np.nan
    return x


def inside(ctx, host, ld, lead):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart"""
    T, C = host.shape
    if (ld, lead) == (C, 0):
        return ctx.to_device(host, host.dtype)
    parent = np.full((T, ld), 7.0, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    return ctx.to_device(parent, host.dtype).cells(lead, lead + C)


def run(ctx, host, op, thr, offsets, stats, L=1, group=None, layout=None, what=""):
    """Context.spells in a layout (source ld, lead, table ld, lead, output ld, lead, rows between the planes beyond M) -> host
    [nstat * M, C]; everything of the output's parent outside the result must stay untouched"""
    T, C = host.shape
    M, n = len(offsets) - 1, len(stats)
    ld, lead, ld_t, lead_t, ld_out, lead_out, extra = layout or (C, 0, C, 0, C, 0, 0)
    src = inside(ctx, host, ld, lead)
    dthr = inside(ctx, np.ascontiguousarray(thr, dtype=np.float64), ld_t, lead_t) if np.ndim(thr) == 2 else thr
    plane = M + extra
    parent = ctx.to_device(np.full((n * plane, ld_out), 7.0))
    view = parent if (ld_out, lead_out) == (C, 0) else parent.cells(lead_out, lead_out + C)
    if extra == 0:
        out = ctx.spells(src, op, dthr, offsets, stats, L, group, out=view)
        assert out is view
    else:
        ctx.spells(src, op, dthr, offsets, stats, L, group, out=view.rows(0, M), plane_rows=plane)
    back = parent.to_host().reshape(n, plane, ld_out)
    untouched = np.ones(back.shape, dtype=bool)
    untouched[:, :M, lead_out:lead_out + C] = False
    assert (back[untouched] == 7.0).all(), f"{what}: padding written"
    return back[:, :M, lead_out:lead_out + C].reshape(n * M, C).copy()


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]} want {want[bad][0]}"


@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C):
    rng = np.random.default_rng(2000 + C)
    offsets = table(LENGTHS)
    T, M = int(offsets[-1]), len(LENGTHS)
    assert T == 120 and M == GROUP + 4
    x64 = quarters(rng, (T, C), 0.05)
    long = int(np.flatnonzero(np.diff(offsets) == 31)[0])
    x64[offsets[long]:offsets[long + 1], 0] = np.nan  # an all-NaN bin in cell 0
    per_cell = quarters(rng, (1, C), 0.1 if C > 1 else 0.0)
    by_group = quarters(rng, (5, C), 0.1)
    group = rng.integers(0, 5, size=T).astype(np.int32)
    even = C + 6 if C % 2 == 0 else C + 5
    odd = C + 5 - C % 2
    # (name, source ld, lead, table ld, lead, output ld, lead, rows between two planes beyond M)
    layouts = [("tight", (C, 0, C, 0, C, 0, 0)), ("padded even", (even + 2, 4, even + 4, 2, even, 2, 2)),
               ("padded odd", (odd, 4, odd + 2, 1, odd - 2, 2, 1)), ("output off by one double", (C, 0, C, 0, C + 2, 1, 1))]
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        for kind, thr, ids in (("scalar", 0.25, None), ("per cell", per_cell, None), ("table", by_group, group)):
            for k, op in enumerate(OPS):
                L = (1, 2, 3, 7)[k]
                want = sp.spells(host, offsets, op, thr, STATS, L, ids)
                for name, layout in layouts:
                    what = f"C={C} {np.dtype(dtype).name} {kind} {op} L={L} {name}"
                    same(run(ctx, host, op, thr, offsets, STATS, L, ids, layout, what), want, what)
            # one by one: the same rows as in the call for all six
            want = sp.spells(host, offsets, ">", thr, STATS, 2, ids).reshape(len(STATS), M, C)
            for s, stat in enumerate(STATS):
                same(run(ctx, host, ">", thr, offsets, [stat], 2, ids), want[s], f"C={C} {np.dtype(dtype).name} {kind} {stat} alone")
    empty = np.diff(offsets) == 0
    got = run(ctx, x64, ">", 0.25, offsets, STATS).reshape(len(STATS), M, C)
    assert np.isnan(got[2][empty]).all() and (got[[0, 1, 3, 4, 5]][:, empty] == 0.0).all()  # empty bins
    assert np.isnan(got[2, long, 0]) and (got[[0, 1, 3, 4, 5], long, 0] == 0.0).all()  # the all-NaN bin


def test_constructed_series(ctx):
    nan, inf = np.nan, np.inf
    lengths = [7, 9, 12, 12, 5]
    offsets = table(lengths)
    b = offsets
    T, C = int(offsets[-1]), 10
    x = np.zeros((T, C))
    thr = np.ones((2, C))
    group = np.zeros(T, dtype=np.int32)
    x[b[1] - 1, 0] = x[b[2] - 1, 0] = 2.0        # 0: the last step of a bin of 7 and of a bin of 9 is the only hit
    x[b[2] + 6:b[2] + 11, 1] = 2.0                # 1: a run over steps 6 .. 10 of a bin: across the batch boundary
    x[b[3] - 3:b[3] + 4, 2] = 2.0                 # 2: a run of 3 to the end of a bin that goes on for 4 in the next
    x[b[2] + 2:b[2] + 11, 3] = 2.0                # 3: a NaN sample in the middle of a run of 9
    x[b[2] + 6, 3] = nan
    x[b[3] + 2:b[3] + 11, 4] = 2.0                # 4: a NaN threshold in the middle of a run of 9 (the step of group 1)
    thr[1, 4] = nan
    group[b[3] + 6] = 1
    x[:, 5] = 2.0                                 # 5: every step a hit
    x[:, 6] = 0.0                                 # 6: none
    x[:, 7] = nan                                 # 7: no valid step
    x[:, 8] = 1.0                                 # 8: x == t: no hit under > and <, all under >= and <=
    x[:, 9] = np.resize([inf, inf, -inf, 2.0, -inf], T)  # 9: +-inf are ordinary values
    for op in OPS:
        for L in (1, 2, 6, 12, 13):
            for dtype in (np.float64, np.float32):
                what = f"{op} L={L} {np.dtype(dtype).name}"
                same(run(ctx, x.astype(dtype), op, thr, offsets, STATS, L, group, what=what), sp.spells(x, offsets, op, thr, STATS, L, group), what)
    got = run(ctx, x, ">", thr, offsets, STATS, 1, group).reshape(6, 5, C)
    valid, count, frac, longest, days, spells = got
    assert list(longest[:, 0]) == [1, 1, 0, 0, 0] and list(count[:, 0]) == [1, 1, 0, 0, 0]  # the clamped rows did not extend the run
    assert longest[2, 1] == 5 and spells[2, 1] == 1
    assert list(longest[:, 2]) == [0, 0, 3, 4, 0] and list(spells[:, 2]) == [0, 0, 1, 1, 0]  # cut at the bin's end
    assert longest[2, 3] == 4 and spells[2, 3] == 2 and valid[2, 3] == 11 and count[2, 3] == 8
    assert longest[3, 4] == 4 and spells[3, 4] == 2 and valid[3, 4] == 11 and count[3, 4] == 8
    assert list(longest[:, 5]) == lengths and list(days[:, 5]) == lengths and (frac[:, 5] == 1.0).all() and (spells[:, 5] == 1).all()
    assert (got[[0]][:, :, 6] == np.array(lengths)).all() and (got[[1, 2, 3, 4, 5]][:, :, 6] == 0.0).all()
    assert np.isnan(frac[:, 7]).all() and (got[[0, 1, 3, 4, 5]][:, :, 7] == 0.0).all()
    assert (count[:, 8] == 0).all() and (run(ctx, x, ">=", thr, offsets, ["count"], 1, group)[:, 8] == np.array(lengths)).all()
    six = run(ctx, x, ">", thr, offsets, ["spell_days", "spell_count"], 6, group).reshape(2, 5, C)
    assert list(six[0, :, 5]) == [7, 9, 12, 12, 0] and list(six[1, :, 5]) == [1, 1, 1, 1, 0] and six[0, 2, 1] == 0 and six[0, 2, 3] == 0
    at, beyond = (run(ctx, x, ">", thr, offsets, ["spell_days"], L, group)[:, 5] for L in (12, 13))
    assert list(at) == [0, 0, 12, 12, 0] and list(beyond) == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("lengths", [[120], [5] * GROUP, [13] * (GROUP + 1), [3, 0] * GROUP + [3]], ids=["M=1", "M=8", "M=9", "M=17"])
def test_bin_counts_at_the_edges_of_a_workgroup(ctx, lengths):
    rng = np.random.default_rng(len(lengths))
    offsets = table(lengths)
    T = int(offsets[-1])
    for C in (65, 130):
        x = quarters(rng, (T, C), 0.05)
        tab = quarters(rng, (3, C), 0.05)
        group = rng.integers(0, 3, size=T).astype(np.int32)
        for thr, ids in ((0.0, None), (tab, group)):
            got = ctx.spells(x, "<=", thr, offsets, STATS, 2, ids)
            assert got.shape == (len(STATS) * len(lengths), C)
            same(got.to_host(), sp.spells(x, offsets, "<=", thr, STATS, 2, ids), f"M={len(lengths)} C={C}")


def test_float32_source_and_the_host_twin(ctx):
    rng = np.random.default_rng(3)
    offsets = table(LENGTHS)
    for C in (63, 130, 260):  # one, two and four cells per lane for float32
        x32 = quarters(rng, (120, C), 0.05).astype(np.float32)
        tab = quarters(rng, (4, C), 0.05)
        group = rng.integers(0, 4, size=120).astype(np.int32)
        for thr, ids in ((0.25, None), (tab[:1], None), (tab, group)):
            got32 = ctx.spells(x32, ">=", thr, offsets, STATS, 3, ids).to_host()
            same(got32, sp.spells(x32, offsets, ">=", thr, STATS, 3, ids), f"float32 C={C}")
            same(ctx.spells(x32.astype(np.float64), ">=", thr, offsets, STATS, 3, ids).to_host(), got32, "the widened source")
            same(ctx.spells(ctx.to_device(x32, np.float32), ">=", thr, offsets, STATS, 3, ids).to_host(), got32, "resident float32")
            same(ctx.spells_host(x32, ">=", thr, offsets, STATS, 3, ids), got32, "sd_spells")
    # the comparison is made on doubles: np.float32(0.1) widened is above 0.1, np.float32(0.7) widened is below 0.7
    x = np.array([[0.1, 0.7]], dtype=np.float32)
    assert np.array_equal(ctx.spells(x, ">", 0.1, [0, 1], ["count"]).to_host(), [[1.0, 1.0]])
    assert np.array_equal(ctx.spells(x, "<", 0.7, [0, 1], ["count"]).to_host(), [[1.0, 1.0]])
    assert np.array_equal(ctx.spells(x, ">=", 0.7, [0, 1], ["count"]).to_host(), [[0.0, 0.0]])
    assert np.array_equal(ctx.spells(x, ">=", np.array([[float(np.float32(0.1)), 0.7]]), [0, 1], ["count"]).to_host(), [[1.0, 0.0]])


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def obs():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(21)
    time = pd.date_range("2001-01-01", "2003-12-31", freq="D")  # three years without a leap day: 365 day-of-year groups of 3
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(len(time)) / 365.25)
    v = 285.0 + season[:, None, None] + 4.0 * rng.normal(size=(len(time), 10, 13))
    v[rng.random(v.shape) < 0.01] = np.nan
    return GridArray(v, ("time", "lat", "lon"), dict(time=time, lat=np.linspace(42.0, 38.0, 10), lon=np.linspace(-110.0, -106.0, 13)))


YEARS = np.array([0, 365, 730, 1095])


def test_tx90p_chain_against_numpy_quantiles(ctx, obs):
    flat = obs.values.reshape(1095, 130)
    doy = np.asarray(obs.coords["time"].dayofyear) - 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (a group of three NaN: an All-NaN slice, NaN as on the device)
        q90 = np.stack([np.nanquantile(flat[doy == g], 0.9, axis=0) for g in range(365)])
    names = ["fraction", "spell_days", "count", "valid"]
    want = sp.spells(flat, YEARS, ">", q90, names, 2, doy)
    thr = obs.quantile(0.9, "time", by="time.dayofyear")
    first = None
    for scratch_bytes in (None, 800 * 130 * 8, 1):  # one block, two blocks (two years and one), one bin per block
        hot = obs.where(">", thr, by="time.dayofyear", scratch_bytes=scratch_bytes)
        lazy = hot.resample(time="YS").indices(names, min_length=2)
        assert not lazy.computed and lazy.shape == (4, 3, 10, 13)
        got = lazy.values
        assert not thr.computed  # the table stayed in HBM
        same(got.reshape(12, 130), want, f"tx90p scratch_bytes={scratch_bytes}")
        first = got if first is None else first
        assert np.array_equal(got, first, equal_nan=True)
    assert np.array_equal(lazy.device_field(ctx).to_host(), want, equal_nan=True)
    # one statistic, and a selection along the other dims that stays lazy
    one = obs.where(">", thr, by="time.dayofyear").resample(time="YS").fraction()
    same(one.values.reshape(3, 130), want[:3], "fraction alone")
    cut = one.isel(lat=slice(2, 5))
    assert not cut.computed and np.array_equal(cut.values, one.values[:, 2:5], equal_nan=True)
    # the same table as a host array, and as a per-cell threshold without by
    host = obs.where(">", q90.reshape(365, 10, 13), by="time.dayofyear").resample(time="YS").indices(names, min_length=2)
    assert np.array_equal(host.values, first, equal_nan=True)
    cell = obs.where("<", q90[180].reshape(10, 13)).resample(time="YS").longest_spell()
    same(cell.values.reshape(3, 130), sp.spells(flat, YEARS, "<", q90[180:181], "longest_spell"), "per-cell threshold")


def test_sources_of_the_lazy_surface(ctx, obs):
    from skdownscale_amd import GridArray

    flat = obs.values.reshape(1095, 130)
    names = ["count", "longest_spell", "spell_count"]
    # a float32 host source goes up as float32, block by block
    v32 = obs.values.astype(np.float32)
    a32 = GridArray(v32, obs.dims, obs.coords)
    want32 = sp.spells(v32.reshape(1095, 130), YEARS, "<", 283.15, names, 3)
    for scratch_bytes in (None, 400 * 130 * 4):
        same(a32.where("<", 283.15, scratch_bytes=scratch_bytes).resample(time="YS").indices(names, 3).values.reshape(9, 130), want32, "float32 host")
    # the whole axis is one bin and the dim is dropped; time in the middle
    fd = obs.where("<", 273.15 + 8.0).count()
    assert fd.dims == ("lat", "lon")
    same(fd.values.reshape(1, 130), sp.spells(flat, [0, 1095], "<", 281.15, "count"), "whole axis")
    mid = obs.transpose("lat", "time", "lon").where("<", 281.15).resample(time="YS").count()
    same(mid.values.transpose(1, 0, 2).reshape(3, 130), sp.spells(flat, YEARS, "<", 281.15, "count"), "time in the middle")
    # coarse.interp_like(obs): regridded block by block in HBM; the same values as the materialised fine field
    rng = np.random.default_rng(5)
    coarse = GridArray(285.0 + 5.0 * rng.normal(size=(1095, 3, 3)), ("time", "lat", "lon"),
                       dict(time=obs.coords["time"], lat=np.array([42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0])))
    fine = coarse.interp_like(obs)
    want = sp.spells(fine.compute().values.reshape(1095, 130), YEARS, ">=", 286.0, names, 2)
    for scratch_bytes in (None, 500 * 130 * 8, 1):
        lazy = coarse.interp_like(obs).where(">=", 286.0, scratch_bytes=scratch_bytes).resample(time="YS").indices(names, 2)
        same(lazy.values.reshape(9, 130), want, f"interp_like scratch_bytes={scratch_bytes}")
        assert not lazy.source.computed  # the fine field never came to the host
    # a lazy anomaly gb - clim is taken whole from HBM
    anom = obs.groupby("time.month") - obs.groupby("time.month").mean()
    values = (obs.groupby("time.month") - obs.groupby("time.month").mean()).values.reshape(1095, 130)  # (another instance: the same kernels)
    lazy = anom.where(">", 0.0).resample(time="YS").indices(names, 2)
    same(lazy.values.reshape(9, 130), sp.spells(values, YEARS, ">", 0.0, names, 2), "lazy anomaly")
    assert not anom.computed
    # a lazy monthly mean as the source: yearly counts of warm months
    monthly = obs.resample(time="MS").mean()
    warm = monthly.where(">", 288.0).resample(time="YS").count()
    same(warm.values.reshape(3, 130), sp.spells(obs.resample(time="MS").mean().values.reshape(36, 130), [0, 12, 24, 36], ">", 288.0, "count"), "lazy monthly")
    assert not monthly.computed


def test_refusals_through_the_c_abi_launch_nothing(ctx):
    from skdownscale_amd._lib import check, ptr

    x = np.zeros((10, 4))
    d, tab, out = ctx.to_device(x), ctx.to_device(np.zeros((3, 4))), ctx.empty((6, 4))
    off = np.array([0, 4, 10], dtype=np.int64)
    group = np.zeros(10, dtype=np.int32)
    codes = np.array([1, 3, 4, 0, 0, 0], dtype=np.intc)

    def call(op=0, ld=4, T=10, C=4, table=None, ld_t=4, ids=None, G=1, offsets=off, M=2, L=1, stats=codes, nstat=3, ld_out=4, stride=8):
        check(ctx.lib.sd_spells_dev(ctx.handle, d.vptr, 0, ld, T, C, op, 0.5, None if table is None else table.vptr, ld_t,
                                    None if ids is None else ptr(ids), G, ptr(offsets), M, L, ptr(stats), nstat, out.vptr, ld_out, stride))

    ctx.prof_reset()
    ctx.prof_enable(True)
    bad_group = group.copy()
    bad_group[7] = 3
    for kw, msg in ((dict(op=4), "sd_spells: unknown op code 4"),
                    (dict(stats=np.array([1, 6, 0, 0, 0, 0], dtype=np.intc)), r"sd_spells: unknown statistic code 6 \(stats\[1\]\)"),
                    (dict(nstat=0), "sd_spells: nstat = 0, expected 1 to 6 statistics"), (dict(nstat=7), "sd_spells: nstat = 7"),
                    (dict(L=0), "sd_spells: min_length = 0, expected at least 1"),
                    (dict(T=0), r"sd_spells: bad sizes \(T=0, C=4, M=2\)"), (dict(M=0), "sd_spells: bad sizes"),
                    (dict(ld=3), "sd_spells: ld = 3 is less than the 4 cells of a row"),
                    (dict(table=tab, ld_t=3, ids=group, G=3), "sd_spells: ld_t = 3 is less than the 4 cells of a row"),
                    (dict(ld_out=3), "sd_spells: ld_out = 3 is less than the 4 cells of a row"),
                    (dict(stride=7), r"sd_spells: stride_out = 7 is less than the 8 elements of one statistic \(M \* ld_out\)"),
                    (dict(table=tab, ids=group, G=0), r"sd_spells: bad sizes \(G=0\)"),
                    (dict(table=tab, G=3), r"sd_spells: a table of 3 rows needs group ids \(group is NULL\)"),
                    (dict(table=tab, ids=bad_group, G=3), "sd_spells: group\\[7\\] = 3 lies outside the 3 groups"),
                    (dict(offsets=np.array([0, 5, 4], dtype=np.int64)), r"sd_spells: offsets decrease at bin 1 \(4 after 5\)"),
                    (dict(offsets=np.array([1, 4, 10], dtype=np.int64)), r"sd_spells: offsets\[0\] = 1, expected 0"),
                    (dict(offsets=np.array([0, 4, 9], dtype=np.int64)), r"sd_spells: offsets\[M\] = 9, expected T = 10")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="sd_spells: offsets decrease at bin 1"):
        ctx.spells_host(x, ">", 0.5, [0, 5, 4, 10], ["count"])
    with pytest.raises(ValueError, match="sd_spells: group\\[7\\] = 3 lies outside the 3 groups"):
        ctx.spells(x, ">", np.zeros((3, 4)), off, ["count"], group=bad_group)
    assert "spells_kernel" not in ctx.prof()  # nothing was launched
    call(table=tab, ids=group, G=3)
    assert ctx.prof()["spells_kernel"]["launches"] == 1
    ctx.prof_enable(False)
    assert np.array_equal(out.to_host(), np.array([[0.0] * 4] * 6))  # 0 > 0 nowhere: no hit, no spell
    # the Python wrapper
    with pytest.raises(ValueError, match=r"where op '!=': expected one of '>', '>=', '<', '<='"):
        ctx.spells(x, "!=", 0.5, off, ["count"])
    with pytest.raises(ValueError, match="spell statistic 'mean': expected one of"):
        ctx.spells(x, ">", 0.5, off, ["mean"])
    with pytest.raises(ValueError, match="sd_spells: nstat = 0"):
        ctx.spells(x, ">", 0.5, off, [])
    with pytest.raises(ValueError, match="sd_spells: min_length = 0"):
        ctx.spells(x, ">", 0.5, off, ["count"], min_length=0)
    with pytest.raises(ValueError, match="threshold: expected a number or a float64 \\[G, 4\\] table"):
        ctx.spells(x, ">", np.zeros((3, 5)), off, ["count"], group=group)
    with pytest.raises(ValueError, match="group: a scalar threshold takes no group ids"):
        ctx.spells(x, ">", 0.5, off, ["count"], group=group)
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape \\(4, 4\\)"):
        ctx.spells(x, ">", 0.5, off, ["count", "valid"], out=ctx.empty((2, 4)))
    with pytest.raises(ValueError, match="out: expected the rows of 2 bins inside the first of 2 planes of 3 rows"):
        ctx.spells(x, ">", 0.5, off, ["count", "valid"], out=ctx.empty((4, 4)).rows(0, 2), plane_rows=3)
    with pytest.raises(ValueError, match="field: expected a float32 or float64"):
        ctx.spells(np.zeros(10), ">", 0.5, off, ["count"])
