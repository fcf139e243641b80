"""GPU: twosample_segment_kernel / quantile_runs_kernel + twosample_select_kernel (csrc/sd_twosample.hip) through Context.twosample /
sd_twosample against tests/_twosample_oracle.py, and the lazy GridArray.compare(...).ks() / .perkins() / .distribution() surface on
host, interp_like and lazy HBM sources.

Every statistic is integer arithmetic on the two sorted series followed by one division, so everything here is compared bit for bit
(np.array_equal with equal_nan): with the oracle, and between layouts, dtype pairs, the two paths, the block sizes of the walk and the
host-buffer twin.  The sizes are the edges of the plan (tests/test_twosample_plan.py): 64 * K rows for the segment widths K = 5, 7, 13, 19 and
16 * 64 * K for the series widths K = 13, 17, 19."""
import numpy as np
import pandas as pd
import pytest

import _twosample_oracle as ts

pytestmark = pytest.mark.gpu

STATS = list(ts.STATS)
PAIRS = [(np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32)]
CELLS = [1, 7, 8, 9, 17]
WIDTH, ORIGIN = 0.5, 0.0625  # histogram edges off the multiples of 1 / 8 (and the score is exact wherever they lie)
SEGMENT_K = {1: 5, 64: 5, 65: 5, 320: 5, 321: 7, 448: 7, 449: 13, 832: 13, 833: 19, 1216: 19}
SERIES_K = {1217: 13, 13313: 17, 17409: 19, 19456: 19}


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def table(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def fields(rng, shape, nan_share=0.05, tied=True):
    """a pair of fields -- in multiples of 1 / 8 (exact in float32 too, heavily tied) or continuous -- with NaN at places of their own"""
    a = rng.normal(size=shape) * 2.0
    b = 0.25 + rng.normal(size=shape) * 2.5
    if tied:
        a, b = np.round(a * 8.0) / 8.0, np.round(b * 8.0) / 8.0
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


def run(ctx, a, b, offsets, stats, layout=None, what="", width=WIDTH, origin=ORIGIN):
    """Context.twosample in a layout (ld and lead of a, of b, of the output, rows between the planes beyond M) -> host [nstat * M, C];
    everything of the output's parent outside the result must stay untouched"""
    T, C = a.shape
    M, n = len(offsets) - 1, len(stats)
    ld_a, lead_a, ld_b, lead_b, ld_out, lead_out, extra = layout or (C, 0, C, 0, C, 0, 0)
    da, db = inside(ctx, a, ld_a, lead_a), inside(ctx, b, ld_b, lead_b)
    plane = M + extra
    parent = ctx.to_device(np.full((n * plane, ld_out), 7.0))
    view = parent if (ld_out, lead_out) == (C, 0) else parent.cells(lead_out, lead_out + C)
    if extra == 0:
        out = ctx.twosample(da, db, offsets, stats, width, origin, out=view)
        assert out is view
    else:
        ctx.twosample(da, db, offsets, stats, width, origin, out=view.rows(0, M), plane_rows=plane)
    back = parent.to_host().reshape(n, plane, ld_out)
    untouched = np.ones(back.shape, dtype=bool)
    untouched[:, :M, lead_out:lead_out + C] = False
    assert (back[untouched] == 7.0).all(), f"{what}: padding written"
    return back[:, :M, lead_out:lead_out + C].reshape(n * M, C).copy()


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} want {want[bad][0]!r}"


def kernels_of(ctx, call):
    """the profiler names of the launches of ``call()``"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        res = call()
        names = sorted(ctx.prof())
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    return res, names


def layouts_of(C):
    even = C + 6 if C % 2 == 0 else C + 5
    odd = C + 5 - C % 2
    # (name, ld and lead of a, of b, of the output, rows between two planes beyond M)
    return [("padded by fours", (C + 8, 4, C + 12, 8, C + 4, 4, 2)), ("padded even", (even + 2, 4, even + 4, 2, even, 2, 2)),
            ("padded odd", (odd, 4, odd + 2, 1, odd - 2, 2, 1)), ("a off by one element", (C + 4, 1, C, 0, C, 0, 0)),
            ("b off by one element", (C, 0, C + 4, 1, C, 0, 0)), ("output off by one double", (C, 0, C, 0, C + 2, 1, 1))]


# ---- the segment path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_max", list(SEGMENT_K))
def test_segment_path(ctx, n_max):
    rng = np.random.default_rng(100 + n_max)
    short = min(n_max, 7)
    lengths = [0, 1, short, n_max, 0]  # an empty first and last bin, a bin of one row, a short one, the longest
    offsets = table(lengths)
    T, M = int(offsets[-1]), len(lengths)
    name = f"twosample_segment_kernel<{SEGMENT_K[n_max]}>"
    for C in CELLS:
        for share in (0.0, 0.05):
            a64, b64 = fields(rng, (T, C), share)
            b64[offsets[3]:offsets[4], 0] = np.nan  # b all NaN in the longest bin of cell 0
            a64[offsets[2]:offsets[3], C - 1] = np.nan  # a all NaN in the short bin of the last cell
            want = ts.twosample(a64, b64, offsets, STATS, WIDTH, ORIGIN)
            for ta, tb in PAIRS:  # (multiples of 1 / 8 are exact in float32: the same expectation)
                what = f"n_max={n_max} C={C} nan={share} {np.dtype(ta).name} {np.dtype(tb).name}"
                got, names = kernels_of(ctx, lambda: run(ctx, a64.astype(ta), b64.astype(tb), offsets, STATS, what=what))
                assert names == [name], names
                same(got, want, what)
            got = got.reshape(4, M, C)
            assert (got[2:, [0, 4]] == 0.0).all() and np.isnan(got[:2, [0, 4]]).all()  # the empty bins
            assert got[3, 3, 0] == 0.0 and np.isnan(got[:2, 3, 0]).all() and got[2, 2, C - 1] == 0.0 and np.isnan(got[:2, 2, C - 1]).all()
        # continuous data, float32 on one side: the expectation of the cast field
        a64, b64 = fields(rng, (T, C), 0.05, tied=False)
        same(run(ctx, a64, b64, offsets, STATS), ts.twosample(a64, b64, offsets, STATS, WIDTH, ORIGIN), f"n_max={n_max} C={C} continuous")
        a32 = a64.astype(np.float32)
        same(run(ctx, a32, b64, offsets, STATS), ts.twosample(a32, b64, offsets, STATS, WIDTH, ORIGIN), f"n_max={n_max} C={C} continuous float32")


@pytest.mark.parametrize("C", [7, 8, 17])
def test_views_give_the_bits_of_the_contiguous_call(ctx, C):
    rng = np.random.default_rng(50 + C)
    offsets = table([0, 1, 40, 330, 9])
    T = int(offsets[-1])
    a64, b64 = fields(rng, (T, C))
    for ta, tb in PAIRS:
        a, b = a64.astype(ta), b64.astype(tb)
        tight = run(ctx, a, b, offsets, STATS)
        same(tight, ts.twosample(a, b, offsets, STATS, WIDTH, ORIGIN), "tight")
        for name, layout in layouts_of(C):
            what = f"C={C} {np.dtype(ta).name} {np.dtype(tb).name} {name}"
            same(run(ctx, a, b, offsets, STATS, layout, what), tight, what)
    # rows of a longer field: the bins of a block of the time axis
    da, db = ctx.to_device(a64), ctx.to_device(b64)
    assert offsets[3] == 41
    part = ctx.twosample(da.rows(41, T), db.rows(41, T), offsets[3:] - 41, STATS, WIDTH, ORIGIN).to_host()
    same(part, ts.twosample(a64[41:], b64[41:], offsets[3:] - 41, STATS, WIDTH, ORIGIN), "rows 41 ..")


def test_each_statistic_alone_and_repeated_codes(ctx):
    rng = np.random.default_rng(4)
    for lengths in ([0, 1, 40, 330, 9], [3, 1300, 0, 50]):  # the segment path and the series path
        offsets = table(lengths)
        M = len(lengths)
        a, b = fields(rng, (int(offsets[-1]), 9))
        want = ts.twosample(a, b, offsets, STATS, WIDTH, ORIGIN)
        same(run(ctx, a, b, offsets, STATS), want, "all four")
        for s, stat in enumerate(STATS):
            same(run(ctx, a, b, offsets, [stat]), want[s * M:(s + 1) * M], f"{stat} alone")
        names = ["perkins", "nb", "ks", "perkins"]  # a repeated code is served
        same(run(ctx, a, b, offsets, names), ts.twosample(a, b, offsets, names, WIDTH, ORIGIN), "repeated codes")
        # the histogram is read only where Perkins is asked for
        same(ctx.twosample(a, b, offsets, ["ks", "na"]).to_host(), np.concatenate([want[:M], want[2 * M:3 * M]]), "no width")
        # other histograms; an origin far off
        for width, origin in ((2.0, 0.0), (0.125, 0.0), (1e-3, -7.0), (100.0, 1e6)):
            same(run(ctx, a, b, offsets, ["perkins"], width=width, origin=origin), ts.twosample(a, b, offsets, "perkins", width, origin),
                 f"width={width} origin={origin}")


def test_constructed_cells(ctx):
    nan, inf = np.nan, np.inf
    for lengths in ([30, 1, 24], [1300, 1, 24]):  # both paths
        offsets = table(lengths)
        T, C = int(offsets[-1]), 8
        rng = np.random.default_rng(9)
        a, b = fields(rng, (T, C), 0.0)
        b[:, 0] = a[:, 0]                                   # 0: the same values
        b[:, 1] = a[:, 1] + 1000.0                          # 1: disjoint supports
        a[3, 2] = a[5, 2] = -inf                            # 2: infinities of both signs in both
        a[7, 2] = b[4, 2] = inf
        b[8, 2] = -inf
        a[:, 3] = 2.5                                       # 3: a constant
        a[0:lengths[0], 4] = nan                            # 4: a all NaN in bin 0
        a[1:lengths[0], 5] = nan                            # 5: one sample of a in bin 0
        a[:, 6], b[:, 6] = 0.0, -0.0                        # 6: zeros of both signs are the same value
        b[::2, 7] = nan                                     # 7: nb about half of na
        for ta, tb in PAIRS:
            what = f"{np.dtype(ta).name} {np.dtype(tb).name} {lengths[0]}"
            x, y = a.astype(ta), b.astype(tb)
            same(run(ctx, x, y, offsets, STATS, what=what), ts.twosample(x, y, offsets, STATS, WIDTH, ORIGIN), what)
        ks, perkins, na, nb = run(ctx, a, b, offsets, STATS).reshape(4, 3, C)
        assert (ks[:, 0] == 0.0).all() and (perkins[:, 0] == 1.0).all() and (ks[:, 1] == 1.0).all() and (perkins[:, 1] == 0.0).all()
        assert np.isnan(ks[0, 4]) and np.isnan(perkins[0, 4]) and na[0, 4] == 0 and nb[0, 4] == lengths[0] and np.isfinite(ks[1:, 4]).all()
        assert na[0, 5] == 1 and 0.0 < ks[0, 5] <= 1.0
        assert (ks[:, 6] == 0.0).all() and (perkins[:, 6] == 1.0).all()
        assert na[0, 7] == lengths[0] and nb[0, 7] == lengths[0] // 2
        # a is b through the same pointer: 0 and 1
        d = ctx.to_device(a)
        twice = ctx.twosample(d, d, offsets, STATS, WIDTH, ORIGIN).to_host().reshape(4, 3, C)
        ok = twice[2] > 0
        assert (twice[0][ok] == 0.0).all() and (twice[1][ok] == 1.0).all() and np.array_equal(twice[2], twice[3])
        assert np.isnan(twice[0][~ok]).all() and not ok[0, 4] and ok.sum() == 3 * C - 1


def test_the_host_twin(ctx):
    rng = np.random.default_rng(6)
    for lengths in ([0, 1, 40, 330, 9], [1300, 20]):
        offsets = table(lengths)
        a64, b64 = fields(rng, (int(offsets[-1]), 9))
        for ta, tb in PAIRS:
            a, b = a64.astype(ta), b64.astype(tb)
            got = ctx.twosample(a, b, offsets, STATS, WIDTH, ORIGIN).to_host()
            same(ctx.twosample_host(a, b, offsets, STATS, WIDTH, ORIGIN), got, "sd_twosample")
            same(ctx.twosample(ctx.to_device(a, ta), ctx.to_device(b, tb), offsets, STATS, WIDTH, ORIGIN).to_host(), got, "resident sources")


# ---- the series path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_max", list(SERIES_K))
def test_series_path(ctx, n_max):
    rng = np.random.default_rng(n_max)
    lengths = [0, 1, 50, n_max]
    offsets = table(lengths)
    T, M = int(offsets[-1]), len(lengths)
    K = SERIES_K[n_max]
    for C in (1, 9):
        for tied in (True, False):
            a, b = fields(rng, (T, C), 0.05, tied)
            b[offsets[3]:, 0] = np.nan if tied else b[offsets[3]:, 0]  # b all NaN in the longest bin of cell 0
            a32 = a.astype(np.float32)
            want = ts.twosample(a32, b, offsets, STATS, WIDTH, ORIGIN)
            got, names = kernels_of(ctx, lambda: run(ctx, a32, b, offsets, STATS, what=f"n_max={n_max} C={C}"))
            assert names == [f"quantile_runs_kernel<{K}>", f"twosample_select_kernel<{K}>"], names
            same(got, want, f"n_max={n_max} C={C} tied={tied}")
            if C == 9:
                name, layout = layouts_of(C)[2]
                same(run(ctx, a32, b, offsets, STATS, layout, name), want, f"n_max={n_max} {name}")
    got = got.reshape(4, M, C)
    assert (got[2:, 0] == 0.0).all() and np.isnan(got[:2, 0]).all()


def test_a_bin_beyond_the_workgroup_merge_is_refused(ctx):
    x = np.zeros((19457, 1))
    with pytest.raises(NotImplementedError, match=r"sd_twosample: a bin of 19457 samples exceeds the workgroup merge \(19456\)"):
        ctx.twosample(x, x, [0, 19457], ["ks"])
    with pytest.raises(NotImplementedError, match="sd_twosample: a bin of 19457 samples"):
        ctx.twosample_host(x, x, [0, 19457], ["ks"])
    assert ctx.twosample(x, x, [0, 1, 19457], ["ks", "na"]).to_host().tolist() == [[0.0], [0.0], [1.0], [19456.0]]


def test_refusals_through_the_c_abi_launch_nothing(ctx):
    from skdownscale_amd._lib import check, ptr

    x = np.arange(40.0).reshape(10, 4)
    a, b, out = ctx.to_device(x), ctx.to_device(x + 1.0), ctx.empty((6, 4))
    off = np.array([0, 4, 10], dtype=np.int64)
    codes = np.array([0, 1, 2, 0], dtype=np.intc)

    def call(ld_a=4, ld_b=4, T=10, C=4, offsets=off, M=2, stats=codes, nstat=3, width=1.0, origin=0.0, ld_out=4, stride=8):
        check(ctx.lib.sd_twosample_dev(ctx.handle, a.vptr, 0, ld_a, b.vptr, 0, ld_b, T, C, ptr(offsets), M, ptr(stats), nstat, width, origin,
                                       out.vptr, ld_out, stride))

    ctx.prof_reset()
    ctx.prof_enable(True)
    for kw, msg in ((dict(stats=np.array([1, 4, 0, 0], dtype=np.intc)), r"sd_twosample: unknown statistic code 4 \(stats\[1\]\)"),
                    (dict(nstat=0), "sd_twosample: nstat = 0, expected 1 to 4 statistics"), (dict(nstat=5), "sd_twosample: nstat = 5"),
                    (dict(width=0.0), "sd_twosample: width = 0, expected a positive finite bin width"),
                    (dict(width=np.nan), "sd_twosample: width = nan"), (dict(origin=np.inf), "sd_twosample: origin = inf, expected a finite number"),
                    (dict(T=0), r"sd_twosample: bad sizes \(T=0, C=4, M=2\)"), (dict(M=0), "sd_twosample: bad sizes"),
                    (dict(ld_a=3), "sd_twosample: ld_a = 3 is less than the 4 cells of a row"),
                    (dict(ld_b=3), "sd_twosample: ld_b = 3 is less than the 4 cells of a row"),
                    (dict(ld_out=3), "sd_twosample: ld_out = 3 is less than the 4 cells of a row"),
                    (dict(stride=7), r"sd_twosample: stride_out = 7 is less than the 8 elements of one statistic \(M \* ld_out\)"),
                    (dict(ld_a=1 << 61), "sd_twosample: field too large"),
                    (dict(ld_a=1 << 29), "sd_twosample: rows of 536870912 and 4 elements exceed the 32-bit row addressing"),
                    (dict(offsets=np.array([0, 5, 4], dtype=np.int64)), r"sd_twosample: offsets decrease at bin 1 \(4 after 5\)"),
                    (dict(offsets=np.array([1, 4, 10], dtype=np.int64)), r"sd_twosample: offsets\[0\] = 1, expected 0"),
                    (dict(offsets=np.array([0, 4, 9], dtype=np.int64)), r"sd_twosample: offsets\[M\] = 9, expected T = 10")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="sd_twosample: offsets decrease at bin 1"):
        ctx.twosample_host(x, x, [0, 5, 4, 10], ["ks"])
    assert not any(k.startswith(("twosample", "quantile")) for k in ctx.prof())  # nothing was launched
    call()
    assert ctx.prof()["twosample_segment_kernel<5>"]["launches"] == 1
    ctx.prof_enable(False)
    same(out.to_host(), ts.twosample(x, x + 1.0, off, ["ks", "perkins", "na"], 1.0), "the raw call")
    # the Python wrapper
    with pytest.raises(ValueError, match="distribution statistic 'mean': expected one of 'ks', 'perkins', 'na', 'nb'"):
        ctx.twosample(x, x, off, ["mean"])
    with pytest.raises(ValueError, match="sd_twosample: nstat = 0"):
        ctx.twosample(x, x, off, [])
    with pytest.raises(ValueError, match="perkins needs the width of the histogram bins"):
        ctx.twosample(x, x, off, ["perkins"])
    with pytest.raises(ValueError, match="width: expected a positive finite number, got -1.0"):
        ctx.twosample(x, x, off, ["perkins"], width=-1.0)
    with pytest.raises(ValueError, match="origin: expected a finite number, got nan"):
        ctx.twosample(x, x, off, ["perkins"], width=1.0, origin=np.nan)
    with pytest.raises(ValueError, match=r"b: expected a \[T, C\] field of shape \(10, 4\) like a, got shape \(10, 5\)"):
        ctx.twosample(x, np.zeros((10, 5)), off, ["ks"])
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape \\(4, 4\\)"):
        ctx.twosample(x, x, off, ["ks", "na"], out=ctx.empty((2, 4)))
    with pytest.raises(ValueError, match="out: expected the rows of 2 bins inside the first of 2 planes of 3 rows"):
        ctx.twosample(x, x, off, ["ks", "na"], out=ctx.empty((4, 4)).rows(0, 2), plane_rows=3)
    with pytest.raises(ValueError, match="twosample_host: expected host arrays"):
        ctx.twosample_host(a, x, off, ["ks"])
    from skdownscale_amd.engine import Context

    other = Context(0)
    with pytest.raises(ValueError, match="sd_twosample: `b` belongs to another context"):
        ctx.twosample(a, other.to_device(x), off, ["ks"])


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2002-12-31", freq="D")  # two years without a leap day
YEARS = np.array([0, 365, 730])
LAT, LON = np.linspace(42.0, 38.0, 10), np.linspace(-110.0, -106.0, 13)
NAMES = ["ks", "perkins", "na", "nb"]


def grid(values, time=TIME):
    from skdownscale_amd import GridArray

    return GridArray(values, ("time", "lat", "lon"), dict(time=time, lat=LAT, lon=LON))


@pytest.fixture(scope="module")
def obs():
    rng = np.random.default_rng(21)
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(len(TIME)) / 365.25)
    v = 285.0 + season[:, None, None] + 4.0 * rng.normal(size=(len(TIME), 10, 13))
    v[rng.random(v.shape) < 0.01] = np.nan
    return grid(v)


@pytest.fixture(scope="module")
def model(obs):
    rng = np.random.default_rng(22)
    v = obs.values + 0.5 + rng.normal(size=obs.shape)
    v[rng.random(v.shape) < 0.01] = np.nan
    v[np.isnan(obs.values) & (rng.random(v.shape) < 0.5)] = 1.0
    return grid(v)


def test_host_against_host_for_every_block_size(ctx, obs, model):
    fa, fb = model.values.reshape(730, 130), obs.values.reshape(730, 130)
    want = ts.twosample(fa, fb, YEARS, NAMES, 1.0, 0.0)
    whole = ts.twosample(fa, fb, [0, 730], NAMES, 1.0, 0.0)
    first = None
    for scratch_bytes in (None, 365 * 130 * 16, 1):  # the whole field, one year and one bin per block
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = model.compare(obs, **kw).resample(time="YS").distribution(NAMES, width=1.0)
        assert not lazy.computed and lazy.shape == (4, 2, 10, 13)
        got = lazy.values
        same(got.reshape(8, 130), want, f"yearly scratch_bytes={scratch_bytes}")
        first = got if first is None else first
        assert np.array_equal(got, first, equal_nan=True)
        same(model.compare(obs, **kw).distribution(NAMES, 1.0).values.reshape(4, 130), whole, f"whole axis scratch_bytes={scratch_bytes}")
    assert np.array_equal(lazy.device_field(ctx).to_host(), want, equal_nan=True)
    # one statistic: the dim is dropped for the whole axis; a selection along the other dims stays lazy
    ks = model.compare(obs).ks()
    assert ks.dims == ("lat", "lon")
    same(ks.values.reshape(1, 130), whole[0:1], "ks alone")
    same(model.compare(obs).perkins(1.0).values.reshape(1, 130), whole[1:2], "perkins alone")
    cut = model.compare(obs).resample(time="YS").perkins(1.0).isel(lat=slice(2, 5))
    assert not cut.computed and np.array_equal(cut.values, first[1][:, 2:5], equal_nan=True)
    # float32 against float64, the other array in another order of dims, time in the middle
    a32 = grid(model.values.astype(np.float32))
    want32 = ts.twosample(a32.values.reshape(730, 130), fb, YEARS, NAMES, 1.0, 0.0)
    same(a32.compare(obs.transpose("lon", "time", "lat"), scratch_bytes=400 * 130 * 12).resample(time="YS").distribution(NAMES, 1.0).values.reshape(8, 130),
         want32, "float32 a")
    mid = model.transpose("lat", "time", "lon").compare(obs).resample(time="YS").ks()
    same(mid.values.transpose(1, 0, 2).reshape(2, 130), want[0:2], "time in the middle")


def test_a_lazy_resample_result_against_a_host_array(ctx, obs, model):
    monthly_obs = np.asarray(obs.resample(time="MS").mean().values)
    monthly_model = np.asarray(model.resample(time="MS").mean().values)
    labels = pd.date_range("2001-01-01", periods=24, freq="MS")
    want = ts.twosample(monthly_model.reshape(24, 130), monthly_obs.reshape(24, 130), [0, 12, 24], NAMES, 2.0, 0.0)
    host = grid(monthly_obs, labels)
    for scratch_bytes in (None, 1):
        lazy = model.resample(time="MS").mean()
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        got = lazy.compare(host, **kw).resample(time="YS").distribution(NAMES, width=2.0)
        same(got.values.reshape(8, 130), want, f"lazy monthly means scratch_bytes={scratch_bytes}")
        assert not lazy.computed  # the monthly means stayed in HBM


def test_an_unchunked_interp_like_against_host(ctx, obs):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(5)
    coarse = GridArray(285.0 + 5.0 * rng.normal(size=(730, 3, 3)), ("time", "lat", "lon"),
                       dict(time=TIME, lat=np.array([42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0])))
    want = ts.twosample(coarse.interp_like(obs).compute().values.reshape(730, 130), obs.values.reshape(730, 130), YEARS, NAMES, 1.0, 0.0)
    for scratch_bytes in (None, 500 * 130 * 16, 1):
        fine = coarse.interp_like(obs)
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = fine.compare(obs, **kw).resample(time="YS").distribution(NAMES, width=1.0)
        same(lazy.values.reshape(8, 130), want, f"interp_like scratch_bytes={scratch_bytes}")
        assert not fine.computed  # the fine field never came to the host
