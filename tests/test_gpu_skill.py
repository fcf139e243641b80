"""GPU: skill_kernel (csrc/sd_skill.hip) through Context.skill / sd_skill against tests/_skill_oracle.py, and the lazy
GridArray.compare surface on host, interp_like and lazy HBM sources.

Every statistic is one fixed sequence of IEEE operations per cell, so everything here is compared bit for bit (np.array_equal with
equal_nan): with the oracle, and between layouts, cells per lane, the block sizes of the walk and the host-buffer twin.  Only the
comparison with plain NumPy (pairwise sums) has a tolerance: the measured one of the oracle module.

The correlation of a series with itself is qaa / (sqrt(qaa) * sqrt(qaa)): exactly 1 where the product of the two roots rounds back to
qaa, else the double below 1 (the quotient is at least 1 - 4 * 2^-53; above 1 it is clamped).  Where a test asks for exactly 1 or -1 its
series are built so that qaa has an exact root (sixteen deviations of +-2^k around an exact mean); on plain data the bound is asserted."""
import numpy as np
import pandas as pd
import pytest

import _skill_oracle as sk

pytestmark = pytest.mark.gpu

GROUP = 8  # bins of a workgroup (sdbn::kBinsPerGroup, pinned by tests/test_skill_plan.py); 8 rows are in flight per batch
# T = 97: an empty first, middle and last bin; lengths 1, 7, 8, 9, 16, 17 (one row, a partial, a whole, a whole + partial batch, two
# whole, two whole + one row) and 31; M = 11 is more than one workgroup's run of bins
LENGTHS = [0, 1, 7, 8, 9, 16, 17, 0, 31, 8, 0]
CELLS = [1, 2, 63, 64, 65, 130, 256, 260]
PAIRS = [(np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32)]
STATS = list(sk.STATS)
ONE_PASS = ["count", "bias", "ratio", "mae", "rmse"]


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def table(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


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


def run(ctx, a, b, offsets, stats, layout=None, what=""):
    """Context.skill in a layout (ld and lead of a, of b, of the output, rows between the planes beyond M) -> host [nstat * M, C];
    everything of the output's parent outside the result must stay untouched"""
    T, C = a.shape
    M, n = len(offsets) - 1, len(stats)
    ld_a, lead_a, ld_b, lead_b, ld_out, lead_out, extra = layout or (C, 0, C, 0, C, 0, 0)
    da, db = inside(ctx, a, ld_a, lead_a), inside(ctx, b, ld_b, lead_b)
    plane = M + extra
    parent = ctx.to_device(np.full((n * plane, ld_out), 7.0))
    view = parent if (ld_out, lead_out) == (C, 0) else parent.cells(lead_out, lead_out + C)
    if extra == 0:
        out = ctx.skill(da, db, offsets, stats, out=view)
        assert out is view
    else:
        ctx.skill(da, db, offsets, stats, out=view.rows(0, M), plane_rows=plane)
    back = parent.to_host().reshape(n, plane, ld_out)
    untouched = np.ones(back.shape, dtype=bool)
    untouched[:, :M, lead_out:lead_out + C] = False
    assert (back[untouched] == 7.0).all(), f"{what}: padding written"
    return back[:, :M, lead_out:lead_out + C].reshape(n * M, C).copy()


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} want {want[bad][0]!r}"


@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C):
    rng = np.random.default_rng(3000 + C)
    offsets = table(LENGTHS)
    T, M = int(offsets[-1]), len(LENGTHS)
    assert T == 97 and M == GROUP + 3
    a64, b64 = fields(rng, (T, C))
    long = int(np.flatnonzero(np.diff(offsets) == 31)[0])
    a64[offsets[long]:offsets[long + 1], 0] = np.nan  # a bin without a valid pair in cell 0
    for ta, tb in PAIRS:
        a, b = a64.astype(ta), b64.astype(tb)
        what = f"C={C} {np.dtype(ta).name} {np.dtype(tb).name}"
        want = sk.skill(a, b, offsets, STATS)
        got = run(ctx, a, b, offsets, STATS, what=what)
        same(got, want, what)
        # one by one: the same rows as in the call for all seven
        for s, stat in enumerate(STATS):
            same(run(ctx, a, b, offsets, [stat]), want[s * M:(s + 1) * M], f"{what} {stat} alone")
    got = got.reshape(len(STATS), M, C)
    empty = np.diff(offsets) == 0
    assert (got[0][empty] == 0.0).all() and np.isnan(got[1:][:, empty]).all()  # empty bins
    assert got[0, long, 0] == 0.0 and np.isnan(got[1:, long, 0]).all()  # the all-invalid bin
    one = np.diff(offsets) == 1
    full = ~np.isnan(a64[offsets[:-1][one]]) & ~np.isnan(b64[offsets[:-1][one]])  # a bin of one row: one pair where both are there
    assert np.isnan(got[5:][:, one][:, full]).all() and np.isfinite(got[4][one][full]).all() and (got[0][one][full] == 1.0).all()


@pytest.mark.parametrize("lengths", [[120], [60, 60], [17] * (GROUP - 1), [5] * GROUP, [13] * (GROUP + 1), [3, 0] * GROUP + [3]],
                         ids=["M=1", "M=2", "M=7", "M=8", "M=9", "M=17"])
def test_bin_counts_at_the_edges_of_a_workgroup(ctx, lengths):
    rng = np.random.default_rng(len(lengths))
    offsets = table(lengths)
    T = int(offsets[-1])
    for C in (65, 130):
        a, b = fields(rng, (T, C))
        got = ctx.skill(a, b, offsets, STATS)
        assert got.shape == (len(STATS) * len(lengths), C)
        same(got.to_host(), sk.skill(a, b, offsets, STATS), f"M={len(lengths)} C={C}")


def exact_series(n, k=0):
    """n >= 16 values around 3 with sixteen deviations of +-2^k and zeros elsewhere: the mean is exactly 3 and qaa = 16 * 4^k has an
    exact root"""
    dev = np.zeros(n)
    dev[:16] = np.resize([1.0, -1.0], 16) * 2.0 ** k
    return 3.0 + dev


def test_constructed_cells(ctx):
    nan, inf = np.nan, np.inf
    lengths = [20, 17, 1, 24]
    offsets = table(lengths)
    T, C = int(offsets[-1]), 12
    rng = np.random.default_rng(9)
    a, b = fields(rng, (T, C), 0.0)
    a[3, 0] = a[25, 0] = nan                       # 0: NaN only in a
    b[5, 1] = b[40, 1] = nan                       # 1: NaN only in b
    a[7, 2] = b[7, 2] = a[8, 2] = b[9, 2] = nan    # 2: NaN in both, at the same step and at neighbouring ones
    a[20:37, 3] = nan                              # 3: bin 1 without a valid pair (a all NaN), its neighbours whole
    a[0:19, 4] = nan                               # 4: bin 0 with one valid pair, its last row
    a[:, 5] = 2.5                                  # 5: a constant
    for m in range(4):                             # 6: a == b is asked for below through the same pointer; here b = -a
        n = lengths[m]
        a[offsets[m]:offsets[m + 1], 6] = exact_series(n, m) if n >= 16 else 3.0
    b[:, 6] = -a[:, 6]
    a[30, 7] = inf                                 # 7: an inf sample in a
    b[50, 8] = -inf                                # 8: one in b
    a[45, 9] = b[45, 9] = inf                      # 9: inf in both at the same step: inf - inf
    a[:, 10], b[:, 10] = 0.0, 0.0                  # 10: a dry record: the ratio is 0 / 0
    b[:, 11] = a[:, 11] + 0.5                      # 11: a constant offset
    for ta, tb in PAIRS:
        what = f"{np.dtype(ta).name} {np.dtype(tb).name}"
        x, y = a.astype(ta), b.astype(tb)
        same(run(ctx, x, y, offsets, STATS, what=what), sk.skill(x, y, offsets, STATS), what)
    got = run(ctx, a, b, offsets, STATS).reshape(7, 4, C)
    count, bias, ratio, mae, rmse, corr, std_ratio = got
    assert list(count[:, 0]) == [19, 16, 1, 24] and list(count[:, 1]) == [19, 17, 1, 23] and list(count[:, 2]) == [17, 17, 1, 24]
    assert count[1, 3] == 0 and np.isnan(got[1:, 1, 3]).all() and list(count[[0, 2, 3], 3]) == [20, 1, 24]
    assert count[0, 4] == 1 and np.isnan(corr[0, 4]) and np.isnan(std_ratio[0, 4]) and np.isfinite(rmse[0, 4]) and rmse[0, 4] == abs(a[19, 4] - b[19, 4])
    assert np.isnan(corr[[0, 1, 3], 5]).all() and (std_ratio[[0, 1, 3], 5] == 0.0).all()  # a constant: no correlation, no spread
    assert np.isnan(corr[2]).all() and np.isnan(std_ratio[2]).all() and np.isfinite(rmse[2]).all()  # the bin of one row, every cell
    assert (corr[[0, 1, 3], 6] == -1.0).all() and (ratio[:, 6] == -1.0).all() and (std_ratio[[0, 1, 3], 6] == 1.0).all()
    assert bias[1, 7] == inf and rmse[1, 7] == inf and np.isnan(corr[1, 7]) and np.isfinite(got[1:, [0, 3], 7]).all()
    assert bias[3, 8] == inf and mae[3, 8] == inf and np.isnan(corr[3, 8])
    assert np.isnan(bias[3, 9]) and np.isnan(rmse[3, 9]) and count[3, 9] == 24  # inf - inf is NaN, the pair is valid
    assert np.isnan(ratio[:, 10]).all() and (bias[:, 10] == 0.0).all() and np.isnan(corr[:, 10]).all()
    assert (bias[:, 11] == -0.5).all() and (mae[:, 11] == 0.5).all() and (rmse[:, 11] == 0.5).all()
    # a == b through the same pointer: bias 0 and, on the series with an exact root, corr exactly 1
    d = ctx.to_device(a)
    twice = ctx.skill(d, d, offsets, ["bias", "mae", "corr", "std_ratio", "ratio"]).to_host().reshape(5, 4, C)
    same(twice.reshape(20, C), sk.skill(a, a, offsets, ["bias", "mae", "corr", "std_ratio", "ratio"]), "the same pointer")
    ok = count > 0
    ok[:, [7, 9]] = False  # (inf - inf)
    assert (twice[0][ok] == 0.0).all() and (twice[1][ok] == 0.0).all()
    assert (twice[2][[0, 1, 3], 6] == 1.0).all() and (twice[3][[0, 1, 3], 6] == 1.0).all()
    plain = twice[2][[0, 1, 3]][:, [1, 2, 8, 11]]  # plain series: 1 or the double below it
    assert ((plain >= 1.0 - 5 * 2.0 ** -53) & (plain <= 1.0)).all()


def test_one_pass_and_two_pass_calls_and_repeated_codes(ctx):
    rng = np.random.default_rng(4)
    offsets = table(LENGTHS)
    for C in (63, 130, 260):
        a64, b64 = fields(rng, (97, C))
        for ta, tb in PAIRS:
            a, b = a64.astype(ta), b64.astype(tb)
            M = len(LENGTHS)
            one = run(ctx, a, b, offsets, ONE_PASS)
            two = run(ctx, a, b, offsets, ONE_PASS + ["corr"])
            same(two[:5 * M], one, "the shared statistics of a two-pass call")
            same(one, sk.skill(a, b, offsets, ONE_PASS), "one pass")
            names = ["corr", "bias", "corr", "count", "bias", "std_ratio", "corr"]  # a repeated code is served
            rep = run(ctx, a, b, offsets, names)
            same(rep, sk.skill(a, b, offsets, names), "repeated codes")
            same(rep[0:M], rep[2 * M:3 * M], "the same code twice")
            same(run(ctx, a, b, offsets, ["rmse"] * 7), np.concatenate([one[4 * M:5 * M]] * 7), "seven times rmse")


@pytest.mark.parametrize("C", [63, 130, 260])
def test_views_give_the_bits_of_the_contiguous_call(ctx, C):
    rng = np.random.default_rng(50 + C)
    offsets = table(LENGTHS)
    a64, b64 = fields(rng, (97, C))
    even = C + 6 if C % 2 == 0 else C + 5
    odd = C + 5 - C % 2
    # (name, ld and lead of a, of b, of the output, rows between two planes beyond M)
    layouts = [("padded by fours", (C + 8, 4, C + 12, 8, C + 4, 4, 2)), ("padded even", (even + 2, 4, even + 4, 2, even, 2, 2)),
               ("padded odd", (odd, 4, odd + 2, 1, odd - 2, 2, 1)), ("a off by one element", (C + 4, 1, C, 0, C, 0, 0)),
               ("b off by one element", (C, 0, C + 4, 1, C, 0, 0)), ("output off by one double", (C, 0, C, 0, C + 2, 1, 1))]
    for ta, tb in PAIRS:
        a, b = a64.astype(ta), b64.astype(tb)
        tight = run(ctx, a, b, offsets, STATS)
        same(tight, sk.skill(a, b, offsets, STATS), "tight")
        for name, layout in layouts:
            what = f"C={C} {np.dtype(ta).name} {np.dtype(tb).name} {name}"
            same(run(ctx, a, b, offsets, STATS, layout, what), tight, what)
    # rows of a longer field: the bins of a block of the time axis
    da, db = ctx.to_device(a64), ctx.to_device(b64)
    assert offsets[4] == 16
    part = ctx.skill(da.rows(16, 97), db.rows(16, 97), offsets[4:] - 16, STATS).to_host()
    same(part, sk.skill(a64[16:], b64[16:], offsets[4:] - 16, STATS), "rows 16 ..")


def test_the_host_twin(ctx):
    rng = np.random.default_rng(6)
    offsets = table(LENGTHS)
    for C in (63, 130, 260):
        a64, b64 = fields(rng, (97, C))
        for ta, tb in PAIRS:
            a, b = a64.astype(ta), b64.astype(tb)
            got = ctx.skill(a, b, offsets, STATS).to_host()
            same(ctx.skill_host(a, b, offsets, STATS), got, "sd_skill")
            same(ctx.skill(ctx.to_device(a, ta), ctx.to_device(b, tb), offsets, STATS).to_host(), got, "resident sources")
            same(ctx.skill(a.astype(np.float64), b.astype(np.float64), offsets, STATS).to_host(), got, "the widened sources")


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2002-12-31", freq="D")  # two years without a leap day
YEARS = np.array([0, 365, 730])
MONTHS = np.concatenate([[0], np.cumsum(TIME.to_series().groupby([TIME.year, TIME.month]).size().to_numpy())])
LAT, LON = np.linspace(42.0, 38.0, 10), np.linspace(-110.0, -106.0, 13)
NAMES = ["bias", "rmse", "corr", "count", "std_ratio"]


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
    v[np.isnan(obs.values) & (rng.random(v.shape) < 0.5)] = 1.0  # (NaN only in the observations at some steps)
    return grid(v)


def test_host_against_host_for_every_block_size(ctx, obs, model):
    fa, fb = model.values.reshape(730, 130), obs.values.reshape(730, 130)
    want = sk.skill(fa, fb, YEARS, NAMES)
    whole = sk.skill(fa, fb, [0, 730], NAMES)
    first = None
    for scratch_bytes in (None, 730 * 130 * 16, 365 * 130 * 16, 365 * 130 * 16 - 1, 1):  # the whole field down to one bin per block
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = model.compare(obs, **kw).resample(time="YS").indices(NAMES)
        assert not lazy.computed and lazy.shape == (5, 2, 10, 13)
        got = lazy.values
        same(got.reshape(10, 130), want, f"yearly scratch_bytes={scratch_bytes}")
        first = got if first is None else first
        assert np.array_equal(got, first, equal_nan=True)
        same(model.compare(obs, **kw).indices(NAMES).values.reshape(5, 130), whole, f"whole axis scratch_bytes={scratch_bytes}")
    assert np.array_equal(lazy.device_field(ctx).to_host(), want, equal_nan=True)
    # one statistic: the dim is dropped for the whole axis; a selection along the other dims stays lazy
    rmse = model.compare(obs).rmse()
    assert rmse.dims == ("lat", "lon")
    same(rmse.values.reshape(1, 130), whole[1:2], "rmse alone")
    cut = model.compare(obs).resample(time="YS").corr().isel(lat=slice(2, 5))
    assert not cut.computed and np.array_equal(cut.values, first[2][:, 2:5], equal_nan=True)
    # float32 against float64, the other array in another order of dims, time in the middle
    a32 = grid(model.values.astype(np.float32))
    want32 = sk.skill(a32.values.reshape(730, 130), fb, YEARS, NAMES)
    for scratch_bytes in (None, 400 * 130 * 12):
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        same(a32.compare(obs.transpose("lon", "time", "lat"), **kw).resample(time="YS").indices(NAMES).values.reshape(10, 130), want32, "float32 a")
    mid = model.transpose("lat", "time", "lon").compare(obs).resample(time="YS").rmse()
    same(mid.values.transpose(1, 0, 2).reshape(2, 130), want[2:4], "time in the middle")
    # precipitation's relative bias
    wet_a, wet_b = grid(np.maximum(model.values - 290.0, 0.0)), grid(np.maximum(obs.values - 290.0, 0.0))
    same(wet_a.compare(wet_b).ratio().values.reshape(1, 130), sk.skill(wet_a.values.reshape(730, 130), wet_b.values.reshape(730, 130), [0, 730], "ratio"), "ratio")


def test_a_lazy_resample_result_against_a_host_array(ctx, obs, model):
    monthly_obs = np.asarray(obs.resample(time="MS").mean().values)
    monthly_model = np.asarray(model.resample(time="MS").mean().values)
    labels = pd.date_range("2001-01-01", periods=24, freq="MS")
    want = sk.skill(monthly_model.reshape(24, 130), monthly_obs.reshape(24, 130), [0, 12, 24], NAMES)
    host = grid(monthly_obs, labels)
    for scratch_bytes in (None, 1):
        lazy = model.resample(time="MS").mean()
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        got = lazy.compare(host, **kw).resample(time="YS").indices(NAMES)
        same(got.values.reshape(10, 130), want, f"lazy monthly means scratch_bytes={scratch_bytes}")
        assert not lazy.computed  # the monthly means stayed in HBM
    lazy = obs.resample(time="MS").mean()
    flipped = grid(monthly_model, labels).compare(lazy).resample(time="YS").indices(NAMES)
    same(flipped.values.reshape(10, 130), want, "the lazy array as the other")
    assert not lazy.computed


def test_a_disaggregated_field_against_the_observations_it_borrowed_from(ctx):
    """years='same': every month borrows its own daily pattern; where the monthly target is the observations' own mean the shift is
    zero and the days are the observations bit for bit, so the bias is 0.  The observations are built from ``exact_series`` (a mean
    and a sum of squared deviations without rounding), so the correlation is exactly 1 there, shifted months included."""
    rng = np.random.default_rng(8)
    v = np.empty((730, 10, 13))
    amp = 2.0 ** rng.integers(-2, 3, size=(10, 13))
    base = rng.integers(270, 300, size=(10, 13)).astype(np.float64)
    for m in range(24):
        n = MONTHS[m + 1] - MONTHS[m]
        v[MONTHS[m]:MONTHS[m + 1]] = base + (exact_series(n) - 3.0)[rng.permutation(n)][:, None, None] * amp
    o = grid(v)
    labels = pd.date_range("2001-01-01", periods=24, freq="MS")
    target = np.asarray(o.resample(time="MS").mean().values).copy()
    assert np.array_equal(target, np.broadcast_to(base, (24, 10, 13)))
    shifted = np.zeros(24, dtype=bool)
    shifted[[2, 7, 13, 23]] = True
    target[shifted] += 1.5
    names = ["bias", "corr", "rmse", "count"]
    first = None
    for scratch_bytes in (None, 1):
        daily = grid(target, labels).disaggregate(o, years="same")
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = daily.compare(o, **kw).resample(time="MS").indices(names)
        got = lazy.values
        assert not daily.computed  # taken whole from HBM
        first = got if first is None else first
        assert np.array_equal(got, first, equal_nan=True)
    bias, corr, rmse, count = first
    assert (bias[~shifted] == 0.0).all() and (rmse[~shifted] == 0.0).all() and (corr[~shifted] == 1.0).all()
    assert (bias[shifted] == 1.5).all() and (corr[shifted] == 1.0).all() and (count == np.diff(MONTHS)[:, None, None]).all()
    same(first.reshape(4 * 24, 130), sk.skill(grid(target, labels).disaggregate(o, years="same").values.reshape(730, 130), v.reshape(730, 130), MONTHS, names),
         "disaggregated")


def test_an_unchunked_interp_like_against_host(ctx, obs):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(5)
    coarse = GridArray(285.0 + 5.0 * rng.normal(size=(730, 3, 3)), ("time", "lat", "lon"),
                       dict(time=TIME, lat=np.array([42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0])))
    want = sk.skill(coarse.interp_like(obs).compute().values.reshape(730, 130), obs.values.reshape(730, 130), YEARS, NAMES)
    for scratch_bytes in (None, 500 * 130 * 16, 1):
        fine = coarse.interp_like(obs)
        kw = {} if scratch_bytes is None else dict(scratch_bytes=scratch_bytes)
        lazy = fine.compare(obs, **kw).resample(time="YS").indices(NAMES)
        same(lazy.values.reshape(10, 130), want, f"interp_like scratch_bytes={scratch_bytes}")
        assert not fine.computed  # the fine field never came to the host


def test_against_numpy_on_the_field_of_the_oracle(ctx):
    a, b = sk.field()
    for offsets in (np.array([0, sk.T]), sk.BINS):
        M = len(offsets) - 1
        got = ctx.skill(a, b, offsets, STATS).to_host()
        same(got, sk.skill(a, b, offsets, STATS), "the oracle")
        got, want = got.reshape(7, M, 6), sk.numpy_skill(a, b, offsets).reshape(7, M, 6)
        for i, s in enumerate(STATS):
            print(f"{s:10s} M={M:2d} {sk.distance(got[i], want[i], a, b, s):.3e} of the scale (allowed {sk.TOLERANCE[s]:.3e})")
            sk.check(got[i], want[i], a, b, s, f"{s} M={M}")


def test_refusals_through_the_c_abi_launch_nothing(ctx):
    from skdownscale_amd._lib import check, ptr

    x = np.zeros((10, 4))
    a, b, out = ctx.to_device(x), ctx.to_device(x + 1.0), ctx.empty((6, 4))
    off = np.array([0, 4, 10], dtype=np.int64)
    codes = np.array([1, 4, 0, 0, 0, 0, 0], dtype=np.intc)

    def call(ld_a=4, ld_b=4, T=10, C=4, offsets=off, M=2, stats=codes, nstat=3, ld_out=4, stride=8):
        check(ctx.lib.sd_skill_dev(ctx.handle, a.vptr, 0, ld_a, b.vptr, 0, ld_b, T, C, ptr(offsets), M, ptr(stats), nstat, out.vptr, ld_out, stride))

    ctx.prof_reset()
    ctx.prof_enable(True)
    for kw, msg in ((dict(stats=np.array([1, 7, 0, 0, 0, 0, 0], dtype=np.intc)), r"sd_skill: unknown statistic code 7 \(stats\[1\]\)"),
                    (dict(nstat=0), "sd_skill: nstat = 0, expected 1 to 7 statistics"), (dict(nstat=8), "sd_skill: nstat = 8"),
                    (dict(T=0), r"sd_skill: bad sizes \(T=0, C=4, M=2\)"), (dict(M=0), "sd_skill: bad sizes"), (dict(C=-1), "sd_skill: bad sizes"),
                    (dict(ld_a=3), "sd_skill: ld_a = 3 is less than the 4 cells of a row"),
                    (dict(ld_b=3), "sd_skill: ld_b = 3 is less than the 4 cells of a row"),
                    (dict(ld_out=3), "sd_skill: ld_out = 3 is less than the 4 cells of a row"),
                    (dict(stride=7), r"sd_skill: stride_out = 7 is less than the 8 elements of one statistic \(M \* ld_out\)"),
                    (dict(ld_a=1 << 61), "sd_skill: field too large"),
                    (dict(offsets=np.array([0, 5, 4], dtype=np.int64)), r"sd_skill: offsets decrease at bin 1 \(4 after 5\)"),
                    (dict(offsets=np.array([1, 4, 10], dtype=np.int64)), r"sd_skill: offsets\[0\] = 1, expected 0"),
                    (dict(offsets=np.array([0, 4, 9], dtype=np.int64)), r"sd_skill: offsets\[M\] = 9, expected T = 10")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="sd_skill: offsets decrease at bin 1"):
        ctx.skill_host(x, x, [0, 5, 4, 10], ["bias"])
    with pytest.raises(ValueError, match=r"sd_skill: offsets\[M\] = 9, expected T = 10"):
        ctx.skill(x, x, [0, 9], ["bias"])
    assert "skill_kernel" not in ctx.prof()  # nothing was launched
    call()
    assert ctx.prof()["skill_kernel"]["launches"] == 1
    ctx.prof_enable(False)
    assert np.array_equal(out.to_host(), np.array([[-1.0] * 4] * 2 + [[1.0] * 4] * 2 + [[4.0] * 4, [6.0] * 4]))  # bias, rmse, count
    # the Python wrapper
    with pytest.raises(ValueError, match="skill statistic 'mean': expected one of 'count', 'bias', 'ratio', 'mae', 'rmse', 'corr', 'std_ratio'"):
        ctx.skill(x, x, off, ["mean"])
    with pytest.raises(ValueError, match="sd_skill: nstat = 0"):
        ctx.skill(x, x, off, [])
    with pytest.raises(ValueError, match="sd_skill: nstat = 8"):
        ctx.skill(x, x, off, ["bias"] * 8)
    with pytest.raises(ValueError, match=r"b: expected a \[T, C\] field of shape \(10, 4\) like a, got shape \(10, 5\)"):
        ctx.skill(x, np.zeros((10, 5)), off, ["bias"])
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape \\(4, 4\\)"):
        ctx.skill(x, x, off, ["bias", "count"], out=ctx.empty((2, 4)))
    with pytest.raises(ValueError, match="out: expected the rows of 2 bins inside the first of 2 planes of 3 rows"):
        ctx.skill(x, x, off, ["bias", "count"], out=ctx.empty((4, 4)).rows(0, 2), plane_rows=3)
    with pytest.raises(ValueError, match="a: expected a float32 or float64"):
        ctx.skill(np.zeros(10), np.zeros(10), off, ["bias"])
    with pytest.raises(ValueError, match="skill_host: expected host arrays"):
        ctx.skill_host(a, x, off, ["bias"])
    from skdownscale_amd.engine import Context

    other = Context(0)
    with pytest.raises(ValueError, match="sd_skill: `b` belongs to another context"):
        ctx.skill(a, other.to_device(x), off, ["bias"])
