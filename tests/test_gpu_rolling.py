"""GPU: rolling_kernel (csrc/sd_rolling.hip), staged and unstaged, through Context.rolling and the C ABI against
tests/_rolling_oracle.py, pandas' results in tests/golden/g27_rolling.npz, and the lazy GridArray.rolling surface with its chaining
with interp_like, resample and groupby.

The oracle is the definition of a window's statistic (a loop over its rows in time order), so all four statistics are compared with it
bit for bit, as are the results of different layouts, cells per lane, the two paths and cuts of the time axis: a window is evaluated by
one lane from its own samples only.  Against pandas the bound is the measured one of tests/_rolling_oracle.py."""
import os

import numpy as np
import pandas as pd
import pytest

import _rolling_oracle as ro

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CELLS = [1, 63, 64, 65, 130, 257, 260]
WINDOWS = [1, 2, 8, 9, 31, 120]
SD_ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g27_rolling.npz"))
    return {k: g[k] for k in g.files}


def field(rng, T, C):
    """temperatures with 5 % NaN samples, a run of 40 NaN (longer than most windows) in cell 0 and an all-NaN last cell"""
    x = 285.0 + 10.0 * rng.normal(size=(T, C))
    x[rng.random((T, C)) < 0.05] = np.nan
    x[T // 3:T // 3 + 40, 0] = np.nan
    if C > 2:
        x[:, -1] = np.nan
    return x


def view(ctx, host, ld, lead, fill=7):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart -> (parent, view)"""
    T, C = host.shape
    parent = np.full((T, ld), fill, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    parent = ctx.to_device(parent, host.dtype)
    return parent, (parent.cells(lead, lead + C) if (ld, lead) != (C, 0) else parent)


def untouched(parent, lead, C, fill=7):
    back = parent.to_host()
    return (back[:, :lead] == fill).all() and (back[:, lead + C:] == fill).all()


def layouts_of(C):
    even = C + 6 if C % 2 == 0 else C + 5  # a padded leading dimension that keeps two cells per lane possible
    quad = C + 8 - C % 4 if C % 4 == 0 else even  # ... and four for float32 where C allows
    # (name, source ld, elements in front of a source row, ld and lead of the output)
    return [("tight", C, 0, C, 0), ("padded even", even + 2, 4, even + 4, 2), ("padded by four", quad + 4, 4, quad + 8, 4),
            ("padded odd", C + 5 - C % 2, 4, C + 7 - C % 2, 1), ("output off by one double", C, 0, C + 2, 1)]


def statistics(w):
    """(op, min_periods, ddof) of the sweep: min_periods 0, 1 and w, ddof 0 and 1 where it counts"""
    return [(op, mp, ddof) for op in ro.OPS for mp in sorted({0, 1, w}) for ddof in ((0, 1) if op in ("var", "std") else (1,))]


@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C):
    rng = np.random.default_rng(2700 + C)
    T = 120
    x64 = field(rng, T, C)
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        sources = [view(ctx, host, ld, lead)[1] for _, ld, lead, _, _ in layouts_of(C)]
        outs = [view(ctx, np.full((T, C), 7.0), ld_out, lead_out) for _, _, _, ld_out, lead_out in layouts_of(C)]
        for w in WINDOWS:
            for center in (False, True):
                back = ro.back_of(w, center)
                m = ro.moments(host, w, back)
                for op, mp, ddof in statistics(w):
                    want = ro.finish(m, op, mp, ddof)
                    for (name, *_), src, (_, out) in zip(layouts_of(C), sources, outs):
                        ctx.rolling(src, w, op, back, mp, ddof, out=out)
                        assert np.array_equal(out.to_host(), want, equal_nan=True), \
                            f"C={C} {np.dtype(dtype).name} w={w} center={center} {op} min_periods={mp} ddof={ddof} {name}: differs from the oracle"
                # the one-shot host entry: the same bits
                assert np.array_equal(ctx.rolling_host(host, w, "std", back, 1), ro.finish(m, "std", 1, 1), equal_nan=True)
        for (name, _, _, _, lead_out), (parent, _) in zip(layouts_of(C), outs):
            assert untouched(parent, lead_out, C), f"C={C} {name}: padding of out written"
    if C > 2:  # the all-NaN cell: 0.0 for the sum under min_periods=0, NaN for everything else
        assert (ctx.rolling(x64, 9, "sum", min_periods=0).to_host()[:, -1] == 0.0).all()
        assert np.isnan(ctx.rolling(x64, 9, "mean", min_periods=0).to_host()[:, -1]).all()


@pytest.mark.parametrize("T,w", [(37, 1), (37, 9), (37, 36), (37, 37), (120, 31), (120, 120)])
def test_wrap(ctx, T, w):
    rng = np.random.default_rng(T + w)
    for C, dtype in ((65, np.float64), (130, np.float64), (260, np.float32)):
        x = field(rng, T, C).astype(dtype)
        for center in (False, True):
            back = ro.back_of(w, center)
            m = ro.moments(x, w, back, wrap=True)
            for op, mp, ddof in statistics(w):
                got = ctx.rolling(x, w, op, back, mp, ddof, wrap=True).to_host()
                assert np.array_equal(got, ro.finish(m, op, mp, ddof), equal_nan=True), (C, center, op, mp, ddof)
    # at w = T every row sees every sample once, in its own rotation
    assert (ro.moments(x, T, 0, wrap=True)[1] == (~np.isnan(x)).sum(axis=0)).all()


def test_large_window_takes_the_unstaged_path(ctx):
    rng = np.random.default_rng(331)
    T, w, C = 400, 331, 65
    for dtype in (np.float64, np.float32):
        x = field(rng, T, C).astype(dtype)
        ctx.prof_reset()
        ctx.prof_enable(True)
        got = {(op, center): ctx.rolling(x, w, op, ro.back_of(w, center), 1).to_host() for op in ro.OPS for center in (False, True)}
        names = set(ctx.prof())
        ctx.prof_enable(False)
        assert names == {"rolling_unstaged_kernel"}, names
        for center in (False, True):
            m = ro.moments(x, w, ro.back_of(w, center))
            for op in ro.OPS:
                assert np.array_equal(got[op, center], ro.finish(m, op, 1, 1), equal_nan=True), (dtype, op, center)
    # a window both paths take (60 rows: staged with one cell per lane, not with two): the same bits
    for C in (65, 130):
        x = field(rng, T, C)
        m = ro.moments(x, 60, 30)
        for op in ro.OPS:
            assert np.array_equal(ctx.rolling(x, 60, op, 30, 1).to_host(), ro.finish(m, op, 1, 1), equal_nan=True), (C, op)


@pytest.mark.parametrize("cuts", [[37], [1, 38, 119], list(range(1, 120))], ids=["two", "four", "single rows"])
def test_row_ranges_give_the_bits_of_one_call(ctx, cuts):
    rng = np.random.default_rng(len(cuts))
    for C, dtype in ((65, np.float64), (130, np.float64), (260, np.float32)):
        x = field(rng, 120, C).astype(dtype)
        d = ctx.to_device(x, dtype)
        for w, center, op, wrap in ((9, True, "mean", False), (31, True, "std", False), (31, False, "sum", False), (9, True, "var", True)):
            back = ro.back_of(w, center)
            whole = ctx.rolling(d, w, op, back, 1, wrap=wrap).to_host()
            assert np.array_equal(whole, ro.finish(ro.moments(x, w, back, wrap), op, 1, 1), equal_nan=True)
            out = ctx.to_device(np.full((120, C), 7.0))
            for a, b in zip([0] + cuts, cuts + [120]):
                ctx.rolling(d, w, op, back, 1, wrap=wrap, t0=a, n_out=b - a, out=out.rows(a, b))
            assert np.array_equal(out.to_host(), whole, equal_nan=True), (C, w, op)
            if not wrap:  # a block with its halo rows, asked for its interior only
                for a, b in list(zip([0] + cuts, cuts + [120]))[:4]:
                    b0, b1 = max(0, a - back), min(120, b + w - 1 - back)
                    got = ctx.rolling(d.rows(b0, b1), w, op, back, 1, t0=a - b0, n_out=b - a).to_host()
                    assert np.array_equal(got, whole[a:b], equal_nan=True), (C, w, op, a, b)


def test_inf_follows_ieee(ctx):
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, inf, -inf, 1.0], [5.0, 5.0, nan, 5.0], [inf, -inf, nan, 2.0], [2.0, 1.0, 3.0, 3.0]])
    for op in ro.OPS:
        assert np.array_equal(ctx.rolling(x, 3, op, min_periods=1).to_host(), ro.rolling(x, 3, op, min_periods=1), equal_nan=True)
    assert np.array_equal(ctx.rolling(x, 3, "sum", min_periods=1).to_host()[2], [inf, nan, -inf, 8.0], equal_nan=True)


def test_golden_cases_within_the_pandas_bounds(ctx, golden):
    worst = dict.fromkeys(ro.OPS, 0.0)
    for key, f, w, op, center, mp, ddof, wrap in ro.golden_cases(golden):
        got = ctx.rolling(golden[f], w, op, ro.back_of(w, center), mp, ddof, wrap=wrap).to_host()
        worst[op] = max(worst[op], ro.check(got, golden[key], golden[f], op, f"{key} vs pandas"))
        assert np.array_equal(got, ro.rolling(golden[f], w, op, center, mp, ddof, wrap), equal_nan=True), f"{key}: differs from the oracle"
    print({op: f"{v:.2e} of the scale, allowed {ro.TOLERANCE[op]:.2e}" for op, v in worst.items()})


def test_c_abi_refusals_write_nothing(ctx):
    from skdownscale_amd._lib import ptr

    lib, h = ctx.lib, ctx.handle
    x, out = ctx.to_device(np.ones((10, 4))), ctx.to_device(np.full((10, 4), 7.0))

    def message():
        return lib.sd_last_error().decode()

    def call(op=0, ld=4, T=10, C=4, window=3, back=1, min_periods=1, ddof=1, wrap=0, t0=0, n_out=10, ld_out=4):
        return lib.sd_rolling_dev(h, op, x.vptr, 0, ld, T, C, window, back, min_periods, ddof, wrap, t0, n_out, out.vptr, ld_out)

    assert call() == 0
    out.copy_from_host(np.full((10, 4), 7.0))
    for kw, msg in ((dict(op=4), "unknown op code 4"), (dict(op=-1), "unknown op code -1"), (dict(T=0), "bad sizes (T=0, C=4)"),
                    (dict(C=-1), "bad sizes (T=10, C=-1)"), (dict(window=0, back=0, min_periods=0), "window = 0, expected at least 1"),
                    (dict(back=3), "back = 3 lies outside [0, window = 3)"), (dict(back=-1), "back = -1 lies outside [0, window = 3)"),
                    (dict(min_periods=4), "min_periods = 4 lies outside [0, window = 3]"),
                    (dict(min_periods=-1), "min_periods = -1 lies outside [0, window = 3]"), (dict(ddof=-1), "ddof = -1 is negative"),
                    (dict(t0=-1), "the output rows -1 .. 8 lie outside the 10 rows of the source"),
                    (dict(t0=5, n_out=6), "the output rows 5 .. 10 lie outside the 10 rows of the source"),
                    (dict(n_out=0), "the output rows 0 .. -1 lie outside the 10 rows of the source"),
                    (dict(window=11, back=5, wrap=1), "window = 11 is longer than the 10 rows it wraps around"),
                    (dict(ld=3), "ld = 3 is less than the 4 cells of a row"), (dict(ld_out=3), "ld_out = 3 is less than the 4 cells of a row"),
                    (dict(T=1 << 40, C=1 << 30, ld=1 << 30, ld_out=1 << 30, n_out=1), "field too large"),
                    (dict(T=1 << 40, C=1, ld=1, ld_out=1, window=1, back=0, n_out=1 << 40), "grid too large")):
        assert call(**kw) == SD_ERR_INVALID and message().endswith(f"sd_rolling: {msg}"), (kw, message())
    assert lib.sd_rolling_dev(h, 0, None, 0, 4, 10, 4, 3, 1, 1, 1, 0, 0, 10, out.vptr, 4) == SD_ERR_INVALID
    assert message().endswith("sd_rolling: NULL argument")
    host, res = np.ones((10, 4)), np.full((10, 4), 7.0)
    assert lib.sd_rolling(h, 0, ptr(host), 0, 10, 4, 3, 3, 1, 1, 0, ptr(res)) == SD_ERR_INVALID and (res == 7.0).all()
    assert (out.to_host() == 7.0).all()
    # the engine's words
    with pytest.raises(ValueError, match=r"sd_rolling: min_periods = 4 lies outside \[0, window = 3\]"):
        ctx.rolling(host, 3, min_periods=4)
    with pytest.raises(ValueError, match="sd_rolling: window = 11 is longer than the 10 rows it wraps around"):
        ctx.rolling(host, 11, wrap=True)
    with pytest.raises(NotImplementedError, match="only 'mean', 'sum', 'var', 'std'"):
        ctx.rolling(host, 3, "max")
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape"):
        ctx.rolling(host, 3, out=ctx.empty((9, 4)))
    with pytest.raises(ValueError, match="the output rows 10 .. 9 lie outside the 10 rows"):
        ctx.rolling(host, 3, t0=10)


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(27)
    T = 1096
    time = pd.date_range("2003-01-01", periods=T, freq="D")
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    clat, clon = np.linspace(42.0, 38.0, 4), np.linspace(-110.0, -104.0, 5)
    flat, flon = np.linspace(42.0, 38.0, 9), np.linspace(-110.0, -104.0, 11)
    coarse = GridArray(285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, 4, 5)), ("time", "lat", "lon"), dict(time=time, lat=clat, lon=clon))
    values = 283.0 + season[:, None, None] + 2.0 * rng.normal(size=(T, 9, 11))
    values[rng.random(values.shape) < 0.03] = np.nan
    obs = GridArray(values, ("time", "lat", "lon"), dict(time=time, lat=flat, lon=flon))
    return coarse, obs


def oracle3(values, w, op, center=False, min_periods=None, ddof=1, wrap=False):
    """the oracle along axis 0 of a [T, ...] array"""
    v = np.asarray(values)
    return ro.rolling(v.reshape(v.shape[0], -1), w, op, center, min_periods, ddof, wrap).reshape(v.shape)


def test_host_source_in_blocks(ctx, grids):
    from skdownscale_amd import GridArray

    _, obs = grids
    for dtype in (np.float64, np.float32):
        a = GridArray(obs.values.astype(dtype), obs.dims, obs.coords)
        for w, center, mp, op, ddof in ((9, True, 1, "mean", 1), (31, True, None, "std", 1), (30, False, 3, "sum", 1), (31, True, 2, "var", 0)):
            want = oracle3(a.values, w, op, center, mp, ddof)
            r = a.rolling(time=w, center=center, min_periods=mp)
            lazy = getattr(r, op)(ddof) if op in ("var", "std") else getattr(r, op)()
            assert not lazy.computed and lazy.shape == obs.shape
            assert np.array_equal(lazy.values, want, equal_nan=True) and lazy.computed, (dtype, w, op)
            assert np.array_equal(lazy.device_field(ctx).to_host().reshape(obs.shape), want, equal_nan=True)
            # blocks of 200 and of w + 6 steps (halo included): identical bits
            for rows in (200, w + 6):
                r = a.rolling(time=w, center=center, min_periods=mp, scratch_bytes=rows * 99 * a.values.itemsize)
                blocked = getattr(r, op)(ddof) if op in ("var", "std") else getattr(r, op)()
                assert np.array_equal(blocked.values, want, equal_nan=True), (dtype, w, op, rows)
    with pytest.raises(ValueError, match="scratch_bytes=.*too few for one step and the 15 \\+ 15 steps"):
        obs.rolling(time=31, center=True, scratch_bytes=30 * 99 * 8).mean().values
    with pytest.raises(ValueError, match="wrap=True needs the 1096 steps of dim 'time' in one block: scratch_bytes="):
        obs.rolling(time=31, center=True, wrap=True, scratch_bytes=200 * 99 * 8).mean().values
    # time in the middle of the source, and a sliced lazy result
    swapped = GridArray(obs.values.transpose(1, 0, 2), ("lat", "time", "lon"), obs.coords).rolling(time=9, center=True, min_periods=1).mean()
    want = oracle3(obs.values, 9, "mean", True, 1)
    assert swapped.dims == ("lat", "time", "lon") and np.array_equal(swapped.values.transpose(1, 0, 2), want, equal_nan=True)
    part = obs.rolling(time=9, center=True, min_periods=1).mean().isel(lat=slice(2, 5), lon=slice(1, 8))
    assert not part.computed and np.array_equal(part.values, want[:, 2:5, 1:8], equal_nan=True)


def test_interp_like_then_rolling_stays_resident(ctx, grids):
    coarse, obs = grids
    full = coarse.interp_like(obs).values
    for op, kw in (("mean", dict(time=9, center=True, min_periods=1)), ("std", dict(time=31, center=True))):
        fine = coarse.interp_like(obs)
        lazy = getattr(fine.rolling(**kw), op)()
        got = lazy.values
        assert got.shape == obs.shape and not fine.computed  # the fine daily field never came to the host
        want = oracle3(full, kw["time"], op, True, kw.get("min_periods"))
        assert np.array_equal(got, want, equal_nan=True)
        blocked = getattr(coarse.interp_like(obs).rolling(scratch_bytes=200 * 99 * 8, **kw), op)().values  # six blocks and more
        assert np.array_equal(blocked, want, equal_nan=True)


def test_resample_then_rolling_and_rolling_then_groupby(ctx, grids):
    _, obs = grids
    monthly = obs.resample(time="MS").mean()
    smooth = monthly.rolling(time=3, center=True, min_periods=1).mean()
    got = smooth.values
    assert not monthly.computed and got.shape == (36, 9, 11)  # neither the daily nor the monthly field crossed PCIe
    want = oracle3(obs.resample(time="MS").mean().values, 3, "mean", True, 1)
    assert np.array_equal(got, want, equal_nan=True)
    # rolling -> groupby: the accumulated field is reduced from HBM, whatever the blocks
    acc = obs.rolling(time=5, min_periods=1, scratch_bytes=150 * 99 * 8).sum()
    clim = acc.groupby("time.month").mean()
    got = clim.values
    assert not acc.computed and got.shape == (12, 9, 11)
    rolled = oracle3(obs.values, 5, "sum", False, 1)
    from skdownscale_amd import GridArray

    assert np.array_equal(got, GridArray(rolled, obs.dims, obs.coords).groupby("time.month").mean().values, equal_nan=True)
    # rolling of a lazy anomaly field
    anom = obs.groupby("time.month") - obs.groupby("time.month").mean()
    run = anom.rolling(time=9, center=True, min_periods=1).std()
    got = run.values
    assert not anom.computed
    assert np.array_equal(got, oracle3((obs.groupby("time.month") - obs.groupby("time.month").mean()).values, 9, "std", True, 1), equal_nan=True)


def test_smoothed_climatology_chain(ctx, grids):
    _, obs = grids
    clim = obs.groupby("time.dayofyear").mean()
    smooth = clim.rolling(dayofyear=31, center=True, wrap=True).mean()
    anom = obs.groupby("time.dayofyear") - smooth
    got = anom.values
    assert not clim.computed and not smooth.computed and smooth.dims == ("dayofyear", "lat", "lon") and smooth.shape == (366, 9, 11)
    # the NumPy composition of the oracles
    clim_v = obs.groupby("time.dayofyear").mean().values
    smooth_v = oracle3(clim_v, 31, "mean", True, None, wrap=True)
    doy = obs.coords["time"].dayofyear - 1
    assert np.array_equal(smooth.values, smooth_v, equal_nan=True)
    assert np.array_equal(got, obs.values - smooth_v[doy], equal_nan=True)
    # several blocks of the daily field: the same bits (the 366-row climatology itself must stay whole under wrap)
    blocked = (obs.groupby("time.dayofyear", scratch_bytes=200 * 99 * 8) - clim.rolling(dayofyear=31, center=True, wrap=True).mean()).values
    assert np.array_equal(blocked, got, equal_nan=True)
