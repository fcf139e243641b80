"""GPU: quantile_segment_kernel, quantile_runs_kernel and quantile_select_kernel (csrc/sd_quantile.hip) through Context.quantile, the C
ABI and the lazy GridArray.quantile / .median surface, against tests/_quantile_oracle.py.

The oracle is the definition (np.nanquantile / np.nanmedian restated as single IEEE operations; tests/test_quantile_host.py holds it
against NumPy bit for bit) and the library is built without contraction, so every comparison is bit equality (``==``: the sign of a zero
is not pinned; NaN where NaN).  A sort does not care about the order of its samples, so the results of every layout, path and entry
point are the same bits too."""
import numpy as np
import pandas as pd
import pytest

import _quantile_oracle as qo

pytestmark = pytest.mark.gpu

# T = 300, G = 12: 1, 2, 3 rows; 7, 8, 9; 31, 63, 64, 65 (one wave's worth and one more); all served by the narrowest width
SIZES = [1, 2, 3, 7, 8, 9, 31, 63, 64, 65, 16, 31]
CELLS = [1, 7, 8, 9, 17, 130]
QS = [0.0, 1.0 / 3.0, 0.5, 0.95, 1.0]
METHODS = qo.METHODS + ("median",)
SEG_WIDTHS, SERIES_WIDTHS = (5, 13, 21), (13, 17, 19)
SD_ERR_INVALID, SD_ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def scattered(rng, sizes):
    """ids with these group sizes, scattered by a seeded permutation"""
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def field(rng, group, C):
    """temperatures with 5 % NaN samples; in cell 0 an all-NaN group (the one of 65 rows); in the last cell NaN in 9 consecutive rows of
    the group of 64; cell C // 2 is tie-heavy (30 % exact zeros, the rest from a few values)"""
    T = len(group)
    x = 285.0 + 10.0 * rng.normal(size=(T, C))
    x[:, C // 2] = np.where(rng.random(T) < 0.3, 0.0, rng.integers(1, 6, size=T) * 0.25)
    x[rng.random((T, C)) < 0.05] = np.nan
    sizes = np.bincount(group)
    x[np.flatnonzero(group == int(np.argmax(sizes))), 0] = np.nan
    rows = np.flatnonzero(group == int(np.flatnonzero(sizes == 64)[0])) if (sizes == 64).any() else np.arange(T)
    x[rows[3:12], -1] = np.nan
    return x


def view(ctx, host, ld, lead, fill=7):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart -> (parent, view)"""
    T, C = host.shape
    parent = np.full((T, ld), fill, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    parent = ctx.to_device(parent, host.dtype)
    return parent, (parent.cells(lead, lead + C) if (ld, lead) != (C, 0) else parent)


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


@pytest.mark.parametrize("C", CELLS)
def test_segment_path_shape_sweep(ctx, C):
    rng = np.random.default_rng(3000 + C)
    group = scattered(rng, SIZES)
    T, G = len(group), len(SIZES)
    assert T == 300 and G == 12
    for g in np.flatnonzero(np.asarray(SIZES) > 1):
        rows = np.flatnonzero(group == g)
        assert rows[-1] - rows[0] > len(rows) - 1, f"group {g} is a run"
    x64 = field(rng, group, C)
    assert np.isnan(x64[group == 9, 0]).all() and 0.02 < np.isnan(x64).mean() < 0.35
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        sorted_ = qo.sorted_groups(host, group, G)
        dev = ctx.to_device(host, dtype)
        for method in METHODS:
            for skipna in (True, False):
                want = qo.quantile_sorted(sorted_, QS, method, skipna)
                got, names = kernels_of(ctx, lambda: ctx.quantile(dev, QS, group, G, method, skipna))
                assert names == ["quantile_segment_kernel<5>"], names
                assert qo.same(got.to_host(), want), f"C={C} {np.dtype(dtype).name} {method} skipna={skipna}: differs from the oracle"
                Q = 1 if method == "median" else len(QS)
                assert np.isnan(want[9::G, 0]).all() and want.shape == (Q * G, C)
                if not skipna:
                    assert np.isnan(want[8::G, -1]).all()  # the 9 NaN rows of the group of 64
        dev.free()


def test_a_group_without_a_row_and_one_group(ctx):
    rng = np.random.default_rng(11)
    x = rng.normal(size=(40, 9))
    group = (np.arange(40) % 3 * 2).astype(np.int32)  # ids 0, 2, 4 of G = 6
    got = ctx.quantile(x, [0.25, 0.5], group, 6).to_host()
    assert qo.same(got, qo.quantile_field(x, [0.25, 0.5], group, 6)) and np.isnan(got[[1, 3, 5, 7, 9, 11]]).all() and not np.isnan(got[0::2]).any()
    # group=None: one group, whatever G says
    assert qo.same(ctx.quantile(x, 0.9).to_host(), np.nanquantile(x, 0.9, axis=0)[None])
    assert qo.same(ctx.quantile(x, 0.9, method="median").to_host(), np.median(x, axis=0)[None])
    assert qo.same(ctx.quantile(x[:1], [0.0, 0.3, 1.0]).to_host(), np.repeat(x[:1], 3, axis=0))  # one sample is every quantile


@pytest.mark.parametrize("K", SEG_WIDTHS)
def test_segment_width_boundaries(ctx, K):
    C = 9
    wider = [w for w in SEG_WIDTHS if w > K]
    for n, names in ((64 * K - 1, [f"quantile_segment_kernel<{K}>"]), (64 * K, [f"quantile_segment_kernel<{K}>"]),
                     (64 * K + 1, [f"quantile_segment_kernel<{wider[0]}>"] if wider else
                      [f"quantile_runs_kernel<{SERIES_WIDTHS[0]}>", f"quantile_select_kernel<{SERIES_WIDTHS[0]}>"])):
        rng = np.random.default_rng(n)
        group = scattered(rng, [n, 3])
        x = 285.0 + 10.0 * rng.normal(size=(n + 3, C))
        x[rng.random(x.shape) < 0.05] = np.nan
        x[:, 4] = np.where(rng.random(n + 3) < 0.3, 0.0, rng.integers(1, 4, size=n + 3) * 0.5)
        sorted_ = qo.sorted_groups(x, group, 2)
        for method in ("linear", "nearest", "median"):
            got, ran = kernels_of(ctx, lambda: ctx.quantile(x, QS, group, 2, method))
            assert ran == names, (n, ran)
            assert qo.same(got.to_host(), qo.quantile_sorted(sorted_, QS, method)), (n, method)
        got = ctx.quantile(x.astype(np.float32), QS, group, 2, "midpoint", skipna=False).to_host()
        assert qo.same(got, qo.quantile_field(x.astype(np.float32), QS, group, 2, "midpoint", False)), n


@pytest.mark.parametrize("T", [64 * 21 + 1, 1024 * 13 + 1, 1024 * 17 + 1, 19456])
def test_series_path_of_the_whole_axis(ctx, T):
    C = 9
    K = [k for k in SERIES_WIDTHS if T <= 1024 * k][0]
    rng = np.random.default_rng(T)
    x = 285.0 + 10.0 * rng.normal(size=(T, C))
    x[rng.random(x.shape) < 0.05] = np.nan
    x[:, 1] = np.nan
    x[:, 2] = np.where(rng.random(T) < 0.3, 0.0, rng.integers(1, 6, size=T) * 0.25)
    sorted_ = qo.sorted_groups(x)
    for method, skipna in (("linear", True), ("higher", True), ("median", True), ("lower", False)):
        got, names = kernels_of(ctx, lambda: ctx.quantile(x, QS, method=method, skipna=skipna))
        assert names == [f"quantile_runs_kernel<{K}>", f"quantile_select_kernel<{K}>"], names
        assert qo.same(got.to_host(), qo.quantile_sorted(sorted_, QS, method, skipna)), (T, method, skipna)
    x32 = x[:, :3].astype(np.float32)
    assert qo.same(ctx.quantile(x32, QS).to_host(), qo.quantile_field(x32, QS))


def test_series_longer_than_the_merge_is_refused(ctx):
    x = np.zeros((19457, 2))
    with pytest.raises(NotImplementedError, match=r"sd_quantile: a group of 19457 samples exceeds the workgroup merge \(19456\)"):
        ctx.quantile(x, 0.5)
    group = np.zeros(19457 + 5, dtype=np.int32)
    group[[1, 5000, 10000, 15000, 19000]] = 1  # one group too long among two
    with pytest.raises(NotImplementedError, match=r"sd_quantile: a group of 19457 samples exceeds the workgroup merge \(19456\)"):
        ctx.quantile(np.zeros((19457 + 5, 2)), 0.5, group, 2)


def test_series_path_of_two_long_groups_of_unequal_length(ctx):
    rng = np.random.default_rng(77)
    sizes = [1500, 5, 0, 3100, 64]
    group = scattered(rng, sizes)
    C = 17
    x = 285.0 + 10.0 * rng.normal(size=(len(group), C))
    x[rng.random(x.shape) < 0.05] = np.nan
    x[group == 3, 0] = np.nan
    sorted_ = qo.sorted_groups(x, group, 5)
    for method in METHODS:
        for skipna in (True, False):
            got, names = kernels_of(ctx, lambda: ctx.quantile(x, QS, group, 5, method, skipna))
            assert names == ["quantile_runs_kernel<13>", "quantile_select_kernel<13>"], names
            assert qo.same(got.to_host(), qo.quantile_sorted(sorted_, QS, method, skipna)), (method, skipna)
    assert np.isnan(got.to_host()[2::5]).all()  # the group without a row


@pytest.mark.parametrize("case", ["segment", "series"])
def test_layouts_give_the_same_bits(ctx, case):
    rng = np.random.default_rng(5)
    C = 10
    sizes = SIZES if case == "segment" else [1400, 40, 300]
    group = scattered(rng, sizes)
    G = len(sizes)
    x64 = field(rng, group, C)
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        want = qo.quantile_field(host, QS, group, G)
        rows = len(QS) * G
        # (name, source ld, elements in front of a source row, output ld, elements in front of an output row)
        for name, ld, lead, ld_out, lead_out in (("tight", C, 0, C, 0), ("padded even", C + 6, 4, C + 4, 2), ("padded odd", C + 5, 3, C + 3, 1),
                                                 ("source off by one element", C + 2, 1, C, 0)):
            _, src = view(ctx, host, ld, lead)
            parent, out = view(ctx, np.full((rows, C), 7.0), ld_out, lead_out)
            ctx.quantile(src, QS, group, G, out=out)
            assert qo.same(out.to_host(), want), f"{case} {np.dtype(dtype).name} {name}: differs from the oracle"
            back = parent.to_host()
            assert (back[:, :lead_out] == 7).all() and (back[:, lead_out + C:] == 7).all(), f"{case} {name}: padding of out written"
        # a view of the rows of a longer field, and the host twin
        longer = ctx.to_device(np.full((rows + 4, C), 7.0))
        ctx.quantile(host, QS, group, G, out=longer.rows(2, 2 + rows))
        back = longer.to_host()
        assert qo.same(back[2:2 + rows], want) and (back[:2] == 7).all() and (back[2 + rows:] == 7).all()
        assert qo.same(ctx.quantile_host(host, QS, group, G), want)
        assert qo.same(ctx.quantile_host(host, None, group, G, "median"), qo.quantile_field(host, None, group, G, "median"))


def test_c_abi_refusals_write_nothing(ctx):
    from skdownscale_amd._lib import ptr

    lib, h = ctx.lib, ctx.handle
    x = ctx.to_device(np.ones((10, 4)))
    out = ctx.to_device(np.full((6, 4), 7.0))
    ok = np.array([0, 1, 2] * 3 + [0], dtype=np.int32)
    bad = ok.copy()
    bad[6] = 3
    q2 = np.array([0.25, 0.75])

    def call(method=0, ld=4, T=10, C=4, group=ok, G=3, q=q2, Q=2, ld_out=4):
        return lib.sd_quantile_dev(h, method, 1, x.vptr, 0, ld, T, C, ptr(group), G, ptr(q), Q, out.vptr, ld_out)

    for kw, msg in ((dict(method=6), "unknown method code 6"), (dict(T=0), "bad sizes (T=0, C=4)"), (dict(G=0), "bad sizes (G=0, Q=2)"),
                    (dict(Q=0), "bad sizes (G=3, Q=0)"), (dict(q=np.array([0.5, 1.5])), "Quantiles must be in the range [0, 1] (q[1] = 1.5)"),
                    (dict(q=np.array([np.nan, 0.5])), "Quantiles must be in the range [0, 1] (q[0] = nan)"),
                    (dict(ld=3), "ld = 3 is less than the 4 cells of a row"), (dict(ld_out=3), "ld_out = 3 is less than the 4 cells of a row"),
                    (dict(group=bad), "group[6] = 3 lies outside the 3 groups"), (dict(G=2), "group[2] = 2 lies outside the 2 groups")):
        assert call(**kw) == SD_ERR_INVALID and lib.sd_last_error().decode().endswith(f"sd_quantile: {msg}"), (kw, lib.sd_last_error().decode())
    assert lib.sd_quantile_dev(h, 0, 1, None, 0, 4, 10, 4, ptr(ok), 3, ptr(q2), 2, out.vptr, 4) == SD_ERR_INVALID
    assert lib.sd_last_error().decode().endswith("sd_quantile: NULL argument")
    res = np.full((6, 4), 7.0)
    host = np.ones((10, 4))
    assert lib.sd_quantile(h, 0, 1, ptr(host), 0, 10, 4, ptr(bad), 3, ptr(q2), 2, ptr(res)) == SD_ERR_INVALID and (res == 7.0).all()
    assert (out.to_host() == 7).all()
    # the median reads neither q nor Q
    assert lib.sd_quantile_dev(h, 5, 1, x.vptr, 0, 4, 10, 4, ptr(ok), 3, None, 0, out.vptr, 4) == 0 and (out.to_host()[:3] == 1.0).all()
    # the engine's words
    with pytest.raises(ValueError, match=r"sd_quantile: Quantiles must be in the range \[0, 1\]"):
        ctx.quantile(host, [0.5, -0.5])
    with pytest.raises(ValueError, match="quantile method 'weibull'"):
        ctx.quantile(host, 0.5, method="weibull")
    with pytest.raises(ValueError, match="group: expected one group id per row"):
        ctx.quantile(host, 0.5, ok[:9], 3)
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape"):
        ctx.quantile(host, [0.5, 0.6], ok, 3, out=ctx.empty((3, 4)))


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(26)
    T = 1096
    time = pd.date_range("2003-01-01", periods=T, freq="D")
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    clat, clon = np.linspace(42.0, 38.0, 4), np.linspace(-110.0, -104.0, 5)
    flat, flon = np.linspace(42.0, 38.0, 9), np.linspace(-110.0, -104.0, 11)
    coarse = GridArray(285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, 4, 5)), ("time", "lat", "lon"), dict(time=time, lat=clat, lon=clon))
    values = 283.0 + season[:, None, None] + 2.0 * rng.normal(size=(T, 9, 11))
    values[rng.random(values.shape) < 0.05] = np.nan
    obs = GridArray(values, ("time", "lat", "lon"), dict(time=time, lat=flat, lon=flon))
    return coarse, obs


def oracle_of(values, q, group=None, G=None, method="linear", skipna=True):
    """the oracle on a host array whose first axis is time: [Q * G, *rest]"""
    flat = values.reshape(values.shape[0], -1)
    return qo.quantile_field(flat, q, group, G, method, skipna).reshape((-1,) + values.shape[1:])


def test_quantile_and_median_of_a_host_array(ctx, grids):
    from skdownscale_amd import GridArray

    _, obs = grids
    month = (obs.coords["time"].month - 1).to_numpy()
    a = obs.quantile(0.9)
    assert not a.computed and qo.same(a.values, oracle_of(obs.values, 0.9)[0]) and a.computed
    b = obs.quantile([0.05, 0.5, 0.95], "time", by="time.month", method="nearest")
    assert b.shape == (3, 12, 9, 11) and qo.same(b.values, oracle_of(obs.values, [0.05, 0.5, 0.95], month, 12, "nearest").reshape(3, 12, 9, 11))
    m = obs.median("time", by="time.season", skipna=False)
    season = (np.asarray(obs.coords["time"].month) % 12) // 3
    want = oracle_of(obs.values, None, np.argsort(["DJF", "MAM", "JJA", "SON"]).argsort()[season], 4, "median", False)
    assert list(m.coords["season"]) == ["DJF", "JJA", "MAM", "SON"] and qo.same(m.values, want)
    # float32 goes up as float32; time in the middle; a lazy cut of the cells
    f32 = GridArray(obs.values.astype(np.float32).transpose(1, 0, 2), ("lat", "time", "lon"), obs.coords)
    got = f32.quantile(1.0 / 3.0, "time", by="time.month")
    assert got.dims == ("lat", "month", "lon") and got.dtype == np.float64
    want = oracle_of(obs.values.astype(np.float32), 1.0 / 3.0, month, 12)
    assert qo.same(got.values.transpose(1, 0, 2), want)
    part = f32.quantile(1.0 / 3.0, "time", by="time.month").isel(lat=slice(2, 5), lon=slice(1, 8))
    assert not part.computed and qo.same(part.values.transpose(1, 0, 2), want[:, 2:5, 1:8])
    # the day of the year: 366 groups of three or fewer samples; the whole axis: the series path is not needed for 1 096 steps
    doy = obs.quantile(0.5, "time", by="time.dayofyear")
    ids = (obs.coords["time"].dayofyear - 1).to_numpy()
    assert doy.shape == (366, 9, 11) and qo.same(doy.values, oracle_of(obs.values, 0.5, ids, 366))


def test_quantile_of_lazy_sources_stays_resident(ctx, grids):
    coarse, obs = grids
    monthly = obs.resample(time="MS").mean()
    got = monthly.quantile([0.1, 0.9], "time", by="time.month")
    want_src = obs.resample(time="MS").mean().values
    ids = (monthly.coords["time"].month - 1).to_numpy()
    assert qo.same(got.values, oracle_of(want_src, [0.1, 0.9], ids, 12).reshape(2, 12, 9, 11)) and not monthly.computed
    fine = coarse.interp_like(obs)
    med = fine.median()
    assert qo.same(med.values, oracle_of(coarse.interp_like(obs).values, None, method="median")[0]) and not fine.computed
    blocked = coarse.interp_like(obs).quantile(0.5, scratch_bytes=200 * 99 * 8)  # regridded in six blocks of rows
    assert qo.same(blocked.values, med.values)
    rolled = obs.rolling(time=9, center=True, min_periods=1).mean()
    assert qo.same(rolled.quantile(0.95).values, oracle_of(obs.rolling(time=9, center=True, min_periods=1).mean().values, 0.95)[0]) and not rolled.computed


def test_a_lazy_grouped_quantile_feeds_groupby_arithmetic_and_rolling(ctx, grids):
    from skdownscale_amd import GridArray

    _, obs = grids
    med = obs.quantile(0.5, "time", by="time.month")
    anom = obs.groupby("time.month") - med
    got = anom.values
    assert not med.computed  # the medians went from the sort to the subtraction in HBM
    handed = obs.quantile(0.5, "time", by="time.month").compute()
    assert type(handed) is GridArray and np.array_equal((obs.groupby("time.month") - handed).values, got, equal_nan=True)
    # a day-of-year percentile threshold, smoothed
    thr = obs.quantile(0.9, "time", by="time.dayofyear")
    smooth = thr.rolling(dayofyear=5, center=True, wrap=True).mean()
    got = smooth.values
    assert got.shape == (366, 9, 11) and not thr.computed
    handed = obs.quantile(0.9, "time", by="time.dayofyear").compute()
    assert np.array_equal(handed.rolling(dayofyear=5, center=True, wrap=True).mean().values, got, equal_nan=True)
    assert np.isfinite(got[:360]).mean() > 0.99  # (day 366 has one sample in these three years: NaN where that one is)
