"""GPU: resample_kernel (csrc/sd_resample.hip) through Context.resample / sd_resample against tests/_resample_oracle.py and pandas'
results in tests/golden/g25_resample.npz, the lazy GridArray.resample surface, its chaining with interp_like, and the resident BCSD
path of PointWiseDownscaler on lazy monthly X and y.

Tolerance (derived, tests/_resample_oracle.py: bound): for a bin with n non-NaN samples plain and compensated float64 summation both
stay within n * 2^-53 * sum|x_i| of the exact sum, so |got - want| <= (n + 2) * 2^-53 * sum|x_i| for ``sum``; the same divided by n plus
one ulp of the result for ``mean``.  NaN / 0.0 patterns of bins without a sample match exactly.  Results of different layouts, cells
per lane and block sizes of the same data are compared bit for bit: a bin is added in time order by one lane."""
import os

import numpy as np
import pandas as pd
import pytest

import _regrid_oracle as ro
import _resample_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GROUP = 8  # bins of a workgroup (sdrs::kBinsPerGroup, pinned by tests/test_resample_plan.py); 8 rows are in flight per batch
# T = 120: an empty first, middle and last bin; lengths 1, 7, 8, 9 (one row, a partial, a whole and a whole + partial batch), 16, 31;
# M = 12 is more than one workgroup's run of bins
LENGTHS = [0, 1, 7, 8, 9, 31, 0, 31, 8, 16, 9, 0]
CELLS = [1, 63, 64, 65, 130, 257]
OPS = ["mean", "sum"]
CASES = ["ms_gap", "me", "ys", "7d", "1d_subdaily", "nan_run_and_all_nan_bin", "float32"]


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g25_resample.npz"))
    return {name: {k: g[f"{name}.{k}"] for k in ("time", "values", "rule", "labels", "size", "mean", "sum")} for name in CASES}


def table(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def field(rng, T, C, offsets):
    """temperatures with 5 % NaN samples, an all-NaN bin in cell 0 (the first bin of 31) and a NaN run inside a bin in the last cell"""
    x = 285.0 + 10.0 * rng.normal(size=(T, C))
    x[rng.random((T, C)) < 0.05] = np.nan
    long = int(np.flatnonzero(np.diff(offsets) == 31)[0])
    x[offsets[long]:offsets[long + 1], 0] = np.nan
    x[offsets[long] + 3:offsets[long] + 12, -1] = np.nan
    return x


def source_view(ctx, host, ld, lead):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart"""
    T, C = host.shape
    parent = np.full((T, ld), 7.0, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    return ctx.to_device(parent, host.dtype).cells(lead, lead + C)


@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C):
    rng = np.random.default_rng(1000 + C)
    offsets = table(LENGTHS)
    T, M = int(offsets[-1]), len(LENGTHS)
    assert T == 120 and M == GROUP + 4
    x64 = field(rng, T, C, offsets)
    even = C + 6 if C % 2 == 0 else C + 5  # a padded leading dimension that keeps two cells per lane possible
    # (name, source ld, elements in front of a source row, output ld, doubles in front of an output row)
    layouts = [("tight", C, 0, C, 0), ("padded even", even + 2, 4, even, 2), ("padded odd", C + 5 - C % 2, 4, C + 3 - C % 2, 2),
               ("output off by one double", C, 0, C + 2, 1)]
    worst = 0.0
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        want = {op: so.resample(host, offsets, op) for op in OPS}
        for op in OPS:
            first = None
            for name, ld, lead, ld_out, lead_out in layouts:
                src = source_view(ctx, host, ld, lead) if (ld, lead) != (C, 0) else ctx.to_device(host, dtype)
                parent = ctx.to_device(np.full((M, ld_out), 7.0))
                out = ctx.resample(src, offsets, op, out=parent.cells(lead_out, lead_out + C) if (ld_out, lead_out) != (C, 0) else parent)
                got = out.to_host()
                what = f"C={C} {np.dtype(dtype).name} {op} {name}"
                worst = max(worst, so.check(got, want[op], host, offsets, op, what))
                back = parent.to_host()
                assert (back[:, :lead_out] == 7.0).all() and (back[:, lead_out + C:] == 7.0).all(), f"{what}: padding written"
                first = got if first is None else first
                assert np.array_equal(got, first, equal_nan=True), f"{what}: differs from the tight layout"
            empty = np.diff(offsets) == 0
            assert np.isnan(first[empty]).all() if op == "mean" else (first[empty] == 0.0).all()
            long = int(np.flatnonzero(np.diff(offsets) == 31)[0])
            assert np.isnan(first[long, 0]) if op == "mean" else first[long, 0] == 0.0  # the all-NaN bin
    print(f"C={C}: worst |got - want| / bound = {worst:.3f}")


@pytest.mark.parametrize("lengths", [[120], [13] * (GROUP + 1), [5] * GROUP, [3, 0] * GROUP + [3]], ids=["M=1", "M=group+1", "M=group", "M=2*group+1"])
def test_bin_counts_at_the_edges_of_a_workgroup(ctx, lengths):
    rng = np.random.default_rng(len(lengths))
    offsets = table(lengths)
    for C in (65, 130):
        x = field(rng, int(offsets[-1]), C, table([31, int(offsets[-1]) - 31]))
        for op in OPS:
            got = ctx.resample(x, offsets, op)
            assert got.shape == (len(lengths), C)
            so.check(got.to_host(), so.resample(x, offsets, op), x, offsets, op, f"M={len(lengths)} C={C} {op}")


def test_float32_source_equals_the_widened_source(ctx):
    rng = np.random.default_rng(3)
    offsets = table(LENGTHS)
    for C in (63, 130, 260):  # one, two and four cells per lane for float32
        x32 = field(rng, 120, C, offsets).astype(np.float32)
        for op in OPS:
            got32 = ctx.resample(x32, offsets, op).to_host()
            assert got32.dtype == np.float64 and np.array_equal(got32, ctx.resample(x32.astype(np.float64), offsets, op).to_host(), equal_nan=True)
            assert np.array_equal(got32, ctx.resample(ctx.to_device(x32, np.float32), offsets, op).to_host(), equal_nan=True)  # resident float32
            assert np.array_equal(got32, ctx.resample_host(x32, offsets, op), equal_nan=True)  # sd_resample equals sd_resample_dev


def test_inf_follows_ieee(ctx):
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, inf, -inf, 1.0], [inf, -inf, nan, 2.0], [2.0, 1.0, nan, 3.0]])
    got = {op: ctx.resample(x, [0, 3], op).to_host()[0] for op in OPS}
    assert np.array_equal(got["sum"], [inf, nan, -inf, 6.0], equal_nan=True)
    assert np.array_equal(got["mean"], [inf, nan, -inf, 2.0], equal_nan=True)


@pytest.mark.parametrize("name", CASES)
def test_goldens_through_the_c_abi_and_the_grid_array(ctx, golden, name):
    from skdownscale_amd import GridArray

    c = golden[name]
    offsets = table(c["size"])
    array = GridArray(c["values"], ("time", "cell"), dict(time=c["time"], cell=np.arange(c["values"].shape[1])))
    for op in OPS:
        so.check(ctx.resample_host(c["values"], offsets, op), c[op], c["values"], offsets, op, f"{name} {op} sd_resample")
        lazy = getattr(array.resample(time=str(c["rule"])), op)()
        assert not lazy.computed and lazy.shape == c[op].shape
        so.check(lazy.values, c[op], c["values"], offsets, op, f"{name} {op} GridArray.resample")
        assert lazy.computed and np.array_equal(np.asarray(lazy.coords["time"]), c["labels"]) and lazy.values is lazy.values
        assert np.array_equal(lazy.device_field(ctx).to_host(), lazy.values, equal_nan=True)


def test_other_layouts_and_keywords(ctx):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(5)
    time = pd.date_range("2001-01-17", periods=90, freq="D")
    v = rng.normal(size=(3, 90, 5))  # time in the middle: brought to [T, C] on the host
    a = GridArray(v, ("lat", "time", "lon"), dict(time=time, lat=np.arange(3.0), lon=np.arange(5.0)))
    flat = v.transpose(1, 0, 2).reshape(90, 15)
    for kw in (dict(), dict(closed="right", label="right"), dict(offset="3D")):
        frame = pd.DataFrame(flat, index=time).resample("7D", **kw)
        offsets = table(frame.size().to_numpy())
        for op in OPS:
            lazy = getattr(a.resample(time="7D", **kw), op)()
            want = getattr(frame, op)()
            assert lazy.dims == a.dims and lazy.shape == (3, len(want), 5) and list(lazy.coords["time"]) == list(want.index)
            so.check(lazy.values.transpose(1, 0, 2).reshape(len(want), 15), want.to_numpy(), flat, offsets, op, f"7D {kw} {op}")
    computed = a.resample(time="MS").mean()
    assert np.array_equal(computed.isel(time=slice(1, 3)).values, computed.values[:, 1:3]) and computed.transpose("time", "lat", "lon").shape == (4, 3, 5)
    assert np.array_equal(computed.isel(lon=slice(1, 4)).values, computed.values[:, :, 1:4])  # lazy on the sliced source: the same bins


def test_host_source_blocks_are_bit_identical(ctx):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(6)
    time = pd.date_range("2001-01-17", periods=330 + 70, freq="D")
    time = time[:130].append(time[200:])  # two empty months
    for dtype in (np.float64, np.float32):
        v = (285.0 + 10.0 * rng.normal(size=(330, 4, 33))).astype(dtype)
        a = GridArray(v, ("time", "lat", "lon"), dict(time=time))
        for op in OPS:
            whole = getattr(a.resample(time="MS"), op)().values
            offsets = getattr(a.resample(time="MS"), op)().offsets
            so.check(whole.reshape(14, -1), so.resample(v.reshape(330, -1), offsets, op), v.reshape(330, -1), offsets, op, f"blocks {op}")
            for scratch_bytes in (1, 40 * 132 * v.itemsize, 100 * 132 * v.itemsize):  # one bin per block; a bin or two; a few
                assert np.array_equal(getattr(a.resample(time="MS", scratch_bytes=scratch_bytes), op)().values, whole, equal_nan=True), scratch_bytes


# ---- chaining with interp_like and the driver -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_case():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(14)
    T = 2922  # eight years: 96 months
    time = pd.date_range("2001-01-01", periods=T, freq="D")
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    clat, clon = np.array([42.0, 40.0, 38.0]), np.array([-110.0, -108.0, -106.0])  # descending latitude
    fine_lat, fine_lon = np.linspace(42.0, 38.0, 6), np.linspace(-110.0, -106.0, 8)
    fine_lat[-1], fine_lon[-1] = 37.5, -105.5  # the last row and column lie outside the coarse hull: 13 masked cells

    def coarse(shift, dtype):
        v = 285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, 3, 3)) + shift
        return GridArray(v.astype(dtype), ("time", "lat", "lon"), dict(time=time, lat=clat, lon=clon))

    obs_v = 283.0 + season[:, None, None] + 2.0 * rng.normal(size=(T, 6, 8))
    obs = GridArray(obs_v, ("time", "lat", "lon"), dict(time=time, lat=fine_lat, lon=fine_lon))
    return coarse(0.0, np.float64), coarse(1.5, np.float32), obs


def test_chain_equals_regrid_oracle_then_resample_oracle(ctx, driver_case):
    hist, fut, obs = driver_case
    for coarse in (hist, fut):  # float64 and float32 coarse data
        src = np.asarray(coarse.values)
        fine = ro.regrid(src, coarse.coords["lat"], coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"]).reshape(len(src), -1)
        scale = np.abs(src.astype(np.float64)).max()
        for op in OPS:
            lazy = getattr(coarse.interp_like(obs).resample(time="MS"), op)()
            got = lazy.values
            assert got.shape == (96, 6, 8) and not lazy.source.computed  # the fine daily field never came to the host
            want, bound = so.resample(fine, lazy.offsets, op), so.bound(fine, lazy.offsets, op)
            # the regridded samples are within 1e-12 * max|source| of the oracle's (tests/test_gpu_regrid.py); a sum of n of them moves by
            # at most n times that, a mean by at most that
            n = np.diff(lazy.offsets)[:, None] if op == "sum" else 1.0
            got2 = got.reshape(96, -1)
            assert np.array_equal(np.isnan(got2), np.isnan(want))
            err = np.nan_to_num(np.abs(got2 - want), nan=0.0)
            assert (err <= bound + n * 1e-12 * scale).all(), (op, float((err / (bound + n * 1e-12 * scale)).max()))
            outside = np.concatenate([got[:, -1, :].ravel(), got[:, :, -1].ravel()])  # all-NaN bins: NaN for mean, pandas' 0.0 for sum
            assert (np.isnan(outside).all() if op == "mean" else (outside == 0.0).all()) and np.isfinite(got[:, :-1, :-1]).all()
            # one bin per block, a few bins per block, one block for everything: bit-identical
            for scratch_bytes in (1, 100 * 48 * 8):
                blocked = getattr(coarse.interp_like(obs).resample(time="MS", scratch_bytes=scratch_bytes), op)()
                assert np.array_equal(blocked.values, got, equal_nan=True), scratch_bytes
            # and equal to the materialised fine field resampled as a plain host array: the same kernels on the same values
            plain = getattr(coarse.interp_like(obs).compute().resample(time="MS"), op)().values
            assert np.array_equal(plain, got, equal_nan=True)


def test_driver_lazy_monthly_equals_host_arrays(ctx, driver_case):
    from skdownscale_amd import BcsdTemperature, GridArray, PointWiseDownscaler

    hist, fut, obs = driver_case
    X = hist.interp_like(obs).resample(time="MS").mean()
    Xp = fut.interp_like(obs).resample(time="MS").mean()
    y = obs.resample(time="MS").mean()

    def run(X_fit, y_fit, X_pred):
        model = PointWiseDownscaler(BcsdTemperature(return_anoms=False))
        model.fit(X_fit, y_fit)
        return np.asarray(model.predict(X_pred).values), model._models.mask

    resident, mask = run(X, y, Xp)
    assert not X.computed and not Xp.computed and not y.computed  # the monthly fields never came to the host ...
    assert not X.source.computed and not Xp.source.computed       # ... nor the fine daily ones
    host = [GridArray(a.values, a.dims, a.coords) for a in (X, y, Xp)]
    materialised, mask_host = run(*host)
    assert resident.shape == (96, 6, 8) and resident.dtype == np.float64
    assert np.array_equal(resident, materialised, equal_nan=True)
    assert np.array_equal(mask, mask_host) and mask.sum() == 35 and not mask.reshape(6, 8)[-1, :].any() and not mask.reshape(6, 8)[:, -1].any()
    assert np.isnan(resident[:, -1, :]).all() and np.isnan(resident[:, :, -1]).all() and np.isfinite(resident[:, :-1, :-1]).all()
    # a lazy X with host y, and a host X with lazy y (every other path sees a GridArray and uses .values)
    assert np.array_equal(run(X, host[1], Xp)[0], resident, equal_nan=True)
    assert np.array_equal(run(host[0], y, host[2])[0], resident, equal_nan=True)


def test_errors(ctx):
    from skdownscale_amd.engine import Context

    x = np.zeros((10, 4))
    for offsets, msg in (([0, 5, 4, 10], r"sd_resample: offsets decrease at bin 1 \(4 after 5\)"), ([1, 10], r"offsets\[0\] = 1, expected 0"),
                         ([0, 9], r"offsets\[M\] = 9, expected T = 10"), ([0, 12], r"offsets\[M\] = 12, expected T = 10"), ([0], "bad sizes")):
        with pytest.raises(ValueError, match=msg):
            ctx.resample(x, offsets)
        if len(offsets) > 1:
            with pytest.raises(ValueError, match=msg):
                ctx.resample_host(x, offsets)
    with pytest.raises(NotImplementedError, match="only 'mean' and 'sum'"):
        ctx.resample(x, [0, 10], "max")
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape"):
        ctx.resample(x, [0, 10], out=ctx.empty((2, 4)))
    with pytest.raises(ValueError, match="field: expected a float32 or float64"):
        ctx.resample(np.zeros(10), [0, 10])
    other = Context(0)
    with pytest.raises(ValueError, match="sd_resample: `out` belongs to another context"):
        ctx.resample(x, [0, 10], out=other.empty((1, 4)))
    with pytest.raises(ValueError, match="sd_resample: `field` belongs to another context"):
        ctx.resample(other.to_device(x), [0, 10])
    other.close()
    # the C ABI itself refuses a short leading dimension with the plan's message
    from skdownscale_amd._lib import check, ptr

    d, out = ctx.to_device(x), ctx.empty((1, 4))
    off = np.array([0, 10], dtype=np.int64)
    with pytest.raises(ValueError, match="sd_resample: ld = 3 is less than the 4 cells of a row"):
        check(ctx.lib.sd_resample_dev(ctx.handle, 0, d.vptr, 0, 3, 10, 4, ptr(off), 1, out.vptr, 4))
    with pytest.raises(ValueError, match="sd_resample: unknown op code 9"):
        check(ctx.lib.sd_resample_dev(ctx.handle, 9, d.vptr, 0, 4, 10, 4, ptr(off), 1, out.vptr, 4))
