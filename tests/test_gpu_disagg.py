"""GPU: disagg_kernel (csrc/sd_disagg.hip) through Context.disaggregate / sd_disagg_dev / sd_disagg against tests/_disagg_oracle.py, the
lazy GridArray.disaggregate surface, the closed loop with the engine's own GridArray.resample, and the monthly BCSD recipe end to end.

Every comparison with the oracle is bit for bit, the NaN pattern included: the kernel and the oracle make the same single IEEE adds,
subtracts, multiplies and divides in the same order (the library is built with -ffp-contract=off), a lane owns its cells for a whole
bin, and float32 observations are widened per sample -- so neither the layout, the cells per lane nor the block size can move a bit."""
import numpy as np
import pandas as pd
import pytest

import _disagg_oracle as do

pytestmark = pytest.mark.gpu

GROUP = 8  # bins of a workgroup (sddg::kBinsPerGroup, pinned by tests/test_disagg_plan.py); 8 rows are in flight per batch
# 17 bins: months of 28 / 29 / 30 / 31 rows and a bin of one row; (GROUP + 1 of them are one more than a workgroup owns)
LENGTHS = [31, 28, 29, 30, 1, 31, 29, 28, 30, 31, 28, 31, 30, 31, 30, 31, 31]
# rows of the source month relative to the bin: 28 rows on 29 drop the last day, 29 rows on 28 repeat it
SOURCE = [0, +1, -1, 0, 0, -1, +1, 0, +1, 0, 0, -1, 0, 0, +1, 0, -1]
# 129 = 64 * 2 + 1 and 257 = 64 * 4 + 1: one cell more than a tile of two (float64) and of four (float32) cells per lane; 260: more than one
# tile at four cells per lane (an odd C always runs one cell per lane)
CELLS = [1, 63, 129, 130, 257, 260]


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def tables(M, rng):
    """(src_row, offsets, To): bin m borrows a run of LENGTHS[m] + SOURCE[m] rows of its own, the runs in shuffled order"""
    lengths = np.array(LENGTHS[:M])
    n_src = np.maximum(lengths + np.array(SOURCE[:M]), 1)
    start = np.zeros(M, dtype=np.int64)
    at = 2  # (two rows in front and one behind that nobody borrows)
    for m in rng.permutation(M):
        start[m], at = at, at + n_src[m]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    src_row = np.concatenate([start[m] + np.minimum(np.arange(lengths[m]), n_src[m] - 1) for m in range(M)]).astype(np.int64)
    return src_row, offsets, int(at + 1)


def view(ctx, host, ld, lead, fill=7.0):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart -> (parent, view)"""
    T, C = host.shape
    parent = np.full((T, ld), fill, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    d = ctx.to_device(parent, host.dtype)
    return d, d.cells(lead, lead + C)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]!r} != {want[bad][0]!r}"


def weather(rng, To, C):
    """temperatures and zero-inflated precipitation, 3 % NaN samples each"""
    tas = 285.0 + 10.0 * rng.normal(size=(To, C))
    pr = np.where(rng.random((To, C)) < 0.6, 0.0, rng.gamma(0.7, 6.0, size=(To, C)))
    tas[rng.random((To, C)) < 0.03] = np.nan
    pr[rng.random((To, C)) < 0.03] = np.nan
    return tas, pr


@pytest.mark.parametrize("M", [1, GROUP + 1, 17])
@pytest.mark.parametrize("C", CELLS)
def test_shape_sweep(ctx, C, M):
    rng = np.random.default_rng(1000 * M + C)
    src_row, offsets, To = tables(M, rng)
    Tout = int(offsets[-1])
    tas, pr = weather(rng, To, C)
    group = (np.arange(M) % 12).astype(np.int32)
    # (name, elements in front of an obs row, obs ld, doubles in front of an output row, output ld, rows in front of the target)
    layouts = [("tight", 0, C, 0, C, 0),
               ("inside wider fields", 4, C + 10, 2, C + 6, 1),      # 16-byte leads: the widest access the evenness of C allows
               ("off by one element", 1, C + 3, 1, C + 2, 0)]        # pointers off 16 bytes: one cell per lane
    for dtype in (np.float64, np.float32):
        for op in do.OPS:
            obs = (tas if op == "shift" else pr).astype(dtype)
            target = 288.0 + 5.0 * rng.normal(size=(M, C)) if op == "shift" else rng.gamma(2.0, 40.0 if op == "scale_sum" else 1.5, size=(M, C))
            base = 280.0 + rng.normal(size=(12, C)) if op == "shift" else 0.5 + rng.gamma(2.0, 1.0, size=(12, C))
            for climo in (None, base):
                anomaly = target if climo is None else (target - base[group] if op == "shift" else target / base[group])
                want = do.disaggregate(anomaly, obs, src_row, offsets, op, climo, None if climo is None else group)
                for name, lead, ld, lead_out, ld_out, rows_front in layouts:
                    what = f"C={C} M={M} {np.dtype(dtype).name} {op} climo={climo is not None} {name}"
                    d_obs = ctx.to_device(obs, dtype) if (lead, ld) == (0, C) else view(ctx, obs, ld, lead)[1]
                    parent = ctx.to_device(np.full((Tout, ld_out), 7.0))
                    out = parent if (lead_out, ld_out) == (0, C) else parent.cells(lead_out, lead_out + C)
                    long_target = np.concatenate([np.full((rows_front, C), 9.0), anomaly, np.full((1, C), 9.0)])
                    d_target = ctx.to_device(long_target).rows(rows_front, rows_front + M)
                    d_climo = None if climo is None else (ctx.to_device(climo) if lead == 0 else view(ctx, climo, ld, lead)[1])
                    got = ctx.disaggregate(d_target, d_obs, src_row, offsets, op, d_climo, None if climo is None else group, out=out)
                    assert got is out
                    same(got.to_host(), want, what)
                    back = parent.to_host()
                    assert (back[:, :lead_out] == 7.0).all() and (back[:, lead_out + C:] == 7.0).all(), f"{what}: padding written"


def test_special_values(ctx):
    """a NaN cell, one NaN day, an all-NaN bin, a NaN target, a dry source month with a positive and with a zero target, inf"""
    rng = np.random.default_rng(5)
    M, C = GROUP + 1, 130
    src_row, offsets, To = tables(M, rng)
    nan, inf = np.nan, np.inf

    def bin_rows(m):
        return src_row[offsets[m]:offsets[m + 1]]

    for dtype in (np.float64, np.float32):
        for op in do.OPS:
            tas, pr = weather(rng, To, C)
            obs = tas if op == "shift" else pr
            obs[:, 7] = nan                      # a NaN cell
            obs[bin_rows(0), 1] = 250.0 + np.arange(31)
            obs[bin_rows(0)[4], 1] = nan         # one NaN day
            obs[bin_rows(3), 2] = nan            # an all-NaN bin
            obs[bin_rows(5), 3:5] = 0.0          # a dry source month: cell 3 with a positive target, cell 4 with a zero target
            obs[bin_rows(4), 3] = 0.0            # ... and a dry bin of one row
            obs[bin_rows(6), 5] = 1.0
            obs[bin_rows(6)[2], 5] = inf         # inf follows IEEE arithmetic
            obs[bin_rows(7)[0], 6] = -0.0
            obs[bin_rows(2), 10] = 1.0 + np.arange(29)
            obs = obs.astype(dtype)
            target = 288.0 + rng.normal(size=(M, C)) if op == "shift" else rng.gamma(2.0, 20.0, size=(M, C))
            target[5, 3], target[5, 4], target[4, 3] = 12.5, 0.0, 3.0
            target[2, 9] = nan                   # a NaN target
            target[8, 10] = inf
            for climo, group in ((None, None), (1.0 + rng.random((3, C)), (np.arange(M) % 3).astype(np.int32))):
                want = do.disaggregate(target, obs, src_row, offsets, op, climo, group)
                got = ctx.disaggregate(target, obs, src_row, offsets, op, climo, group).to_host()
                same(got, want, f"{np.dtype(dtype).name} {op} climo={climo is not None}")
                assert np.isnan(got[:, 7]).all() and np.isnan(got[offsets[3]:offsets[4], 2]).all() and np.isnan(got[offsets[2]:offsets[3], 9]).all()
                day = got[offsets[0]:offsets[1], 1]
                assert np.isnan(day[4]) and np.isfinite(np.delete(day, 4)).all()
                assert np.isfinite(got[offsets[2]:offsets[3], 10]).all()  # the neighbours of the NaN target
                if climo is None and op != "shift":
                    n = offsets[6] - offsets[5]
                    assert (got[offsets[5]:offsets[6], 3] == (12.5 if op == "scale_mean" else 12.5 / n)).all()
                    assert (got[offsets[5]:offsets[6], 4] == 0.0).all() and got[offsets[4], 3] == 3.0
                if climo is None and op == "shift":  # the monthly mean of the NaN-day cell equals its target
                    assert abs(np.nanmean(day) - target[0, 1]) <= 1e-12 * 300.0


def test_the_host_twin_equals_the_device_path(ctx):
    rng = np.random.default_rng(8)
    M = 5
    src_row, offsets, To = tables(M, rng)
    group = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    for C in (63, 130, 260):  # one, two and four cells per lane for float32
        tas, pr = weather(rng, To, C)
        for dtype in (np.float64, np.float32):
            for op in do.OPS:
                obs = (tas if op == "shift" else pr).astype(dtype)
                target = 1.0 + rng.random((M, C))
                for climo in (None, 1.0 + rng.random((2, C))):
                    g = None if climo is None else group
                    want = do.disaggregate(target, obs, src_row, offsets, op, climo, g)
                    same(ctx.disaggregate_host(target, obs, src_row, offsets, op, climo, g), want, f"sd_disagg C={C} {op}")
                    same(ctx.disaggregate(target, obs, src_row, offsets, op, climo, g).to_host(), want, f"sd_disagg_dev C={C} {op}")
                    resident = ctx.disaggregate(ctx.to_device(target), ctx.to_device(obs, dtype), src_row, offsets, op,
                                                None if climo is None else ctx.to_device(climo), g)
                    same(resident.to_host(), want, f"resident C={C} {op}")


# ---- the GridArray surface ---------------------------------------------------------------------------------------------------------------
def daily_obs(rng, start, end, shape, dtype=np.float64, precip=False):
    from skdownscale_amd import GridArray

    time = pd.date_range(start, end, freq="D")
    T = len(time)
    if precip:
        v = np.where(rng.random((T,) + shape) < 0.6, 0.0, rng.gamma(0.7, 6.0, size=(T,) + shape))
    else:
        v = 283.0 + 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25).reshape((T,) + (1,) * len(shape)) + 2.0 * rng.normal(size=(T,) + shape)
    return GridArray(v.astype(dtype), ("time", "lat", "lon"), dict(time=time, lat=np.arange(float(shape[0])), lon=np.arange(float(shape[1]))))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_same_year_reconstruction_closes_the_loop_with_resample(ctx, dtype):
    """resample -> disaggregate with every month's own year gives the observations back, bit for bit"""
    rng = np.random.default_rng(21)
    obs = daily_obs(rng, "2003-01-01", "2004-12-31", (3, 5), dtype)  # a leap year among them
    v = obs.values
    v[:, 0, 0] = np.nan          # a NaN cell
    v[40, 1, 1] = np.nan         # a NaN day
    v[59:90, 2, 2] = np.nan      # March 2003 all NaN in one cell
    back = obs.resample(time="MS").mean().disaggregate(obs, years="same")
    assert not back.computed and back.shape == v.shape and back.dims == obs.dims and back.dtype == np.float64
    assert back.coords["time"].equals(pd.DatetimeIndex(obs.coords["time"]))
    assert np.array_equal(back.values, v.astype(np.float64), equal_nan=True)
    assert back.computed and back.values is back.values
    pr = daily_obs(rng, "2003-01-01", "2004-12-31", (3, 5), dtype, precip=True)
    pr.values[31:59, 1, 2] = 0.0  # a dry February
    pr.values[40, 1, 1] = np.nan
    back = pr.resample(time="MS").sum().disaggregate(pr, kind="scale", stat="sum", years="same")
    assert np.array_equal(back.values, pr.values.astype(np.float64), equal_nan=True)


def test_block_size_independence_and_the_device_field(ctx):
    from skdownscale_amd import GridArray, time_map

    rng = np.random.default_rng(22)
    obs = daily_obs(rng, "2001-01-01", "2004-12-31", (4, 33), np.float32)
    months = pd.date_range("2050-01-01", periods=14, freq="MS")
    monthly = GridArray(288.0 + rng.normal(size=(14, 4, 33)), ("time", "lat", "lon"), dict(time=months))
    climatology = rng.normal(size=(12, 4, 33))
    C = 4 * 33
    for kw in (dict(), dict(climatology=climatology), dict(kind="scale", stat="mean", climatology=GridArray(1.0 + climatology ** 2, ("month", "lat", "lon")))):
        whole = monthly.disaggregate(obs, seed=5, **kw)
        out_time, src_row, offsets = time_map(months, obs.coords["time"], None, 5)
        assert whole.coords["time"].equals(out_time) and np.array_equal(whole.src_row, src_row) and np.array_equal(whole.offsets, offsets)
        op = "scale_mean" if kw.get("kind") == "scale" else "shift"
        climo = None if not kw else np.asarray(kw["climatology"].values if isinstance(kw["climatology"], GridArray) else kw["climatology"]).reshape(12, C)
        want = do.disaggregate(monthly.values.reshape(14, C), obs.values.reshape(-1, C), src_row, offsets, op, climo,
                               None if climo is None else (months.month.to_numpy() - 1).astype(np.int32))
        same(whole.values.reshape(-1, C), want, f"whole {sorted(kw)}")
        for scratch_bytes in (1, 70 * C * 8, 1 << 30):  # one month per block; two; everything
            blocked = monthly.disaggregate(obs, seed=5, scratch_bytes=scratch_bytes, **kw)
            assert np.array_equal(blocked.values, whole.values, equal_nan=True), scratch_bytes
            field = blocked.device_field(ctx)
            assert field.shape == (len(out_time), C) and np.array_equal(field.to_host(), want, equal_nan=True)
            field.free()
    # time in the middle: the result keeps the dims of the monthly array
    turned = GridArray(monthly.values.transpose(1, 0, 2), ("lat", "time", "lon"), dict(time=months)).disaggregate(obs, seed=5)
    assert turned.dims == ("lat", "time", "lon") and np.array_equal(turned.values.transpose(1, 0, 2), monthly.disaggregate(obs, seed=5).values)


def test_public_refusals(ctx):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(23)
    obs = daily_obs(rng, "2001-01-01", "2002-12-31", (2, 3))
    months = pd.date_range("2001-01-01", periods=4, freq="MS")
    monthly = GridArray(np.zeros((4, 2, 3)), ("time", "lat", "lon"), dict(time=months))
    with pytest.raises(ValueError, match="kind='scale' needs stat='mean' or stat='sum'"):
        monthly.disaggregate(obs, kind="scale")
    with pytest.raises(ValueError, match="kind='scale' needs stat='mean' or stat='sum'"):
        monthly.disaggregate(obs, kind="scale", stat="median")
    with pytest.raises(ValueError, match="expected 'shift' or 'scale'"):
        monthly.disaggregate(obs, kind="ratio")
    with pytest.raises(ValueError, match="kind='shift' matches the monthly mean"):
        monthly.disaggregate(obs, stat="sum")
    with pytest.raises(ValueError, match="the monthly time coordinate must be a DatetimeIndex"):
        GridArray(np.zeros((4, 2, 3)), ("time", "lat", "lon"), dict(time=np.arange(4))).disaggregate(obs)
    with pytest.raises(ValueError, match="the daily time coordinate must be a DatetimeIndex"):
        monthly.disaggregate(GridArray(obs.values, obs.dims, dict(time=np.arange(obs.shape[0]))))
    with pytest.raises(ValueError, match="has no coordinate for dim 'time'"):
        GridArray(np.zeros((4, 2, 3)), ("time", "lat", "lon")).disaggregate(obs)
    with pytest.raises(ValueError, match="daily_obs has sizes"):
        monthly.disaggregate(GridArray(obs.values[:, :, :2], obs.dims, dict(time=obs.coords["time"])))
    with pytest.raises(ValueError, match="daily_obs: expected a GridArray"):
        monthly.disaggregate(obs.values)
    with pytest.raises(ValueError, match=r"climatology has shape \(11, 2, 3\); expected \(12, 2, 3\)"):
        monthly.disaggregate(obs, climatology=np.zeros((11, 2, 3)))
    with pytest.raises(ValueError, match="do not hold every day of 2003-02 exactly once: it cannot be borrowed for 2001-02"):
        monthly.disaggregate(obs, years=np.array([2001, 2003, 2001, 2002]))
    with pytest.raises(ValueError, match="do not hold every day of 2003-01 exactly once"):
        GridArray(np.zeros((1, 2, 3)), ("time", "lat", "lon"), dict(time=pd.DatetimeIndex(["2003-01-01"]))).disaggregate(obs, years="same")
    # the engine and the C ABI
    src_row, offsets = np.arange(4), np.array([0, 4])
    x, target = np.zeros((10, 4)), np.zeros((1, 4))
    for rows, off, msg in ((src_row, [0, 3], r"sd_disagg: offsets\[M\] = 3, expected Tout = 4"), (src_row, [1, 4], r"offsets\[0\] = 1, expected 0"),
                           ([0, 1, 10, 2], offsets, r"sd_disagg: src_row\[2\] = 10 lies outside the 10 rows of obs")):
        with pytest.raises(ValueError, match=msg):
            ctx.disaggregate(target, x, rows, off)
        with pytest.raises(ValueError, match=msg):
            ctx.disaggregate_host(target, x, rows, off)
    with pytest.raises(ValueError, match=r"sd_disagg: group\[0\] = 2 lies outside the 2 rows of climo"):
        ctx.disaggregate(target, x, src_row, offsets, "shift", np.zeros((2, 4)), [2])
    with pytest.raises(ValueError, match="sd_disagg: climo without group"):
        ctx.disaggregate(target, x, src_row, offsets, "shift", np.zeros((2, 4)))
    with pytest.raises(NotImplementedError, match="only 'shift', 'scale_mean' and 'scale_sum'"):
        ctx.disaggregate(target, x, src_row, offsets, "scale")
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape"):
        ctx.disaggregate(target, x, src_row, offsets, out=ctx.empty((3, 4)))
    with pytest.raises(ValueError, match=r"target: expected a float64 \[M, 4\] field"):
        ctx.disaggregate(np.zeros((1, 5)), x, src_row, offsets)
    from skdownscale_amd._lib import check, ptr

    d_t, d_x, d_out = ctx.to_device(target), ctx.to_device(x), ctx.empty((4, 4))
    rows, off = src_row.astype(np.int64), offsets.astype(np.int64)
    with pytest.raises(ValueError, match="sd_disagg: ld_obs = 3 is less than the 4 cells of a row"):
        check(ctx.lib.sd_disagg_dev(ctx.handle, 0, d_t.vptr, 4, d_x.vptr, 0, 3, 10, 4, ptr(rows), 4, ptr(off), 1, None, 0, 0, None, d_out.vptr, 4))
    with pytest.raises(ValueError, match="sd_disagg: unknown op code 9"):
        check(ctx.lib.sd_disagg_dev(ctx.handle, 9, d_t.vptr, 4, d_x.vptr, 0, 4, 10, 4, ptr(rows), 4, ptr(off), 1, None, 0, 0, None, d_out.vptr, 4))


def test_monthly_bcsd_end_to_end(ctx):
    """coarse.interp_like(obs).resample('MS').mean() -> PointWiseDownscaler(BcsdTemperature) -> disaggregate: the daily field is the
    oracle's on the downloaded monthly prediction"""
    from skdownscale_amd import BcsdTemperature, GridArray, PointWiseDownscaler, time_map

    rng = np.random.default_rng(31)
    T = 2922  # eight years: 96 months
    time = pd.date_range("2001-01-01", periods=T, freq="D")
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    clat, clon = np.array([42.0, 40.0, 38.0]), np.array([-110.0, -108.0, -106.0])
    fine_lat, fine_lon = np.linspace(42.0, 38.0, 6), np.linspace(-110.0, -106.0, 7)

    def coarse(shift):
        v = 285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, 3, 3)) + shift
        return GridArray(v, ("time", "lat", "lon"), dict(time=time, lat=clat, lon=clon))

    y_obs = GridArray(283.0 + season[:, None, None] + 2.0 * rng.normal(size=(T, 6, 7)), ("time", "lat", "lon"), dict(time=time, lat=fine_lat, lon=fine_lon))
    pw = PointWiseDownscaler(BcsdTemperature(return_anoms=False))
    pw.fit(coarse(0.0).interp_like(y_obs).resample(time="MS").mean(), y_obs.resample(time="MS").mean())
    monthly = pw.predict(coarse(1.5).interp_like(y_obs).resample(time="MS").mean())
    assert monthly.shape == (96, 6, 7)
    daily = monthly.disaggregate(y_obs, seed=3)
    out_time, src_row, offsets = time_map(monthly.coords["time"], time, None, 3)
    assert daily.shape == (T, 6, 7) and daily.coords["time"].equals(out_time) and out_time.equals(time)
    want = do.disaggregate(np.asarray(monthly.values).reshape(96, 42), y_obs.values.reshape(T, 42), src_row, offsets, "shift")
    same(daily.values.reshape(T, 42), want, "end to end")
    assert np.isfinite(daily.values).all()
    # the monthly mean of the daily field is the prediction (the bound of tests/_disagg_oracle.py)
    back = pd.DataFrame(daily.values.reshape(T, 42), index=out_time).resample("MS").mean().to_numpy()
    bound = do.bound(daily.values.reshape(T, 42), np.asarray(monthly.values).reshape(96, 42), y_obs.values.reshape(T, 42), src_row, offsets, "shift")
    err = np.abs(back - np.asarray(monthly.values).reshape(96, 42))
    print(f"end to end: largest err / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
