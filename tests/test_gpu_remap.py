"""GPU: remap_kernel (csrc/sd_remap.hip) through Context.remap_create and GridArray.remap_like against tests/_remap_oracle.py.

Every value check is bit-exact, NaN positions included: the oracle restates the sums of the kernel in their order, every product
rounded on its own (tests/test_remap_host.py pins the oracle itself against a block mean and a long-double dense formulation).  Only
the conservation check has a tolerance, (ny + nx + 4) * 2^-53 * sum w|v|: the two sides associate the same products differently."""
import math

import numpy as np
import pytest

import _groupby_oracle as go
import _remap_oracle as mo
import _resample_oracle as so

pytestmark = pytest.mark.gpu

CHUNK, LANES = 64, 64  # time steps of a workgroup, source columns of a strip per column of a lane (pinned by tests/test_remap_plan.py)
STEPS = [1, 5, CHUNK - 1, CHUNK, CHUNK + 1]
# (3, 600) -> (2, 1): one target column wider than a strip also with two (float64) and four (float32) columns per lane
SHAPES = [((2, 2), (1, 1)), ((7, 9), (3, 4)), ((16, 130), (4, 13)), ((5, 257), (2, 3)), ((3, 700), (1, 66)), ((9, 9), (12, 11)), ((3, 600), (2, 1))]


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    ok = np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))
    if not ok:
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        print(f"{what}: {len(bad)} of {got.size} differ, first at {bad[:3].tolist()}, max |diff| {np.nanmax(np.abs(got - want)):.3e}")
    assert ok, what


def bounds(rng, n, lo, hi):
    """n cells of random widths that fill [lo, hi]"""
    return np.concatenate([[lo], np.sort(rng.uniform(lo, hi, n - 1)), [hi]])


def field(rng, T, ny, nx, nan=0.05, dtype=np.float64):
    v = 280.0 + 15.0 * rng.normal(size=(T, ny, nx))
    v[rng.uniform(size=v.shape) < nan] = np.nan
    return v.astype(dtype)


@pytest.mark.parametrize("src,dst", SHAPES)
def test_shape_sweep(ctx, src, dst):
    (ny, nx), (Ny, Nx) = src, dst
    rng = np.random.default_rng(1000 * ny + nx)
    syb, sxb = bounds(rng, ny, 30.0, 50.0), bounds(rng, nx, -120.0, -100.0)
    dyb, dxb = bounds(rng, Ny, 30.0, 50.0), bounds(rng, Nx, -120.0, -100.0)
    _, ky, _, _ = mo.axis_table(syb, dyb)
    _, kx, _, _ = mo.axis_table(sxb, dxb)
    if src == (5, 257):
        assert nx % 2 == 1 and kx.max() > LANES  # one column per lane: a single target column wider than the strip of 64
    if src == (3, 600):
        assert kx.max() > 4 * LANES  # wider than the strip at four columns per lane
    if src == (3, 700):
        assert Nx > 64  # more target columns than a wave has lanes, several tiles
    state = ctx.remap_create(syb, sxb, dyb, dxb)
    assert state.info() == dict(ny=ny, nx=nx, Ny=Ny, Nx=Nx, y_entries=int(ky.sum()), x_entries=int(kx.sum()))
    for T in STEPS:
        for dtype in (np.float64, np.float32):
            v = field(rng, T, ny, nx, dtype=dtype)
            want = mo.remap(v, syb, sxb, dyb, dxb, 0.5).reshape(T, -1)
            same(state.apply(v, 0.5).to_host(), want, f"{src}->{dst} T={T} {np.dtype(dtype).name}")
    v = field(rng, 5, ny, nx, nan=0.4)
    for mv in (0.0, 0.25, 1.0):
        same(state.apply(v, mv).to_host(), mo.remap(v, syb, sxb, dyb, dxb, mv).reshape(5, -1), f"{src}->{dst} min_valid={mv}")
    state.close()


def test_descending_latitude_and_a_target_beyond_the_hull(ctx):
    rng = np.random.default_rng(2)
    syb, sxb = bounds(rng, 9, 30.0, 50.0)[::-1].copy(), bounds(rng, 140, -120.0, -100.0)
    dyb, dxb = bounds(rng, 5, 25.0, 55.0), bounds(rng, 70, -125.0, -95.0)[::-1].copy()  # beyond the hull on every side, x descending
    v = field(rng, 7, 9, 140)
    for mv in (0.0, 0.5, 1.0):
        got = ctx.remap_create(syb, sxb, dyb, dxb).apply(v, mv).to_host()
        same(got, mo.remap(v, syb, sxb, dyb, dxb, mv).reshape(7, -1), f"beyond the hull, min_valid={mv}")
    got = got.reshape(7, 5, 70)
    _, ky, _, _ = mo.axis_table(syb, dyb)
    _, kx, _, _ = mo.axis_table(sxb, dxb)
    assert (ky == 0).any() and (kx == 0).any() and np.isnan(got[:, ky == 0, :]).all() and np.isnan(got[:, :, kx == 0]).all()
    # a partly covered cell is the mean over its covered part
    part = ctx.remap_create(syb, sxb, dyb, dxb).apply(np.ones_like(v), 0.0).to_host().reshape(7, 5, 70)
    assert (part[:, ky > 0][:, :, kx > 0] == 1.0).all()  # (num and den are the same sums)
    # the same field stored the other way round is the same field within rounding (the order of the sums differs)
    a = ctx.remap_create(syb[::-1].copy(), sxb, dyb, dxb).apply(v[:, ::-1, :].copy(), 0.5).to_host()
    b = ctx.remap_create(syb, sxb, dyb, dxb).apply(v, 0.5).to_host()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) <= 1e-12 * 300.0


def test_min_valid_at_its_edge(ctx):
    state = ctx.remap_create([0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 2.0], [0.0, 2.0])  # a 2 x 2 block onto one cell, weights 1
    nan = np.nan
    blocks = np.array([[[3.0, nan], [nan, 5.0]], [[3.0, nan], [nan, nan]], [[1.0, 2.0], [3.0, 4.5]], [[nan, nan], [nan, 7.25]],
                       [[nan, nan], [nan, nan]]])
    half = state.apply(blocks, 0.5).to_host()[:, 0]
    assert half[0] == 4.0 and np.isnan(half[1]) and half[2] == 10.5 / 4.0 and np.isnan(half[3]) and np.isnan(half[4])
    full = state.apply(blocks, 1.0).to_host()[:, 0]
    assert np.isnan(full[[0, 1, 3, 4]]).all() and full[2] == 10.5 / 4.0  # all four valid pass at min_valid = 1
    any_ = state.apply(blocks, 0.0).to_host()[:, 0]
    assert any_[3] == 7.25 and any_[1] == 3.0 and np.isnan(any_[4])  # one valid cell gives that cell; none gives NaN
    for mv in (0.0, 0.5, 1.0):
        same(state.apply(blocks, mv).to_host(), mo.remap(blocks, [0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 2.0], [0.0, 2.0], mv).reshape(5, -1))
    # fully covered and fully valid cells pass at 1.0 on uneven grids too (the 2^-30 slack)
    rng = np.random.default_rng(3)
    syb, sxb, dyb, dxb = bounds(rng, 37, 0.0, 1.0), bounds(rng, 131, 0.0, 3.0), bounds(rng, 5, 0.0, 1.0), bounds(rng, 7, 0.0, 3.0)
    v = field(rng, 3, 37, 131, nan=0.0)
    got = ctx.remap_create(syb, sxb, dyb, dxb).apply(v, 1.0).to_host()
    assert np.isfinite(got).all()
    same(got, mo.remap(v, syb, sxb, dyb, dxb, 1.0).reshape(3, -1))


def test_all_nan_inf_and_float32(ctx):
    rng = np.random.default_rng(4)
    syb, sxb, dyb, dxb = bounds(rng, 16, 30.0, 50.0), bounds(rng, 130, -120.0, -100.0), bounds(rng, 4, 30.0, 50.0), bounds(rng, 13, -120.0, -100.0)
    fy, ky, _, _ = mo.axis_table(syb, dyb)
    fx, kx, _, _ = mo.axis_table(sxb, dxb)
    v = field(rng, 6, 16, 130, nan=0.02)
    v[1, fy[1]:fy[1] + ky[1], fx[2]:fx[2] + kx[2]] = np.nan  # everything under target (1, 2)
    v[2, 3, 7], v[3, 3, 7], v[3, 3, 8] = np.inf, np.inf, -np.inf
    v[4, 9, 100] = -np.inf
    v[5] = np.nan
    state = ctx.remap_create(syb, sxb, dyb, dxb)
    for mv in (0.0, 0.5):
        got = state.apply(v, mv).to_host()
        same(got, mo.remap(v, syb, sxb, dyb, dxb, mv).reshape(6, -1), f"nan / inf, min_valid={mv}")
    got = got.reshape(6, 4, 13)
    assert np.isnan(got[1, 1, 2]) and np.isnan(got[5]).all() and np.isposinf(got[2]).sum() >= 1 and np.isneginf(got[4]).sum() >= 1
    v32 = field(rng, CHUNK + 1, 16, 130, dtype=np.float32)
    got32 = state.apply(v32, 0.5).to_host()
    same(got32, state.apply(v32.astype(np.float64), 0.5).to_host(), "float32 equals the widened source")
    same(got32, state.apply(ctx.to_device(v32.reshape(CHUNK + 1, -1), np.float32), 0.5).to_host(), "resident float32")
    same(got32, mo.remap(v32, syb, sxb, dyb, dxb, 0.5).reshape(CHUNK + 1, -1))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_padded_fields_unaligned_pointers_and_the_host_twin(ctx, dtype):
    rng = np.random.default_rng(5)
    ny, nx, Ny, Nx, T = 6, 132, 3, 10, CHUNK + 1
    syb, sxb, dyb, dxb = bounds(rng, ny, 0.0, 1.0), bounds(rng, nx, 0.0, 2.0), bounds(rng, Ny, 0.0, 1.0), bounds(rng, Nx, 0.0, 2.0)
    v = field(rng, T, ny, nx, dtype=dtype)
    want = mo.remap(v, syb, sxb, dyb, dxb, 0.5).reshape(T, -1)
    state = ctx.remap_create(syb, sxb, dyb, dxb)
    same(state.apply(v, 0.5).to_host(), want, "plain")
    same(state.apply_host(v, 0.5), want, "sd_remap_apply equals sd_remap_apply_dev")
    same(ctx.remap_host(v, syb, sxb, dyb, dxb, 0.5), want, "remap_host")
    cells, C = ny * nx, Ny * Nx
    # (source offset, source pitch, output offset, output pitch): aligned wide loads, a pitch that allows only pairs, odd offsets and
    # pitches (one column per lane; an output pointer that is only 8-byte aligned)
    for s_off, s_pitch, o_off, o_pitch in ((4, cells + 8, 2, C + 4), (2, cells + 6, 1, C + 3), (1, cells + 3, 3, C + 5), (3, cells + 5, 0, C)):
        parent = np.full((T, s_pitch), -1.0, dtype=dtype)
        parent[:, s_off:s_off + cells] = v.reshape(T, cells)
        src = ctx.to_device(parent, dtype).cells(s_off, s_off + cells)
        out_parent = ctx.to_device(np.full((T, o_pitch), 7.0))
        out = state.apply(src, 0.5, out=out_parent.cells(o_off, o_off + C))
        assert src.ld == s_pitch and out.ld == o_pitch
        same(out.to_host(), want, f"offsets {s_off}, {o_off}, pitches {s_pitch}, {o_pitch}")
        back = out_parent.to_host()
        assert (back[:, :o_off] == 7.0).all() and (back[:, o_off + C:] == 7.0).all()  # the padding is untouched


def test_conservation(ctx):
    rng = np.random.default_rng(6)
    ny, nx, Ny, Nx, T = 16, 130, 4, 13, 3
    syb, sxb, dyb, dxb = bounds(rng, ny, 30.0, 50.0), bounds(rng, nx, -120.0, -100.0), bounds(rng, Ny, 30.0, 50.0), bounds(rng, Nx, -120.0, -100.0)
    v = 5.0 * rng.normal(size=(T, ny, nx))  # no NaN, coinciding hulls
    out = ctx.remap_create(syb, sxb, dyb, dxb).apply(v, 1.0).to_host().reshape(T, Ny, Nx)
    _, _, _, fully = mo.axis_table(syb, dyb)
    _, _, _, fullx = mo.axis_table(sxb, dxb)
    wy, wx = np.abs(np.diff(syb)), np.abs(np.diff(sxb))
    for t in range(T):
        dst = math.fsum((fully[:, None] * fullx[None, :] * out[t]).ravel())
        src = math.fsum((wy[:, None] * wx[None, :] * v[t]).ravel())
        tol = (ny + nx + 4) * 2.0 ** -53 * math.fsum((wy[:, None] * wx[None, :] * np.abs(v[t])).ravel())
        print(f"conservation t={t}: |dst - src| = {abs(dst - src):.3e}, bound {tol:.3e}")
        assert abs(dst - src) <= tol


# ---- the chains: obs.remap_like(gcm) feeding the time-axis reductions, and fed by one ------------------------------------------------
@pytest.fixture(scope="module")
def chain_case():
    import pandas as pd

    from skdownscale_amd import GridArray

    rng = np.random.default_rng(7)
    T = 120
    time = pd.date_range("2001-01-01", periods=T, freq="D")
    lat, lon = np.linspace(49.75, 30.25, 40), np.linspace(-119.75, -100.25, 66)  # descending latitude
    v = (283.0 + 10.0 * np.sin(np.arange(T) / 58.0)[:, None, None] + 2.0 * rng.normal(size=(T, 40, 66))).astype(np.float32)
    v[rng.uniform(size=v.shape) < 0.03] = np.nan
    obs = GridArray(v, ("time", "lat", "lon"), dict(time=time, lat=lat, lon=lon))
    glat, glon = np.array([32.5, 37.5, 42.5, 47.5]), np.array([-117.5, -112.5, -107.5, -102.5, -97.5])  # the last column outside the hull, the one before partly
    gcm = GridArray(np.zeros((2, 4, 5)), ("time", "lat", "lon"), dict(time=time[:2], lat=glat, lon=glon))
    b = dict(syb=mo.area_bounds(mo.cell_bounds(lat)), sxb=mo.cell_bounds(lon), dyb=mo.area_bounds(mo.cell_bounds(glat)), dxb=mo.cell_bounds(glon))
    coarse = mo.remap(v, b["syb"], b["sxb"], b["dyb"], b["dxb"], 0.5)
    return obs, gcm, b, coarse


def test_remap_like_values_and_block_independence(ctx, chain_case):
    obs, gcm, b, coarse = chain_case
    for scratch in (None, 3 * 40 * 66 * 4, 1):  # one block, blocks of three steps, a step at a time
        got = obs.remap_like(gcm, scratch_bytes=scratch)
        assert not got.computed and got.shape == (120, 4, 5) and got.dtype == np.float64
        same(got.values, coarse, f"remap_like scratch_bytes={scratch}")
    same(obs.remap_like(gcm).isel(time=slice(10, 20)).values, coarse[10:20], "isel stays lazy")


def test_chains_into_resample_and_groupby(ctx, chain_case):
    from skdownscale_amd import time_bins

    obs, gcm, b, coarse = chain_case
    _, offsets = time_bins(obs.coords["time"], "MS")
    month = np.asarray(obs.coords["time"].month)
    labels, ids = np.unique(month, return_inverse=True)
    want_ms = so.resample(coarse.reshape(120, -1), offsets, "mean").reshape(-1, 4, 5)
    want_gb = go.reduce(coarse.reshape(120, -1), ids, len(labels), "mean").reshape(-1, 4, 5)
    for scratch in (None, 7 * 40 * 66 * 4):
        same(obs.remap_like(gcm, scratch_bytes=scratch).resample(time="MS").mean().values, want_ms, f"resample, scratch_bytes={scratch}")
        same(obs.remap_like(gcm, scratch_bytes=scratch).groupby("time.month").mean().values, want_gb, f"groupby, scratch_bytes={scratch}")
    # small scratch on the walker's side as well: blocks of whole bins of the coarse field
    same(obs.remap_like(gcm, scratch_bytes=5 * 40 * 66 * 4).resample(time="MS", scratch_bytes=40 * 20 * 8).mean().values, want_ms, "both small")


def test_a_lazy_monthly_field_is_remapped_in_hbm(ctx, chain_case, monkeypatch):
    from skdownscale_amd import time_bins
    from skdownscale_amd.resample import ResampledGridArray

    obs, gcm, b, coarse = chain_case
    _, offsets = time_bins(obs.coords["time"], "MS")
    monthly = so.resample(obs.values.reshape(120, -1), offsets, "mean").reshape(-1, 40, 66)
    want = mo.remap(monthly, b["syb"], b["sxb"], b["dyb"], b["dxb"], 0.5)
    lazy = obs.resample(time="MS").mean()
    monkeypatch.setattr(ResampledGridArray, "_compute_values", lambda self: pytest.fail("the monthly field went through the host"))
    got = lazy.remap_like(gcm)
    same(got.values, want, "lazy monthly source")
    assert not lazy.computed


def test_errors(ctx):
    with pytest.raises(ValueError, match="non-monotonic or duplicated source bounds of 'y'"):
        ctx.remap_create([0.0, 2.0, 1.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="non-monotonic or duplicated target bounds of 'x'"):
        ctx.remap_create([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [0.0, 0.0])
    with pytest.raises(ValueError, match="NaN in the source bounds of 'x'"):
        ctx.remap_create([0.0, 1.0], [0.0, np.nan], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="NaN in the target bounds of 'y'"):
        ctx.remap_create([0.0, 1.0], [0.0, 1.0], [np.nan, 1.0], [0.0, 1.0])
    for bad in ([0.0], [], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="src_yb: expected the n \\+ 1 bounds"):
            ctx.remap_create(bad, [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    state = ctx.remap_create([0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], [0.0, 3.0], [0.0, 1.0, 2.0])
    for bad in (np.zeros((2, 2, 3)), np.zeros((3, 2)), np.zeros((0, 3, 2)), np.zeros((2, 7))):
        with pytest.raises(ValueError, match="field: expected a float32 or float64"):
            state.apply(bad)
    for mv in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="min_valid"):
            state.apply(np.zeros((2, 3, 2)), mv)
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray"):
        state.apply(np.zeros((2, 3, 2)), out=ctx.empty((2, 3)))
    with pytest.raises(ValueError, match="apply_host: expected a host array"):
        state.apply_host(ctx.to_device(np.zeros((2, 6))))
    assert state.apply(np.zeros((2, 6))).shape == (2, 2)  # [T, ny * nx] is taken as well
    state.close()
    state.close()
    with pytest.raises(ValueError, match="state has been destroyed"):
        state.apply(np.zeros((2, 3, 2)))
