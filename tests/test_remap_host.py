"""CPU: the conservative-remapping rule and its Python surface without a GPU.

* tests/_remap_oracle.py, the definition the engine is compared with bit for bit, is pinned independently in two ways: for plain
  weights, uniform grids and an integer factor k it equals the block mean ``v.reshape(T, Ny, k, Nx, k).mean((2, 4))`` within
  ``(k^2 + 2) * 2^-53 * max|v|``; on random non-aligned grids it agrees with the dense ``Wy @ v @ Wx.T`` formulation in
  ``np.longdouble`` within ``(ky + kx + 4) * 2^-53 * sum w|v| / den``.
* ``cell_bounds`` and ``ConservativeRemapper``: inference of bounds, the area / plain / latitude choices, explicit bounds, refusals.
* ``GridArray.remap_like``: dims, coords, laziness, ``isel``, the chains into ``resample`` / ``groupby`` / ``rolling`` and block
  independence -- on an engine replaced by the oracles (tests/_oracle_engine.py), so nothing here needs the library."""
import numpy as np
import pandas as pd
import pytest

import _groupby_oracle as go
import _remap_oracle as mo
import _resample_oracle as so
import _rolling_oracle as rol
from _oracle_engine import engine  # noqa: F401  (the fixture)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- the oracle itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,Ny,Nx", [(1, 3, 4), (2, 2, 2), (4, 3, 5), (16, 2, 3)])
def test_oracle_equals_the_block_mean_on_aligned_grids(k, Ny, Nx):
    rng = np.random.default_rng(k)
    T = 3
    v = 280.0 + 15.0 * rng.normal(size=(T, Ny * k, Nx * k))
    syb, sxb = np.arange(Ny * k + 1.0), np.arange(Nx * k + 1.0)
    got = mo.remap(v, syb, sxb, syb[::k], sxb[::k], 1.0)
    want = v.reshape(T, Ny, k, Nx, k).mean((2, 4))
    err = np.abs(got - want).max()
    print(f"k={k}: max |oracle - block mean| = {err:.3e}, bound {(k * k + 2) * 2.0 ** -53 * np.abs(v).max():.3e}")
    assert np.isfinite(got).all() and err <= (k * k + 2) * 2.0 ** -53 * np.abs(v).max()
    # descending storage of either grid is the same field
    assert np.array_equal(mo.remap(v[:, ::-1], syb[::-1], sxb, syb[::k], sxb[::k], 1.0), got) or k > 1
    assert np.abs(mo.remap(v[:, ::-1], syb[::-1], sxb, syb[::k][::-1], sxb[::k], 1.0)[:, ::-1] - got).max() <= (k * k + 2) * 2.0 ** -53 * np.abs(v).max()


def dense(v, syb, sxb, dyb, dxb):
    """(num, den, mag, ky, kx) of the dense long-double formulation: W[j, k] = overlap of target j with source k"""
    def matrix(sb, db):
        first, count, w, _ = mo.axis_table(sb, db)
        W = np.zeros((len(db) - 1, len(sb) - 1), dtype=np.longdouble)
        for j in range(len(first)):
            W[j, first[j]:first[j] + count[j]] = w[j]
        return W, count

    (Wy, ky), (Wx, kx) = matrix(syb, dyb), matrix(sxb, dxb)
    val = np.where(np.isnan(v), 0.0, v).astype(np.longdouble)
    one = (~np.isnan(v)).astype(np.longdouble)
    num, den, mag = (np.einsum("jy,tyx,ix->tji", Wy, a, Wx) for a in (val, one, np.abs(val)))
    return num, den, mag, ky, kx


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_agrees_with_the_dense_long_double_formulation(seed):
    rng = np.random.default_rng(seed)
    ny, nx, Ny, Nx = 17, 23, 4, 6
    b = lambda n, lo, hi: np.concatenate([[lo], np.sort(rng.uniform(lo, hi, n - 1)), [hi]])  # noqa: E731
    syb, sxb, dyb, dxb = b(ny, 0.0, 1.0), b(nx, -2.0, 3.0)[::-1].copy(), b(Ny, -0.1, 1.1), b(Nx, -2.0, 3.0)
    v = 280.0 + 15.0 * rng.normal(size=(4, ny, nx))
    v[rng.uniform(size=v.shape) < 0.1] = np.nan
    got = mo.remap(v, syb, sxb, dyb, dxb, 0.0)
    num, den, mag, ky, kx = dense(v, syb, sxb, dyb, dxb)
    assert np.array_equal(np.isnan(got), ~(den > 0))
    ok = den > 0
    tol = ((ky[:, None] + kx[None, :] + 4) * 2.0 ** -53)[None] * mag / np.where(ok, den, 1)
    err = np.abs(got.astype(np.longdouble) - num / np.where(ok, den, 1))
    print(f"max |oracle - dense| / bound = {float((err[ok] / tol[ok]).max()):.3f}")
    assert (err[ok] <= tol[ok]).all()


def test_oracle_min_valid_partial_cover_and_empty_runs():
    v = np.array([[[1.0, np.nan], [np.nan, np.nan]]])
    g = ([0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 2.0], [0.0, 2.0])
    assert mo.remap(v, *g, 0.25)[0, 0, 0] == 1.0 and np.isnan(mo.remap(v, *g, 0.5)[0, 0, 0]) and mo.remap(v, *g, 0.0)[0, 0, 0] == 1.0
    full = np.arange(4.0).reshape(1, 2, 2)
    assert mo.remap(full, *g, 1.0)[0, 0, 0] == 1.5
    # a target twice as large as the source hull is the mean over its covered part; one wholly outside is NaN
    out = mo.remap(full, [0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 4.0, 8.0], [-2.0, 2.0], 1.0)
    assert out[0, 0, 0] == 1.5 and np.isnan(out[0, 1, 0])
    first, count, w, fullw = mo.axis_table([0.0, 1.0, 2.0], [3.0, 2.0, 1.5, -1.0])  # (a touching cell has no overlap)
    assert count.tolist() == [0, 1, 2] and first.tolist() == [0, 1, 0] and fullw.tolist() == [0.0, 0.5, 1.5] and w[2].tolist() == [1.0, 0.5]


# ---- cell_bounds and the remapper -----------------------------------------------------------------------------------------------------
def test_cell_bounds():
    from skdownscale_amd import cell_bounds

    assert np.array_equal(cell_bounds([1.0, 2.0, 4.0]), [0.5, 1.5, 3.0, 5.0])
    assert np.array_equal(cell_bounds([4.0, 2.0, 1.0]), [5.0, 3.0, 1.5, 0.5])  # in the order of the centres
    assert np.array_equal(cell_bounds([10.0, 20.0]), [5.0, 15.0, 25.0])
    c = np.linspace(-89.5, 89.5, 180)
    assert np.array_equal(cell_bounds(c), mo.cell_bounds(c)) and cell_bounds(c).dtype == np.float64
    for bad, msg in (([1.0], "has 1 centre\\(s\\): at least 2 are needed"), ([], "has 0 centre"), ([1.0, np.nan, 3.0], "contains NaN"),
                     ([1.0, 3.0, 2.0], "is not strictly monotonic"), ([1.0, 1.0], "is not strictly monotonic"), ([[1.0, 2.0]], "must be one-dimensional")):
        with pytest.raises(ValueError, match=msg):
            cell_bounds(bad, "coordinate 'lat'")


def test_remapper_measures_and_bounds():
    from skdownscale_amd import ConservativeRemapper

    src = dict(lat=np.linspace(49.5, 30.5, 20), lon=np.linspace(-119.5, -100.5, 20))
    dst = dict(lat=[35.0, 45.0], lon=[-115.0, -105.0])
    r = ConservativeRemapper(src, dst)
    assert r.dims == ("lat", "lon") and r.shape_in == (20, 20) and r.shape_out == (2, 2) and r.latitude == "lat" and r._state is None
    assert np.array_equal(r.measure("source", "lat"), mo.area_bounds(mo.cell_bounds(src["lat"])))
    assert np.array_equal(r.measure("target", "lat"), np.sin(np.deg2rad([30.0, 40.0, 50.0])))
    assert np.array_equal(r.measure("source", "lon"), mo.cell_bounds(src["lon"]))
    plain = ConservativeRemapper(src, dst, weights="plain")
    assert plain.latitude is None and np.array_equal(plain.measure("source", "lat"), mo.cell_bounds(src["lat"]))
    assert ConservativeRemapper(src, dst, latitude=None).latitude is None and ConservativeRemapper(src, dst, latitude="lon").latitude == "lon"
    named = ConservativeRemapper(dict(y=src["lat"], x=src["lon"]), dict(y=dst["lat"], x=dst["lon"]))
    assert named.latitude is None and ConservativeRemapper(dict(latitude=src["lat"], x=src["lon"]), dict(latitude=dst["lat"], x=dst["lon"])).latitude == "latitude"
    assert ConservativeRemapper(dict(y=src["lat"], x=src["lon"]), dict(y=dst["lat"], x=dst["lon"]), latitude="y").latitude == "y"
    # latitudes beyond the poles are clipped before the sine
    polar = ConservativeRemapper(dict(lat=[-88.0, -84.0], lon=[0.0, 1.0]), dict(lat=[-86.0, -80.0], lon=[0.0, 1.0]))
    assert polar.measure("source", "lat")[0] == -1.0 and polar.bounds["source"]["lat"][0] == -90.0
    # explicit bounds: for either grid by name, or through `bounds` by the length that fits; a single centre needs them
    eb = ConservativeRemapper(src, dst, dst_bounds=dict(lat=[30.0, 38.0, 50.0]), src_bounds=dict(lon=np.linspace(-120.0, -100.0, 21)))
    assert np.array_equal(eb.bounds["target"]["lat"], [30.0, 38.0, 50.0]) and np.array_equal(eb.bounds["target"]["lon"], [-120.0, -110.0, -100.0])
    assert np.array_equal(eb.bounds["source"]["lon"], np.linspace(-120.0, -100.0, 21))
    by_len = ConservativeRemapper(src, dst, bounds=dict(lat=[30.0, 38.0, 50.0]))
    assert np.array_equal(by_len.bounds["target"]["lat"], [30.0, 38.0, 50.0]) and np.array_equal(by_len.bounds["source"]["lat"], mo.cell_bounds(src["lat"]))
    one = ConservativeRemapper(src, dict(lat=[40.0], lon=[-110.0]), dst_bounds=dict(lat=[30.0, 50.0], lon=[-120.0, -100.0]))
    assert one.shape_out == (1, 1)


def test_remapper_refusals():
    from skdownscale_amd import ConservativeRemapper

    src = dict(lat=[0.0, 1.0, 2.0], lon=[5.0, 4.0, 3.0])
    dst = dict(lat=[0.5, 1.5], lon=[3.5, 4.5])
    for bad, msg in (([0.0, 2.0, 1.0], "source coordinate 'lat' is not strictly monotonic"), ([0.0, np.nan, 2.0], "source coordinate 'lat' contains NaN"),
                     ([1.0], "source coordinate 'lat' has 1 centre"), ([[0.0, 1.0]], "source coordinate 'lat' must be one-dimensional")):
        with pytest.raises(ValueError, match=msg):
            ConservativeRemapper(dict(src, lat=bad), dst)
    with pytest.raises(ValueError, match="target coordinate 'lon' contains NaN"):
        ConservativeRemapper(src, dict(dst, lon=[np.nan, 1.0]))
    with pytest.raises(ValueError, match="target coordinate 'lat' has 1 centre\\(s\\): at least 2 are needed to infer cell bounds; give explicit bounds"):
        ConservativeRemapper(src, dict(dst, lat=[0.5]))
    with pytest.raises(ValueError, match="exactly two source dims"):
        ConservativeRemapper(dict(src, z=[0.0, 1.0]), dst)
    with pytest.raises(ValueError, match="do not name the source dims"):
        ConservativeRemapper(src, dict(lat=[0.5, 1.0], x=[1.0, 2.0]))
    with pytest.raises(NotImplementedError, match="only 'area' and 'plain'"):
        ConservativeRemapper(src, dst, weights="bilinear")
    with pytest.raises(ValueError, match="latitude='y' is not one of the spatial dims"):
        ConservativeRemapper(src, dst, latitude="y")
    with pytest.raises(ValueError, match="source bounds of 'lat': expected 4 bounds for 3 cells, got shape \\(3,\\)"):
        ConservativeRemapper(src, dst, src_bounds=dict(lat=[0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="target bounds of 'lon' are not strictly monotonic"):
        ConservativeRemapper(src, dst, dst_bounds=dict(lon=[3.0, 5.0, 4.0]))
    with pytest.raises(ValueError, match="target bounds of 'lon' contain NaN"):
        ConservativeRemapper(src, dst, dst_bounds=dict(lon=[3.0, np.nan, 4.0]))
    with pytest.raises(ValueError, match="source bounds name 'z'"):
        ConservativeRemapper(src, dst, src_bounds=dict(z=[0.0, 1.0]))
    with pytest.raises(ValueError, match="bounds of 'lat' with shape \\(7,\\) fit neither the source nor the target grid"):
        ConservativeRemapper(src, dst, bounds=dict(lat=np.arange(7.0)))


# ---- GridArray.remap_like on a stand-in engine ------------------------------------------------------------------------------------------
def obs_and_gcm(T=90, dtype=np.float64):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(3)
    time = pd.date_range("2001-01-01", periods=T, freq="D")
    lat, lon = np.linspace(47.75, 32.25, 32), np.linspace(-117.7, -102.3, 45)  # descending latitude
    v = (280.0 + 10.0 * rng.normal(size=(T, 32, 45))).astype(dtype)
    v[rng.uniform(size=v.shape) < 0.05] = np.nan
    obs = GridArray(v, ("time", "lat", "lon"), dict(time=time, lat=lat, lon=lon))
    gcm = GridArray(np.zeros((4, 3, 4)), ("time", "lat", "lon"), dict(time=time[:4], lat=[35.0, 40.0, 45.0], lon=[-117.5, -112.5, -107.5, -102.5]))
    return obs, gcm


def coarse_of(obs, gcm, min_valid=0.5, area=True):
    y = (lambda c: mo.area_bounds(mo.cell_bounds(c))) if area else mo.cell_bounds
    return mo.remap(obs.values, y(obs.coords["lat"]), mo.cell_bounds(obs.coords["lon"]), y(gcm.coords["lat"]), mo.cell_bounds(gcm.coords["lon"]), min_valid)


def test_remap_like_dims_coords_laziness_and_values(engine):
    from skdownscale_amd.remap import RemappedGridArray

    obs, gcm = obs_and_gcm()
    got = obs.remap_like(gcm)
    assert isinstance(got, RemappedGridArray) and not got.computed and engine.created == 0
    assert got.dims == ("time", "lat", "lon") and got.shape == (90, 3, 4) and got.sizes == dict(time=90, lat=3, lon=4)  # gcm's time is ignored
    assert got.dtype == np.float64 and got.chunks is None and np.array_equal(got.coords["lat"], gcm.coords["lat"])
    assert got.coords["time"] is obs.coords["time"]
    want = coarse_of(obs, gcm)
    assert same_bits(got.values, want) and got.computed and got.values is got.values and engine.created == 1
    assert type(got.compute()).__name__ == "GridArray" and same_bits(got.compute().values, want)
    assert same_bits(obs.remap_like(gcm, weights="plain").values, coarse_of(obs, gcm, area=False))
    assert same_bits(obs.remap_like(gcm, latitude=None).values, coarse_of(obs, gcm, area=False))
    assert not same_bits(coarse_of(obs, gcm, area=False), want)
    assert same_bits(obs.remap_like(gcm, min_valid=1.0).values, coarse_of(obs, gcm, 1.0))
    assert np.isnan(coarse_of(obs, gcm, 1.0)).sum() > np.isnan(want).sum()  # (5 % of the fine cells are NaN)
    b = dict(lat=[32.0, 36.0, 44.0, 48.0])
    explicit = obs.remap_like(gcm, weights="plain", dst_bounds=b).values
    assert same_bits(explicit, mo.remap(obs.values, mo.cell_bounds(obs.coords["lat"]), mo.cell_bounds(obs.coords["lon"]), b["lat"],
                                        mo.cell_bounds(gcm.coords["lon"]), 0.5))


def test_other_dims_pass_through_and_float32_goes_up_as_float32(engine):
    from skdownscale_amd import GridArray

    obs, gcm = obs_and_gcm(T=6)
    want = coarse_of(obs, gcm)
    v = np.stack([obs.values, 2.0 * obs.values], axis=1)  # [time, variable, lat, lon]
    four = GridArray(v, ("time", "variable", "lat", "lon"), dict(obs.coords, variable=np.array(["a", "b"])))
    got = four.remap_like(gcm)
    assert got.dims == four.dims and got.shape == (6, 2, 3, 4) and same_bits(got.values[:, 0], want)
    with pytest.raises(ValueError, match="device_field needs dims"):
        got.device_field()
    lon_first = obs.transpose("lon", "time", "lat").remap_like(gcm)
    assert lon_first.dims == ("lon", "time", "lat") and lon_first.shape == (4, 6, 3)
    swapped = mo.remap(obs.values.transpose(0, 2, 1), mo.cell_bounds(obs.coords["lon"]), mo.area_bounds(mo.cell_bounds(obs.coords["lat"])),
                       mo.cell_bounds(gcm.coords["lon"]), mo.area_bounds(mo.cell_bounds(gcm.coords["lat"])), 0.5)
    assert same_bits(lon_first.values, swapped.transpose(1, 0, 2))
    plane = GridArray(obs.values[0], ("lat", "lon"), {k: obs.coords[k] for k in ("lat", "lon")}).remap_like(gcm)
    assert plane.dims == ("lat", "lon") and same_bits(plane.values, want[0])
    engine.uploads.clear()
    obs32, _ = obs_and_gcm(T=6, dtype=np.float32)
    f32 = obs32.remap_like(gcm)
    assert f32.dtype == np.float64 and same_bits(f32.values, coarse_of(obs32, gcm)) and engine.uploads == [(6, np.float32)]


def test_isel_stays_lazy_along_the_other_dims(engine):
    obs, gcm = obs_and_gcm(T=12)
    got = obs.remap_like(gcm)
    want = coarse_of(obs, gcm)
    sub = got.isel(time=slice(2, 7))
    assert type(sub) is type(got) and not sub.computed and not got.computed and sub.shape == (5, 3, 4)
    assert np.array_equal(sub.coords["time"], obs.coords["time"][2:7]) and same_bits(sub.values, want[2:7]) and not got.computed
    cut = got.isel(lat=slice(0, 2), time=slice(1, 3))
    assert type(cut).__name__ == "GridArray" and got.computed and same_bits(cut.values, want[1:3, 0:2])


def test_chains_equal_the_host_composition_whatever_the_blocks(engine):
    obs, gcm = obs_and_gcm(dtype=np.float32)
    from skdownscale_amd import time_bins

    coarse = coarse_of(obs, gcm).reshape(90, -1)
    _, offsets = time_bins(obs.coords["time"], "MS")
    labels, ids = np.unique(np.asarray(obs.coords["time"].month), return_inverse=True)
    want = dict(resample=so.resample(coarse, offsets, "mean").reshape(-1, 3, 4), groupby=go.reduce(coarse, ids, len(labels), "sum").reshape(-1, 3, 4),
                rolling=rol.rolling(coarse, 9, "mean", center=True, min_periods=1).reshape(-1, 3, 4))
    step = 32 * 45 * 4  # bytes of one fine float32 step
    for scratch in (None, 7 * step, 1):
        for walker_scratch in (None, 3 * 4 * 8 * 40):  # (the walkers cut the coarse field: 40 steps of 12 cells)
            engine.uploads.clear()
            kw = {} if walker_scratch is None else dict(scratch_bytes=walker_scratch)
            lazy = obs.remap_like(gcm, scratch_bytes=scratch)
            got = dict(resample=lazy.resample(time="MS", **kw).mean(), groupby=lazy.groupby("time.month", **kw).sum(),
                       rolling=lazy.rolling(time=9, center=True, min_periods=1, **kw).mean())
            for name, g in got.items():
                assert same_bits(g.values, want[name]), (name, scratch, walker_scratch)
            assert not lazy.computed  # the coarse field was produced block by block, never as a host array
            rows = max(1, (1 << 30 if scratch is None else scratch) // step)
            assert all(dtype == np.float32 and n <= rows for n, dtype in engine.uploads) and len(engine.uploads) >= 3 * -(-90 // rows)
    # a computed remap and any other combination go through the host like any GridArray
    done = obs.remap_like(gcm)
    done.values
    assert same_bits(done.resample(time="MS").mean().values, want["resample"])
    assert same_bits(obs.remap_like(gcm).transpose("lat", "time", "lon").resample(time="MS").mean().values, want["resample"].transpose(1, 0, 2))


def test_a_lazy_time_axis_result_is_taken_from_its_device_field(engine, monkeypatch):
    from skdownscale_amd import time_bins
    from skdownscale_amd.resample import ResampledGridArray

    obs, gcm = obs_and_gcm()
    _, offsets = time_bins(obs.coords["time"], "MS")
    monthly = so.resample(obs.values.reshape(90, -1), offsets, "mean").reshape(-1, 32, 45)
    lazy = obs.resample(time="MS").mean()
    monkeypatch.setattr(ResampledGridArray, "_compute_values", lambda self: pytest.fail("the monthly field went through the host"))
    got = lazy.remap_like(gcm)
    want = mo.remap(monthly, mo.area_bounds(mo.cell_bounds(obs.coords["lat"])), mo.cell_bounds(obs.coords["lon"]),
                    mo.area_bounds(mo.cell_bounds(gcm.coords["lat"])), mo.cell_bounds(gcm.coords["lon"]), 0.5)
    assert same_bits(got.values, want) and not lazy.computed and got.shape == (3, 3, 4)


def test_remap_like_refusals(engine):
    from skdownscale_amd import GridArray

    obs, gcm = obs_and_gcm(T=3)
    with pytest.raises(ValueError, match="exactly two shared spatial dims"):
        obs.remap_like(GridArray(np.zeros((2, 3)), ("time", "lat"), dict(lat=[36.0, 37.0, 38.0])))
    with pytest.raises(ValueError, match="`other` has no coordinate for dim 'lon'"):
        obs.remap_like(GridArray(np.zeros((2, 3)), ("lat", "lon"), dict(lat=[36.0, 37.0])))
    with pytest.raises(ValueError, match="the array has no coordinate for dim 'lat'"):
        GridArray(obs.values, obs.dims, dict(lon=obs.coords["lon"])).remap_like(gcm)
    for mv in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="min_valid=.*expected a share of the covered area in \\[0, 1\\]"):
            obs.remap_like(gcm, min_valid=mv)
    with pytest.raises(ValueError, match="scratch_bytes=0: expected a positive number of bytes"):
        obs.remap_like(gcm, scratch_bytes=0)
    with pytest.raises(NotImplementedError, match="only 'area' and 'plain'"):
        obs.remap_like(gcm, weights="patch")
    with pytest.raises(ValueError, match="source coordinate 'lat' is not strictly monotonic"):
        GridArray(obs.values, obs.dims, dict(obs.coords, lat=np.r_[obs.coords["lat"][1], obs.coords["lat"][0], obs.coords["lat"][2:]])).remap_like(gcm)
    with pytest.raises(ValueError, match="target coordinate 'lat' has 1 centre"):
        obs.remap_like(GridArray(np.zeros((1, 4)), ("lat", "lon"), dict(lat=[40.0], lon=gcm.coords["lon"])))
    assert engine.created == 0  # every refusal comes before any engine call


def test_package_exports_the_remapper():
    import skdownscale_amd
    from skdownscale_amd import _lib

    assert {"ConservativeRemapper", "RemappedGridArray", "cell_bounds"} <= set(skdownscale_amd.__all__) and hasattr(skdownscale_amd.GridArray, "remap_like")
    assert {"sd_remap_create", "sd_remap_destroy", "sd_remap_info", "sd_remap_apply", "sd_remap_apply_dev"} <= set(_lib.SIGNATURES)
