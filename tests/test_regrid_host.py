"""CPU: the regridding rule and its Python surface without a GPU.

* tests/_regrid_oracle.py equals scipy's interp1d applied per dimension bit for bit (NaN pattern included), on the fixture cases of
  tests/golden/g24_regrid.npz and against a live scipy where one is installed; it agrees with RegularGridInterpolator to 1e-14.
* ``Regridder`` refuses bad coordinates with its messages before any engine call.
* ``GridArray.interp_like`` / ``interp``: dims, coords, pass-through of ``time`` and ``variable``, blocks, slices -- on an engine
  replaced by the oracle (tests/_oracle_engine.py), so nothing here needs the library."""
import os

import numpy as np
import pytest

import _regrid_oracle as ro
from _oracle_engine import OracleState, engine  # noqa: F401  (engine: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g24_regrid.npz")


def golden_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in z.files})
    return {n: {k: z[f"{n}.{k}"] for k in ("src", "src_y", "src_x", "dst_y", "dst_x", "want")} | {"kind": str(z[f"{n}.kind"])} for n in names}


CASES = golden_cases()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_the_recorded_scipy_result_bit_for_bit(name):
    c = CASES[name]
    got = ro.regrid(c["src"], c["src_y"], c["src_x"], c["dst_y"], c["dst_x"], c["kind"])
    assert same_bits(got, c["want"])


def test_fixture_covers_the_edge_cases():
    assert len(CASES) == 8 and os.path.getsize(GOLDEN) < 32 * 1024
    io = CASES["inside_outside"]["want"]
    assert np.isnan(io[:, [0, -1], :]).all() and np.isnan(io[:, :, [0, -1]]).all() and np.isfinite(io[:, 1:-1, 1:-1]).all()
    nn = CASES["nan_node"]
    assert np.isfinite(nn["want"][0]).all() and np.isnan(nn["want"][1]).any() and np.isfinite(nn["want"][1]).any()
    # the NaN node is (2, 3); a target on node k >= 1 brackets k - 1 .. k, so the targets on the nodes (3, 3), (2, 4) and (3, 4) hold it
    # at weight 0 in one dimension or in both
    assert np.isnan(nn["want"][1, 3, 3]) and np.isnan(nn["want"][1, 2, 4]) and np.isnan(nn["want"][1, 3, 4])
    assert CASES["float32"]["src"].dtype == np.float32 and CASES["float32"]["want"].dtype == np.float64


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_live_scipy_interp1d_per_dimension(name):
    interp1d = pytest.importorskip("scipy.interpolate").interp1d
    c = CASES[name]
    a = interp1d(c["src_y"], c["src"], kind=c["kind"], axis=-2, bounds_error=False, fill_value=np.nan, assume_sorted=False)(c["dst_y"])
    want = interp1d(c["src_x"], a, kind=c["kind"], axis=-1, bounds_error=False, fill_value=np.nan, assume_sorted=False)(c["dst_x"])
    assert same_bits(ro.regrid(c["src"], c["src_y"], c["src_x"], c["dst_y"], c["dst_x"], c["kind"]), want)
    assert same_bits(want, c["want"])  # (the recorded result is this scipy's)


def test_oracle_agrees_with_regular_grid_interpolator():
    rgi = pytest.importorskip("scipy.interpolate").RegularGridInterpolator
    rng = np.random.default_rng(5)
    sy, sx = np.sort(rng.uniform(0, 10, 7)), np.sort(rng.uniform(0, 10, 9))
    src = rng.normal(size=(7, 9))
    dy, dx = rng.uniform(sy[0], sy[-1], 37), rng.uniform(sx[0], sx[-1], 53)
    want = rgi((sy, sx), src, method="linear")(np.stack(np.meshgrid(dy, dx, indexing="ij"), axis=-1))
    got = ro.regrid(src, sy, sx, dy, dx)
    rel = np.abs(got - want).max() / np.abs(src).max()
    print("oracle vs RegularGridInterpolator: max relative difference", rel)
    assert np.isfinite(got).all() and rel <= 1e-14


def test_np_interp_differs_only_where_a_bracket_node_is_nan():
    c = CASES["nan_node"]
    col = c["src"][1, :, 3]  # the column with the NaN node
    got = ro.interp_axis(c["src_y"], col, c["dst_y"], 0)
    ref = np.interp(c["dst_y"], c["src_y"], col)
    assert np.isnan(got[3]) and ref[3] == col[3]  # the target on node 3: weight 0 on the NaN node 2
    differ = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert differ.any() and np.isnan(got[differ]).all()


# ---- Regridder: coordinate validation ---------------------------------------------------------------------------------------------
def test_regridder_refuses_bad_coordinates():
    from skdownscale_amd import Regridder

    good = dict(lat=[0.0, 1.0, 2.0], lon=[5.0, 4.0, 3.0])
    dst = dict(lat=[0.5], lon=[3.5, 4.5])
    r = Regridder(good, dst)
    assert r.dims == ("lat", "lon") and r.shape_in == (3, 3) and r.shape_out == (1, 2) and r._state is None  # no engine call yet
    for bad, msg in (([0.0, 2.0, 1.0], "source coordinate 'lat' is not strictly monotonic"), ([0.0, 1.0, 1.0], "not strictly monotonic"),
                     ([0.0, np.nan, 2.0], "source coordinate 'lat' contains NaN"), ([1.0], "source dimension 'lat' has length 1"),
                     ([[0.0, 1.0]], "source coordinate 'lat' must be one-dimensional")):
        with pytest.raises(ValueError, match=msg):
            Regridder(dict(good, lat=bad), dst)
    with pytest.raises(ValueError, match="target coordinate 'lon' contains NaN"):
        Regridder(good, dict(dst, lon=[np.nan]))
    with pytest.raises(ValueError, match="exactly two source dims"):
        Regridder(dict(good, z=[0.0, 1.0]), dst)
    with pytest.raises(ValueError, match="do not name the source dims"):
        Regridder(good, dict(lat=[0.5], x=[1.0]))
    for method in ("cubic", "quadratic", None):
        with pytest.raises(NotImplementedError, match="only 'linear' and 'nearest'"):
            Regridder(good, dst, method=method)


# ---- GridArray.interp_like on a stand-in engine -----------------------------------------------------------------------------------
def coarse_and_obs(T=4, dtype=np.float64):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(3)
    lat, lon = np.array([40.0, 38.0, 36.0]), np.array([-110.0, -108.0, -106.0, -104.0])  # descending latitude
    coarse = GridArray(rng.normal(size=(T, 3, 4)).astype(dtype), ("time", "lat", "lon"), dict(time=np.arange(T), lat=lat, lon=lon))
    flat, flon = np.linspace(35.5, 40.0, 6), np.linspace(-110.0, -103.5, 8)  # one row and one column outside the hull
    obs = GridArray(rng.normal(size=(T + 3, 6, 8)), ("time", "lat", "lon"), dict(time=np.arange(T + 3), lat=flat, lon=flon))
    return coarse, obs


def test_interp_like_dims_coords_and_values(engine):
    from skdownscale_amd.regrid import InterpolatedGridArray

    coarse, obs = coarse_and_obs()
    fine = coarse.interp_like(obs)
    assert isinstance(fine, InterpolatedGridArray) and not fine.computed and OracleState.created == 0
    assert fine.dims == ("time", "lat", "lon") and fine.shape == (4, 6, 8) and fine.sizes == dict(time=4, lat=6, lon=8)  # obs' time is ignored
    assert fine.dtype == np.float64 and fine.chunks is None
    assert np.array_equal(fine.coords["lat"], obs.coords["lat"]) and np.array_equal(fine.coords["time"], coarse.coords["time"])
    want = ro.regrid(coarse.values, coarse.coords["lat"], coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"])
    assert same_bits(fine.values, want) and fine.computed and fine.values is fine.values
    assert np.isnan(want[:, 0, :]).all() and np.isnan(want[:, :, -1]).all() and np.isfinite(want[:, 1:, :-1]).all()
    assert same_bits(fine.compute().values, want) and type(fine.compute()).__name__ == "GridArray"
    assert same_bits(coarse.interp(lat=obs.coords["lat"], lon=obs.coords["lon"]).values, want)
    assert same_bits(coarse.interp({"lat": obs.coords["lat"]}, lon=obs.coords["lon"], method="nearest").values,
                     ro.regrid(coarse.values, coarse.coords["lat"], coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"], "nearest"))


def test_time_variable_and_dim_order_pass_through(engine):
    from skdownscale_amd import GridArray

    coarse, obs = coarse_and_obs()
    want = ro.regrid(coarse.values, coarse.coords["lat"], coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"])
    # a feature dim and the spatial dims in front of time: dims keep their order, the first spatial dim of the field goes first
    v = np.stack([coarse.values, 2.0 * coarse.values], axis=1)  # [time, variable, lat, lon]
    four = GridArray(v, ("time", "variable", "lat", "lon"), dict(coarse.coords, variable=np.array(["a", "b"])))
    got = four.interp_like(obs)
    assert got.dims == four.dims and got.shape == (4, 2, 6, 8)
    assert same_bits(got.values[:, 0], want) and same_bits(got.values[:, 1], ro.regrid(2.0 * coarse.values, coarse.coords["lat"],
                                                                                    coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"]))
    lon_first = coarse.transpose("lon", "time", "lat")
    swapped = lon_first.interp_like(obs)
    assert swapped.dims == ("lon", "time", "lat") and swapped.shape == (8, 4, 6)
    lonlat = ro.regrid(coarse.values.transpose(0, 2, 1), coarse.coords["lon"], coarse.coords["lat"], obs.coords["lon"], obs.coords["lat"])
    assert same_bits(swapped.values, lonlat.transpose(1, 0, 2))
    plane = coarse.isel(time=slice(0, 1))
    flat2 = GridArray(plane.values[0], ("lat", "lon"), {k: plane.coords[k] for k in ("lat", "lon")}).interp_like(obs)
    assert flat2.dims == ("lat", "lon") and same_bits(flat2.values, want[0])
    f32 = GridArray(coarse.values.astype(np.float32), coarse.dims, coarse.coords).interp_like(obs)
    assert f32.dtype == np.float64 and same_bits(f32.values, ro.regrid(coarse.values.astype(np.float32).astype(np.float64), coarse.coords["lat"],
                                                                      coarse.coords["lon"], obs.coords["lat"], obs.coords["lon"]))


def test_isel_and_chunk_work_on_the_target_grid(engine):
    coarse, obs = coarse_and_obs()
    fine = coarse.interp_like(obs)
    want = fine.values
    sub = fine.isel(lat=slice(1, 4), lon=slice(2, 8), time=slice(1, 3))
    assert type(sub) is type(fine) and sub.shape == (2, 3, 6) and not sub.computed
    assert np.array_equal(sub.coords["lat"], obs.coords["lat"][1:4]) and np.array_equal(sub.coords["time"], [1, 2])
    assert same_bits(sub.values, want[1:3, 1:4, 2:8])
    blocked = coarse.interp_like(obs).chunk({"lat": 3, "lon": 4})
    assert blocked.chunksizes == dict(time=(4,), lat=(3, 3), lon=(4, 4)) and blocked.chunks == ((4,), (3, 3), (4, 4))
    before = OracleState.created
    assert same_bits(blocked.values, want) and OracleState.created == before + 4  # one plan per block
    with pytest.raises(ValueError, match="per block"):
        blocked.device_field()
    assert blocked.unchunked().chunks is None and same_bits(blocked.unchunked().device_field().to_host().reshape(4, 6, 8), want)


def test_interp_like_refusals(engine):
    from skdownscale_amd import GridArray

    coarse, obs = coarse_and_obs()
    with pytest.raises(ValueError, match="exactly two shared spatial dims"):
        coarse.interp_like(GridArray(np.zeros((2, 3)), ("time", "lat"), dict(lat=[36.0, 37.0, 38.0])))
    with pytest.raises(ValueError, match="`other` has no coordinate for dim 'lon'"):
        coarse.interp_like(GridArray(np.zeros((2, 3)), ("lat", "lon"), dict(lat=[36.0, 37.0])))
    with pytest.raises(ValueError, match="the array has no coordinate for dim 'lat'"):
        GridArray(coarse.values, coarse.dims, dict(lon=coarse.coords["lon"])).interp_like(obs)
    with pytest.raises(ValueError, match="'x' is not a dim"):
        coarse.interp(x=[1.0], lat=[37.0])
    with pytest.raises(NotImplementedError, match="only 'linear' and 'nearest'"):
        coarse.interp_like(obs, method="cubic")
    with pytest.raises(ValueError, match="source coordinate 'lat' is not strictly monotonic"):
        GridArray(coarse.values, coarse.dims, dict(coarse.coords, lat=[40.0, 36.0, 38.0])).interp_like(obs)
    four = GridArray(coarse.values[:, None], ("time", "variable", "lat", "lon"), coarse.coords).interp_like(obs)
    with pytest.raises(ValueError, match="device_field needs dims"):
        four.device_field()


def test_package_exports_the_regridder():
    import skdownscale_amd
    from skdownscale_amd import _lib

    assert "Regridder" in skdownscale_amd.__all__ and hasattr(skdownscale_amd.GridArray, "interp_like")
    assert {"sd_regrid_create", "sd_regrid_destroy", "sd_regrid_info", "sd_regrid_apply", "sd_regrid_apply_dev"} <= set(_lib.SIGNATURES)
