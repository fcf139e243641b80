"""CPU, no engine: the host side of GridArray.resample (skdownscale_amd/resample.py) -- pandas' bins as an offsets table, the lazy
surface, the refusals -- and the NumPy oracle (tests/_resample_oracle.py) against what pandas made of the golden cases
(tests/golden/g25_resample.npz, written by tests/golden/make_golden_resample.py with pandas 2.3.3).

Tolerance (derived, tests/_resample_oracle.py: bound): for a bin with n non-NaN samples plain and compensated float64 summation both
stay within n * 2^-53 * sum|x_i| of the exact sum, so |got - want| <= (n + 2) * 2^-53 * sum|x_i| for ``sum``; the same divided by n plus
one ulp of the result for ``mean``.  NaN and 0.0 patterns of bins without a sample must match exactly."""
import os

import numpy as np
import pandas as pd
import pytest

import _resample_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["ms_gap", "me", "ys", "7d", "1d_subdaily", "nan_run_and_all_nan_bin", "float32"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g25_resample.npz"))
    return {name: {k: g[f"{name}.{k}"] for k in ("time", "values", "rule", "labels", "size", "mean", "sum")} for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_time_bins_are_pandas_sizes_and_labels(golden, name):
    from skdownscale_amd.resample import time_bins

    c = golden[name]
    rule = str(c["rule"])
    labels, offsets = time_bins(c["time"], rule)
    assert offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(c["time"])
    assert np.array_equal(np.diff(offsets), c["size"]) and np.array_equal(np.asarray(labels), c["labels"])
    live = pd.Series(0, index=pd.DatetimeIndex(c["time"])).resample(rule).size()  # the installed pandas agrees with the golden file
    assert np.array_equal(live.to_numpy(), c["size"]) and np.array_equal(live.index.values, c["labels"])
    assert np.array_equal(time_bins(pd.DatetimeIndex(c["time"]), rule)[1], offsets)  # an Index or an array of datetime64


def test_the_gap_case_has_two_empty_bins(golden):
    c = golden["ms_gap"]
    assert len(c["time"]) == 330 and len(c["size"]) == 14 and (c["size"] == 0).sum() == 2
    empty = c["size"] == 0
    assert np.isnan(c["mean"][empty]).all() and (c["sum"][empty] == 0.0).all() and np.isfinite(c["mean"][~empty]).all()


def test_time_bins_pass_keywords_to_pandas():
    from skdownscale_amd.resample import time_bins

    time = pd.date_range("2001-01-01", periods=50, freq="D")
    for rule, kw in (("7D", dict(closed="right", label="right")), ("7D", dict(offset="2D")), ("10D", dict(origin="2000-12-28")),
                     ("MS", dict(closed="right"))):
        want = pd.Series(0, index=time).resample(rule, **kw).size()
        labels, offsets = time_bins(time, rule, **kw)
        assert np.array_equal(np.diff(offsets), want.to_numpy()) and labels.equals(want.index), (rule, kw)
    repeated = time.repeat(2)  # monotonic non-decreasing: duplicates are fine
    assert np.array_equal(np.diff(time_bins(repeated, "7D")[1]), 2 * np.diff(time_bins(time, "7D")[1]))


def test_unsorted_time_names_the_first_offending_position():
    from skdownscale_amd import GridArray
    from skdownscale_amd.resample import time_bins

    time = pd.date_range("2001-01-01", periods=20, freq="D").values.copy()
    time[[7, 8]] = time[[8, 7]]
    time[15] = time[2]
    with pytest.raises(ValueError, match=r"not monotonic non-decreasing: position 8 \(2001-01-08"):
        time_bins(time, "7D")
    with pytest.raises(ValueError, match="position 8"):
        GridArray(np.zeros((20, 2)), ("time", "x"), dict(time=time)).resample(time="7D")


def test_pandas_own_errors_come_through():
    from skdownscale_amd.resample import time_bins

    with pytest.raises(TypeError, match="Only valid with DatetimeIndex"):
        time_bins(np.arange(10), "7D")
    with pytest.raises(ValueError, match="Invalid frequency"):
        time_bins(pd.date_range("2001-01-01", periods=10, freq="D"), "fortnight")


def test_the_lazy_surface_and_its_refusals():
    from skdownscale_amd import GridArray, ResampledGridArray

    time = pd.date_range("2001-01-17", periods=100, freq="D")
    a = GridArray(np.zeros((100, 3, 4), dtype=np.float32), ("time", "lat", "lon"), dict(time=time, lat=np.arange(3.0), lon=np.arange(4.0)))
    r = a.resample(time="MS")
    for other in ("max", "min", "median", "std", "count"):
        with pytest.raises(NotImplementedError, match=rf"{other}\(\): only mean\(\) and sum\(\)"):
            getattr(r, other)()
    with pytest.raises(AttributeError):
        r.no_such_thing
    m = r.mean()
    assert isinstance(m, ResampledGridArray) and isinstance(m, GridArray) and not m.computed
    assert m.dims == a.dims and m.shape == (4, 3, 4) and m.sizes == dict(time=4, lat=3, lon=4) and m.dtype == np.float64
    assert list(m.coords["time"]) == list(pd.date_range("2001-01-01", periods=4, freq="MS")) and m.coords["lat"] is a.coords["lat"]
    assert np.array_equal(m.offsets, [0, 15, 43, 74, 100])
    sub = m.isel(lat=slice(1, 3))  # a spatial selection stays lazy and selects from the source
    assert isinstance(sub, ResampledGridArray) and sub.shape == (4, 2, 4) and sub.source.shape == (100, 2, 4) and not sub.computed
    ch = m.chunk({"lat": 2, "lon": -1})
    assert ch.chunks == ((4,), (2, 1), (4,)) and ch.unchunked().chunksizes is None and m.unchunked() is m
    assert a.resample({"time": "MS"}).sum().shape == (4, 3, 4)
    for bad, msg in ((dict(), "exactly one dim=rule"), (dict(time="MS", lat="MS"), "exactly one dim=rule"), (dict(when="MS"), "exactly one dim=rule")):
        with pytest.raises((ValueError, TypeError), match=msg):
            a.resample(**bad)
    with pytest.raises(ValueError, match="no coordinate for dim 'time'"):
        GridArray(np.zeros((5, 2)), ("time", "x")).resample(time="MS")
    lazy = a.interp_like(GridArray(np.zeros((2, 3)), ("lat", "lon"), dict(lat=[0.5, 1.5], lon=[0.5, 1.5, 2.5]))).resample(time="MS").mean()
    assert lazy.shape == (4, 2, 3) and not lazy.computed and not lazy.source.computed  # InterpolatedGridArray inherits resample


@pytest.mark.parametrize("op", ["mean", "sum"])
@pytest.mark.parametrize("name", CASES)
def test_oracle_against_pandas(golden, name, op):
    c = golden[name]
    offsets = np.concatenate([[0], np.cumsum(c["size"])])
    got = so.resample(c["values"], offsets, op)
    ratio = so.check(got, c[op], c["values"], offsets, op, f"{name} {op}")
    assert ratio <= 1.0
    if name == "nan_run_and_all_nan_bin":
        assert np.isnan(c["mean"][1, 1]) and c["sum"][1, 1] == 0.0 and np.isfinite(c["mean"][0, 0])  # all-NaN bin / NaN run inside a bin
