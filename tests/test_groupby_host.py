"""CPU, no engine: the host side of GridArray.groupby (skdownscale_amd/groupby.py) -- the labels, the lazy surface of both arrays, the
refusals, the matching of ``other`` by label -- and the NumPy oracle (tests/_groupby_oracle.py) against what pandas and the reference
made of the golden cases (tests/golden/g26_groupby.npz, written by tests/golden/make_golden_groupby.py with pandas 2.3.3).

Tolerance (derived, tests/_groupby_oracle.py: bound, that of tests/_resample_oracle.py): for a group with n non-NaN samples plain and
compensated float64 summation both stay within n * 2^-53 * sum|x_i| of the exact sum, so |got - want| <= (n + 2) * 2^-53 * sum|x_i| for
``sum``; the same divided by n plus one ulp for ``mean``.  NaN and 0.0 patterns of groups without a sample must match exactly."""
import os

import numpy as np
import pandas as pd
import pytest

import _groupby_oracle as go

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("month", "dayofyear", "year", "season", "month_grouper")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g26_groupby.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def daily(golden):
    from skdownscale_amd import GridArray

    return GridArray(golden["values"], ("time", "cell"), {"time": pd.DatetimeIndex(golden["time"]), "cell": np.arange(6)}, name="tas")


def groupby_of(a, key):
    from skdownscale_amd import MONTH_GROUPER

    return a.groupby(time=MONTH_GROUPER, name="month") if key == "month_grouper" else a.groupby("time." + key)


def test_the_golden_cases_are_what_the_issue_describes(golden):
    time = pd.DatetimeIndex(golden["time"])
    assert len(time) == 1096 and golden["values"].shape == (1096, 6) and time.is_leap_year.any()
    assert 0.03 < np.isnan(golden["values"][:, :5]).mean() < 0.07 and golden["values32"].dtype == np.float32
    assert len(golden["f64.dayofyear.labels"]) == 366 and (time.dayofyear == 366).sum() == 1
    assert np.isnan(golden["f64.month.mean"][1, 5]) and golden["f64.month.sum"][1, 5] == 0.0  # the all-NaN group
    assert list(golden["f64.season.labels"]) == ["DJF", "JJA", "MAM", "SON"]
    assert golden["ref.y_climo"].shape == (12, 4) and golden["ref.x_climo"].shape == (12, 4) and golden["ref.anoms"].shape == (730, 4)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["f64", "f32"])
def test_labels_and_oracle_against_pandas(golden, daily, name, key):
    gb = groupby_of(daily, key)
    assert np.array_equal(gb.labels, golden[f"{name}.{key}.labels"]) and gb.group.dtype == np.int32 and gb.group.shape == (1096,)
    assert np.array_equal(gb.labels[gb.group], np.asarray(golden[f"{name}.{key}.labels"])[gb.group])
    values = golden["values" if name == "f64" else "values32"]
    live = pd.DataFrame(values.astype(np.float64), index=pd.DatetimeIndex(golden["time"])).groupby(gb.labels[gb.group])
    G = len(gb.labels)
    for op in ("mean", "sum"):
        got = go.reduce(values, gb.group, G, op)
        go.check(got, golden[f"{name}.{key}.{op}"], values, gb.group, G, op, f"{name} {key} {op} vs golden")
        go.check(got, getattr(live, op)().to_numpy(), values, gb.group, G, op, f"{name} {key} {op} vs the installed pandas")


def test_oracle_against_the_reference(golden):
    month = (pd.DatetimeIndex(golden["ref.time"]).month - 1).to_numpy()
    for field, want in (("ref.y", "ref.y_climo"), ("ref.X", "ref.x_climo")):
        go.check(go.reduce(golden[field], month, 12), golden[want], golden[field], month, 12, "mean", want)
    # _remove_climatology is one subtraction of the reference's own climatology: exact
    assert np.array_equal(go.apply(golden["ref.X"], month, golden["ref.x_climo"], "sub"), golden["ref.anoms"])


def test_the_oracle_carries_and_does_not_depend_on_the_cut(golden):
    v, g = golden["values"], (pd.DatetimeIndex(golden["time"]).month - 1).to_numpy()
    whole = go.accumulate(v, g, 12)
    for cuts in ([500], [1, 38, 1000]):
        acc = None
        for a, b in zip([0] + cuts, cuts + [len(v)]):
            acc = go.accumulate(v[a:b], g[a:b], 12, acc)
        assert np.array_equal(acc[0], whole[0]) and np.array_equal(acc[1], whole[1])
    rows, offsets = go.tables(g, 12)
    assert offsets[-1] == len(v) and all((np.diff(rows[offsets[m]:offsets[m + 1]]) > 0).all() for m in range(12))


# ---- the surface ----
@pytest.fixture()
def grid():
    from skdownscale_amd import GridArray

    time = pd.date_range("2001-01-01", periods=800, freq="D")
    rng = np.random.default_rng(3)
    return GridArray(rng.normal(size=(800, 3, 4)), ("time", "lat", "lon"), {"time": time, "lat": np.arange(3.0), "lon": np.arange(4.0)}, name="tas")


@pytest.mark.parametrize("key,G,first", [("month", 12, 1), ("dayofyear", 365, 1), ("year", 3, 2001), ("day", 31, 1), ("quarter", 4, 1),
                                         ("dayofweek", 7, 0), ("hour", 1, 0), ("season", 4, "DJF")])
def test_key_parsing_and_the_group_dim(grid, key, G, first):
    gb = grid.groupby(f"time.{key}")
    assert (gb.dim, gb.group_dim, len(gb.labels), gb.labels[0]) == ("time", key, G, first)
    want = grid.coords["time"].month.map({12: "DJF", 1: "DJF", 2: "DJF", 3: "MAM", 4: "MAM", 5: "MAM", 6: "JJA", 7: "JJA", 8: "JJA", 9: "SON",
                                          10: "SON", 11: "SON"}) if key == "season" else getattr(grid.coords["time"], key)
    assert np.array_equal(gb.labels[gb.group], np.asarray(want))
    assert np.array_equal(gb.labels, np.unique(np.asarray(want)))


def test_labels_and_callables(grid):
    from skdownscale_amd import DAY_GROUPER, MONTH_GROUPER

    gb = grid.groupby(time=MONTH_GROUPER)
    assert gb.group_dim == "group" and np.array_equal(gb.labels, np.arange(1, 13)) and np.array_equal(gb.group, grid.coords["time"].month - 1)
    assert grid.groupby(time=DAY_GROUPER, name="dom").group_dim == "dom"
    decade = np.repeat(["b", "a", "c", "a"], 200)
    gb = grid.groupby(time=decade, name="letter")
    assert list(gb.labels) == ["a", "b", "c"] and np.array_equal(gb.group, np.repeat([1, 0, 2, 0], 200))
    # the grouped dim need not be the first, nor time
    lat = grid.groupby(lat=[5, 5, 2])
    assert list(lat.labels) == [2, 5] and lat.mean().dims == ("time", "group", "lon") and lat.mean().sizes == dict(time=800, group=2, lon=4)


def test_the_lazy_arrays_and_nothing_is_computed(grid, monkeypatch):
    import skdownscale_amd.core as core
    from skdownscale_amd import GridGroupBy, GroupAppliedGridArray, GroupReducedGridArray

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(core, "default_context", no_engine)
    gb = grid.groupby("time.month")
    assert isinstance(gb, GridGroupBy) and "12 groups of 800 steps" in repr(gb)
    for red, op in ((gb.mean(), "mean"), (gb.sum(), "sum")):
        assert isinstance(red, GroupReducedGridArray) and red._op == op and not red.computed
        assert red.dims == ("month", "lat", "lon") and red.sizes == dict(month=12, lat=3, lon=4) and red.shape == (12, 3, 4)
        assert red.dtype == np.float64 and red.name == "tas" and "time" not in red.coords
        assert np.array_equal(red.coords["month"], np.arange(1, 13)) and np.array_equal(red.coords["lat"], grid.coords["lat"])
    red = gb.mean()
    sub = red.isel(lat=slice(1, 3), lon=slice(0, 2))
    assert isinstance(sub, GroupReducedGridArray) and not sub.computed and sub.sizes == dict(month=12, lat=2, lon=2)
    assert np.array_equal(sub.coords["lat"], [1.0, 2.0])
    ch = red.chunk({"lat": 2})
    assert isinstance(ch, GroupReducedGridArray) and not ch.computed and ch.chunksizes["lat"] == (2, 1) and ch.unchunked().chunksizes is None
    # time in the middle: replaced in place
    mid = grid.transpose("lat", "time", "lon").groupby("time.season").sum()
    assert mid.dims == ("lat", "season", "lon") and mid.sizes == dict(lat=3, season=4, lon=4)
    for anom in (gb - red, gb + red, gb * red, gb / red, gb - np.zeros((12, 3, 4))):
        assert isinstance(anom, GroupAppliedGridArray) and not anom.computed and not red.computed
        assert anom.dims == grid.dims and anom.sizes == grid.sizes and anom.shape == (800, 3, 4) and anom.dtype == np.float64
        assert anom.coords["time"] is grid.coords["time"] and anom.name == "tas"
    assert [a._op for a in (gb - red, gb + red, gb * red, gb / red)] == ["sub", "add", "mul", "div"]
    # a float32 source stays float32 until it is on the device; the result is float64
    from skdownscale_amd import GridArray

    g32 = GridArray(grid.values.astype(np.float32), grid.dims, grid.coords)
    assert g32.groupby("time.month").mean().dtype == np.float64


def test_other_reductions_are_refused_by_name(grid):
    gb = grid.groupby("time.month")
    for name in ("std", "var", "max", "min", "median", "count", "first", "quantile", "apply", "map"):
        with pytest.raises(NotImplementedError, match=rf"groupby\(\.\.\.\)\.{name}\(\): only mean\(\) and sum\(\) are implemented"):
            getattr(gb, name)()
    with pytest.raises(AttributeError):
        gb.no_such_thing


def test_refusals_and_their_messages(grid):
    from skdownscale_amd import GridArray

    with pytest.raises(ValueError, match="unknown group field 'fortnight'"):
        grid.groupby("time.fortnight")
    with pytest.raises(ValueError, match="unknown group field 'normalize'"):  # a method, not a per-step attribute
        grid.groupby("time.normalize")
    with pytest.raises(ValueError, match="expected '<dim>.<field>'"):
        grid.groupby("month")
    with pytest.raises(ValueError, match="dim 'date' is not a dim of this array"):
        grid.groupby("date.month")
    with pytest.raises(ValueError, match="needs either '<dim>.<field>' or exactly one dim=labels"):
        grid.groupby()
    with pytest.raises(ValueError, match="needs either"):
        grid.groupby("time.month", time=np.zeros(800))
    with pytest.raises(ValueError, match="needs either"):
        grid.groupby(time=np.zeros(800), lat=[0, 0, 1])
    bare = GridArray(grid.values, grid.dims, {"lat": grid.coords["lat"]})
    with pytest.raises(ValueError, match="the array has no coordinate for dim 'time'"):
        bare.groupby("time.month")
    with pytest.raises(ValueError, match="needs a datetime coordinate"):
        grid.groupby("lat.month")
    with pytest.raises(ValueError, match=r"labels of shape \(799,\): expected one label for each of the 800 steps of dim 'time'"):
        grid.groupby(time=np.zeros(799))
    labels = np.arange(800.0)
    labels[17] = np.nan
    with pytest.raises(ValueError, match="label 17 of dim 'time' is NaN / NaT"):
        grid.groupby(time=labels)
    nat = np.array(grid.coords["time"].values, dtype="datetime64[ns]")
    nat[3] = np.datetime64("NaT")
    with pytest.raises(ValueError, match="label 3 of dim 'time' is NaN / NaT"):
        grid.groupby(time=nat)
    with pytest.raises(ValueError, match="the group dim 'lat' is already a dim"):
        grid.groupby(time=np.zeros(800), name="lat")


def test_other_is_matched_by_label(grid):
    from skdownscale_amd import GridArray

    summer = grid.isel(time=slice(151, 243))  # June to August 2001
    gb = summer.groupby("time.month")
    assert list(gb.labels) == [6, 7, 8]
    rng = np.random.default_rng(0)
    # extra labels, in another order, with the other dims reordered
    months = np.array([12, 8, 7, 1, 6])
    clim = GridArray(rng.normal(size=(4, 5, 3)), ("lon", "month", "lat"), {"month": months, "lat": grid.coords["lat"], "lon": grid.coords["lon"]})
    anom = gb - clim
    assert np.array_equal(months[anom.group], summer.coords["time"].month)  # the rows of `other`, by label
    assert anom._other is clim and not anom.computed
    # an ndarray is matched positionally to the sorted labels
    arr = gb * np.ones((3, 3, 4))
    assert np.array_equal(arr.group, gb.group)
    with pytest.raises(ValueError, match=r"other has shape \(12, 3, 4\); expected \(3, 3, 4\)"):
        gb - np.zeros((12, 3, 4))
    with pytest.raises(ValueError, match="other has no month=7"):
        gb - GridArray(np.zeros((2, 3, 4)), ("month", "lat", "lon"), {"month": [6, 8]})
    with pytest.raises(ValueError, match=r"other has dims \('group', 'lat', 'lon'\); expected the group dim 'month'"):
        gb - GridArray(np.zeros((3, 3, 4)), ("group", "lat", "lon"), {"group": [6, 7, 8]})
    with pytest.raises(ValueError, match="other has dims"):
        gb - GridArray(np.zeros((3, 3)), ("month", "lat"), {"month": [6, 7, 8]})
    with pytest.raises(ValueError, match="other has sizes"):
        gb - GridArray(np.zeros((3, 3, 5)), ("month", "lat", "lon"), {"month": [6, 7, 8]})
    with pytest.raises(ValueError, match="other has no coordinate for the group dim 'month'"):
        gb - GridArray(np.zeros((3, 3, 4)), ("month", "lat", "lon"))
    with pytest.raises(TypeError):
        gb - 1.0
