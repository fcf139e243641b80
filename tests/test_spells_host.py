"""CPU: the threshold / spell rule and the lazy surface of GridArray.where (skdownscale_amd/spells.py) -- no device call.

The oracle (tests/_spells_oracle.py: the per-step recurrence, vectorised over the cells) against an independent run-length count per
cell (itertools.groupby); the float32-versus-double comparison rule; dims, coords and sizes of every spelling; every refusal of the
Python surface with its message."""
import numpy as np
import pandas as pd
import pytest

import _spells_oracle as sp

OPS = [">", ">=", "<", "<="]


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_oracle_equals_the_run_length_count(op):
    rng = np.random.default_rng(OPS.index(op))
    lengths = [0, 1, 7, 12, 0, 30, 5]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    T, C = int(offsets[-1]), 40
    x = np.round(rng.normal(size=(T, C)), 1)  # (rounded: ties with the threshold occur, so > and >= differ)
    x[rng.random((T, C)) < 0.08] = np.nan
    table = np.round(rng.normal(scale=0.3, size=(5, C)), 1)
    table[rng.random((5, C)) < 0.1] = np.nan  # NaN thresholds
    group = rng.integers(0, 5, size=T)
    per_step = table[group]
    for L in (1, 2, 3, 6, 30, 31, 40):  # up to and beyond the longest bin
        got = sp.spells(x, offsets, op, table, sp.STATS, L, group).reshape(len(sp.STATS), len(lengths), C)
        for m in range(len(lengths)):
            for c in range(C):
                want = sp.brute(x[offsets[m]:offsets[m + 1], c], per_step[offsets[m]:offsets[m + 1], c], op, L)
                for s, name in enumerate(sp.STATS):
                    assert np.array_equal(got[s, m, c], want[name], equal_nan=True), (op, L, m, c, name, got[s, m, c], want[name])
    ties = np.nansum(x == per_step)
    assert ties > 20  # the case x == t is in the sample


def test_oracle_on_series_written_out_by_hand():
    nan, inf = np.nan, np.inf
    #              0    1    2    3    4    5    6    7    8    9
    x = np.array([2.0, 2.0, 0.0, 2.0, nan, 2.0, 2.0, 2.0, 1.0, inf])[:, None]
    one = lambda op, L=1, thr=1.0, off=(0, 10): sp.spells(x, off, op, thr, sp.STATS, L)[:, 0]  # noqa: E731
    # > 1: hits at 0 1 3 5 6 7 9 -> runs 2, 1, 3, 1 (the NaN ends a run and is not valid)
    assert np.array_equal(one(">"), [9, 7, 7 / 9, 3, 7, 4])
    assert np.array_equal(one(">", 2), [9, 7, 7 / 9, 3, 5, 2]) and np.array_equal(one(">", 3), [9, 7, 7 / 9, 3, 3, 1])
    assert np.array_equal(one(">", 4), [9, 7, 7 / 9, 3, 0, 0])
    assert np.array_equal(one(">="), [9, 8, 8 / 9, 5, 8, 3])  # x == t at step 8 joins 5 .. 9
    assert np.array_equal(one("<"), [9, 1, 1 / 9, 1, 1, 1]) and np.array_equal(one("<="), [9, 2, 2 / 9, 1, 2, 2])
    assert np.array_equal(one("<", thr=inf), [9, 8, 8 / 9, 4, 8, 2]) and np.array_equal(one(">", thr=-inf), [9, 9, 1.0, 5, 9, 2])
    # a NaN threshold: nothing is valid; an empty bin: the same
    assert np.array_equal(one(">", thr=nan), [0, 0, nan, 0, 0, 0], equal_nan=True)
    both = sp.spells(x, [0, 0, 10], ">", 1.0, sp.STATS, 1).reshape(6, 2)
    assert np.array_equal(both[:, 0], [0, 0, nan, 0, 0, 0], equal_nan=True) and np.array_equal(both[:, 1], one(">"))
    # the run 5 6 7 is cut by a bin boundary behind step 6: both halves count by themselves
    cut = sp.spells(x, [0, 7, 10], ">", 1.0, ["longest_spell", "spell_days", "spell_count"], 2).reshape(3, 2)
    assert np.array_equal(cut, [[2, 1], [4, 0], [2, 0]])


def test_float32_samples_are_compared_as_doubles():
    x32 = np.array([[0.1], [0.7]], dtype=np.float32)
    assert float(np.float32(0.1)) > 0.1 and float(np.float32(0.7)) < 0.7  # the widened samples: one rounded up, one rounded down
    one = [0, 1, 2]  # one step per bin
    assert np.array_equal(sp.spells(x32, one, ">", 0.1, "count"), [[1.0], [1.0]])  # the pinned case: NumPy 2 says np.float32(0.1) > 0.1 is False
    assert np.array_equal(sp.spells(x32, one, "<=", 0.1, "count"), [[0.0], [0.0]])
    assert np.array_equal(sp.spells(x32, one, ">=", 0.7, "count"), [[0.0], [0.0]]) and np.array_equal(sp.spells(x32, one, "<", 0.7, "count"), [[1.0], [1.0]])
    assert np.array_equal(sp.spells(x32, one, ">=", np.array([[float(np.float32(0.1))]]), "count"), [[1.0], [1.0]])  # equal as doubles


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def obs():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(7)
    time = pd.date_range("2001-01-01", "2003-12-31", freq="D")
    v = 285.0 + 10.0 * rng.normal(size=(len(time), 3, 4))
    return GridArray(v, ("time", "lat", "lon"), dict(time=time, lat=np.arange(3.0), lon=np.arange(4.0)), name="tasmax")


def test_every_spelling_is_lazy_with_the_right_dims(obs):
    from skdownscale_amd import GridCondition, SpellGridArray

    cond = obs.where(">", 290.0)
    assert isinstance(cond, GridCondition) and cond.group is None and cond.labels is None and list(cond.offsets) == [0, 1095]
    assert cond.op == ">" and cond.dim == "time" and cond.threshold == 290.0 and cond.source is obs
    years = cond.resample(time="YS")
    assert list(years.offsets) == [0, 365, 730, 1095] and list(years.labels) == list(pd.date_range("2001", periods=3, freq="YS"))
    for make in (lambda c: c.valid(), lambda c: c.count(), lambda c: c.fraction(), lambda c: c.longest_spell(), lambda c: c.spell_days(6),
                 lambda c: c.spell_count(min_length=2)):
        a = make(years)
        assert isinstance(a, SpellGridArray) and not a.computed and a.dims == ("time", "lat", "lon") and a.shape == (3, 3, 4)
        assert a.sizes == dict(time=3, lat=3, lon=4) and list(a.coords["time"]) == list(years.labels) and a.dtype == np.float64
        assert np.array_equal(a.coords["lat"], obs.coords["lat"]) and a.name == "tasmax"
        whole = make(cond)  # no resample: one bin, the dim is dropped
        assert not whole.computed and whole.dims == ("lat", "lon") and whole.shape == (3, 4) and "time" not in whole.coords
    assert years.spell_days(6).min_length == 6 and years.spell_days(6).statistics == ("spell_days",) and years.count().min_length == 1
    both = years.indices(["count", "longest_spell"])
    assert both.dims == ("index", "time", "lat", "lon") and both.shape == (2, 3, 3, 4) and list(both.coords["index"]) == ["count", "longest_spell"]
    assert cond.indices(sp.STATS, min_length=3).shape == (6, 3, 4) and cond.indices("count").dims == ("index", "lat", "lon")
    # pandas' keywords go to the resampler
    assert list(cond.resample(time="YS", label="right").labels) == list(pd.date_range("2002", periods=3, freq="YS"))
    assert len(cond.resample({"time": "MS"}).labels) == 36
    # time in the middle
    mid = obs.transpose("lat", "time", "lon").where("<=", 280.0).resample(time="YS").count()
    assert mid.dims == ("lat", "time", "lon") and mid.shape == (3, 3, 4)
    assert "GridCondition" in repr(years) and "SpellGridArray" in repr(both)


def test_isel_along_the_other_dims_stays_lazy(obs):
    from skdownscale_amd import GridArray, SpellGridArray

    per_cell = GridArray(np.arange(12.0).reshape(3, 4), ("lat", "lon"))
    a = obs.where(">", per_cell).resample(time="YS").indices(["count", "fraction"])
    cut = a.isel(lat=slice(1, 3), lon=slice(0, 2))
    assert isinstance(cut, SpellGridArray) and not cut.computed and not a.computed and cut.shape == (2, 3, 2, 2)
    assert np.array_equal(cut.condition.threshold.values, per_cell.values[1:3, 0:2]) and cut.source.shape == (1095, 2, 2)
    assert np.array_equal(cut.coords["lat"], [1.0, 2.0]) and list(cut.condition.offsets) == [0, 365, 730, 1095]
    table = np.arange(12 * 12.0).reshape(12, 3, 4)
    by = obs.where("<", table, by="time.month").count().isel(lon=slice(1, 3))
    assert not by.computed and by.shape == (3, 2) and np.array_equal(by.condition.threshold.values, table[:, :, 1:3])
    assert np.array_equal(by.condition.group, obs.coords["time"].month - 1)
    scalar = obs.where("<", 273.15).count().isel(lat=slice(0, 1))
    assert not scalar.computed and scalar.shape == (1, 4) and scalar.condition.threshold == 273.15


def test_table_rows_are_matched_by_label(obs):
    from skdownscale_amd import GridArray

    doy = obs.coords["time"].dayofyear
    assert doy.max() == 365  # no leap year in 2001 .. 2003
    table = np.zeros((365, 3, 4))
    cond = obs.where(">", table, by="time.dayofyear")
    assert np.array_equal(cond.group, doy - 1) and cond.group.dtype == np.int32
    # a GridArray with more labels than the source has, in another order: rows by label
    labels = np.arange(366, 0, -1)
    other = GridArray(np.zeros((366, 3, 4)), ("dayofyear", "lat", "lon"), dict(dayofyear=labels))
    assert np.array_equal(obs.where(">", other, by="time.dayofyear").group, 366 - doy)
    # the lazy quantile of the same grouping is taken as it is
    thr = obs.quantile(0.9, "time", by="time.dayofyear")
    hot = obs.where(">", thr, by="time.dayofyear")
    assert hot.threshold is thr and not thr.computed and np.array_equal(hot.group, doy - 1)
    assert hot.resample(time="YS").fraction().shape == (3, 3, 4) and not thr.computed
    # labels per step and a callable
    half = np.where(np.arange(1095) < 500, "a", "b")
    assert np.array_equal(obs.where(">", np.zeros((2, 3, 4)), by=half).group, (half == "b").astype(np.int32))
    assert np.array_equal(obs.where(">", np.zeros((3, 3, 4)), by=lambda t: t.year).group, obs.coords["time"].year - 2001)


def test_refusals_of_the_surface(obs):
    from skdownscale_amd import GridArray

    with pytest.raises(ValueError, match=r"where op '==': expected one of '>', '>=', '<', '<='"):
        obs.where("==", 1.0)
    with pytest.raises(ValueError, match="dim 'day' is not a dim of this array"):
        obs.where(">", 1.0, dim="day")
    cond = obs.where(">", 290.0).resample(time="YS")
    with pytest.raises(ValueError, match=r"spell statistic 'max': expected one of 'valid', 'count', 'fraction', 'longest_spell', 'spell_days', 'spell_count'"):
        cond.indices(["count", "max"])
    with pytest.raises(ValueError, match="indices\\(\\) takes 1 to 6 statistics, got 0"):
        cond.indices([])
    with pytest.raises(ValueError, match="indices\\(\\) takes 1 to 6 statistics, got 7"):
        cond.indices(["count"] * 7)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_length=.*: expected an integer of at least 1"):
            cond.spell_days(bad)
        with pytest.raises(ValueError, match="min_length=.*: expected an integer of at least 1"):
            cond.indices(["count"], min_length=bad)
    with pytest.raises(ValueError, match="by='time.month' needs a threshold table with one field per group"):
        obs.where(">", 1.0, by="time.month")
    with pytest.raises(ValueError, match=r"by='month': expected 'time.<field>'"):
        obs.where(">", np.zeros((12, 3, 4)), by="month")
    # the table: the messages of gb - other
    short = GridArray(np.zeros((11, 3, 4)), ("month", "lat", "lon"), dict(month=np.arange(1, 12)))
    with pytest.raises(ValueError, match=r"other has no month=12: its 'month' coordinate must hold every label present in the source \(missing \[12\]\)"):
        obs.where(">", short, by="time.month")
    with pytest.raises(ValueError, match=r"other has dims \('season', 'lat', 'lon'\); expected the group dim 'month' and \('lat', 'lon'\)"):
        obs.where(">", GridArray(np.zeros((4, 3, 4)), ("season", "lat", "lon")), by="time.month")
    with pytest.raises(ValueError, match="other has sizes .*; expected .* beside 'month'"):
        obs.where(">", GridArray(np.zeros((12, 3, 5)), ("month", "lat", "lon"), dict(month=np.arange(1, 13))), by="time.month")
    with pytest.raises(ValueError, match="other has no coordinate for the group dim 'month'"):
        obs.where(">", GridArray(np.zeros((12, 3, 4)), ("month", "lat", "lon")), by="time.month")
    with pytest.raises(ValueError, match=r"other has shape \(11, 3, 4\); expected \(12, 3, 4\): one field per sorted label"):
        obs.where(">", np.zeros((11, 3, 4)), by="time.month")
    # the per-cell threshold
    with pytest.raises(ValueError, match=r"threshold has shape \(4, 3\); expected \(3, 4\): one value per cell"):
        obs.where(">", np.zeros((4, 3)))
    with pytest.raises(ValueError, match=r"threshold has dims \('month', 'lat', 'lon'\); expected \('lat', 'lon'\)"):
        obs.where(">", GridArray(np.zeros((12, 3, 4)), ("month", "lat", "lon")))
    with pytest.raises(ValueError, match="threshold has sizes"):
        obs.where(">", GridArray(np.zeros((3, 5)), ("lat", "lon")))
    # the bins
    with pytest.raises(ValueError, match=r"resample needs exactly time=rule, the dim of this condition, got \['lat'\]"):
        obs.where(">", 1.0).resample(lat="YS")
    with pytest.raises(ValueError, match="resample needs exactly time=rule"):
        obs.where(">", 1.0).resample()
    bare = GridArray(obs.values, obs.dims)
    with pytest.raises(ValueError, match="the array has no coordinate for dim 'time'"):
        bare.where(">", 1.0).resample(time="YS")
    assert bare.where(">", 1.0).count().shape == (3, 4)  # one bin needs no coordinate
    back = GridArray(obs.values, obs.dims, dict(time=obs.coords["time"][::-1]))
    with pytest.raises(ValueError, match="the time coordinate is not monotonic non-decreasing: position 1"):
        back.where(">", 1.0).resample(time="YS")
    with pytest.raises(ValueError, match="nothing to count: dim 'time' has length 0"):
        GridArray(np.zeros((0, 3)), ("time", "cell")).where(">", 1.0)
    with pytest.raises(ValueError, match="the dim 'index' of indices\\(\\) is already a dim"):
        GridArray(np.zeros((5, 3)), ("time", "index")).where(">", 1.0).indices(["count"])

