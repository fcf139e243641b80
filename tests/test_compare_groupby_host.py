"""CPU: the grouped oracle (tests/_grouped_pair_oracle.py) and the lazy surface of GridArray.compare(...).groupby(...)
(skdownscale_amd/skill.py, distribution.py) -- no device call.

The oracle against pandas' groupby and scipy's ks_2samp; dims, coords and label order of every spelling; the refusals; and, on the
stand-in engine of tests/_oracle_engine.py extended by the four paired calls, how both sources come into HBM whole."""
import numpy as np
import pandas as pd
import pytest

import _grouped_pair_oracle as gp
import _skill_oracle as sk
import _twosample_oracle as ts
from _oracle_engine import EngineFailure, OracleContext

F4, F8 = np.dtype(np.float32), np.dtype(np.float64)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_tables_are_a_stable_counting_sort():
    rows, offsets = gp.tables([2, 0, 2, 1, 0, 2, 2, 0, 1, 0], 3)
    assert list(rows) == [1, 4, 7, 9, 3, 8, 0, 2, 5, 6] and list(offsets) == [0, 4, 6, 10]
    rows, offsets = gp.tables([4, 1, 4, 4, 1, 3], 6)  # ids 0, 2 and 5 never occur
    assert list(rows) == [1, 4, 5, 0, 2, 3] and list(offsets) == [0, 0, 2, 2, 3, 6, 6]


def test_consecutive_groups_are_the_binned_oracles():
    a, b = sk.field()
    group = np.repeat(np.arange(10), 40)
    assert np.array_equal(gp.skill(a, b, group, 10), sk.skill(a, b, sk.BINS), equal_nan=True)
    assert np.array_equal(gp.twosample(a, b, group, 10, width=0.5), ts.twosample(a, b, sk.BINS, width=0.5), equal_nan=True)
    # an id that never occurs is an empty bin: count 0 and NaN
    got = gp.skill(a, b, group + 1, 12).reshape(7, 12, -1)
    assert (got[0, [0, 11]] == 0).all() and np.isnan(got[1:, [0, 11]]).all()
    two = gp.twosample(a, b, group + 1, 12, width=0.5).reshape(4, 12, -1)
    assert (two[2:, [0, 11]] == 0).all() and np.isnan(two[:2, [0, 11]]).all()


def test_the_paired_oracle_against_pandas_groupby():
    a, b = sk.field()  # 400 steps, 6 cells: NaN runs, isolated NaN, zero-inflated cells, a large offset
    month = np.asarray(pd.date_range("2001-01-01", periods=len(a), freq="D").month)
    labels, ids = np.unique(month, return_inverse=True)
    got = dict(zip(sk.STATS, gp.skill(a, b, ids, len(labels)).reshape(len(sk.STATS), len(labels), -1)))
    da, db = pd.DataFrame(a), pd.DataFrame(b)
    valid = da.notna() & db.notna()
    d = da - db
    ga, gb = da.where(valid).groupby(month), db.where(valid).groupby(month)
    want = {"count": valid.groupby(month).sum().to_numpy(dtype=np.float64), "bias": d.groupby(month).mean().to_numpy(),
            "mae": d.abs().groupby(month).mean().to_numpy(), "rmse": np.sqrt((d * d).groupby(month).mean().to_numpy()),
            "ratio": ga.sum(min_count=1).to_numpy() / gb.sum(min_count=1).to_numpy(),
            "std_ratio": ga.std(ddof=0).to_numpy() / gb.std(ddof=0).to_numpy(),
            "corr": np.array([[da.loc[month == m, c].corr(db.loc[month == m, c]) for c in da.columns] for m in labels])}
    assert np.array_equal(got["count"], want["count"])
    for s in sk.STATS[1:]:
        worst = sk.check(got[s], want[s], a, b, s, s)
        print(f"{s}: {worst:.3e} of the scale against pandas (allowed {sk.TOLERANCE[s]:.3e})")


def test_the_distribution_oracle_against_scipy_per_group():
    stats = pytest.importorskip("scipy.stats")
    a, b = sk.field()
    season = (np.asarray(pd.date_range("2001-01-01", periods=len(a), freq="D").month) % 12) // 3
    got = gp.twosample(a, b, season, 4, ("ks", "na", "nb")).reshape(3, 4, -1)
    worst = 0.0
    for g in range(4):
        for c in range(a.shape[1]):
            x, y = a[season == g, c], b[season == g, c]
            x, y = x[~np.isnan(x)], y[~np.isnan(y)]
            assert (got[1, g, c], got[2, g, c]) == (len(x), len(y)) and len(x) and len(y)
            worst = max(worst, abs(got[0, g, c] - stats.ks_2samp(x, y, method="asymp").statistic))
    print(f"largest difference to scipy: {worst:.3e} (allowed {ts.TOLERANCE_KS:.3e})")
    assert worst <= ts.TOLERANCE_KS


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2002-12-31", freq="D")
SEASONS = ["DJF", "JJA", "MAM", "SON"]  # the sorted labels


def pair(shape=(3, 4), coords_a=True, coords_b=True):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(7)
    va = 285.0 + 10.0 * rng.normal(size=(len(TIME),) + shape)
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.02] = np.nan
    coords = dict(time=TIME, lat=np.arange(float(shape[0])), lon=np.arange(float(shape[1])))
    bare = {k: v for k, v in coords.items() if k != "time"}
    return (GridArray(va, ("time", "lat", "lon"), coords if coords_a else bare, name="tasmax"),
            GridArray(vb, ("time", "lat", "lon"), coords if coords_b else bare, name="obs"))


def test_every_spelling_is_lazy_with_the_right_dims_coords_and_label_order():
    from skdownscale_amd import MONTH_GROUPER, DistributionGridArray, GridComparison, SkillGridArray

    a, b = pair()
    cmp = a.compare(b)
    month = np.asarray(TIME.month)
    spellings = {"month": cmp.groupby("time.month"), "dayofyear": cmp.groupby("time.dayofyear"), "season": cmp.groupby("time.season"),
                 "group": cmp.groupby(time=month), "mon": cmp.groupby(time=MONTH_GROUPER, name="mon"), "half": cmp.groupby(time=lambda t: t.month > 6, name="half")}
    want = {"month": list(range(1, 13)), "dayofyear": list(range(1, 366)), "season": SEASONS, "group": list(range(1, 13)), "mon": list(range(1, 13)),
            "half": [False, True]}
    for gdim, g in spellings.items():
        assert isinstance(g, GridComparison) and g.group_dim == gdim and list(g.group_labels) == want[gdim] and g.labels is None
        assert g.group.dtype == np.int32 and g.group.shape == (len(TIME),) and list(g.offsets) == [0, len(TIME)]
        n = len(want[gdim])
        for r in (g.bias(), g.count(), g.corr(), g.std_ratio(), g.ks(), g.perkins(0.5)):
            assert isinstance(r, (SkillGridArray, DistributionGridArray)) and not r.computed
            assert r.dims == (gdim, "lat", "lon") and r.shape == (n, 3, 4) and r.sizes == {gdim: n, "lat": 3, "lon": 4}
            assert list(r.coords[gdim]) == want[gdim] and "time" not in r.coords and np.array_equal(r.coords["lat"], a.coords["lat"])
            assert r.name == "tasmax" and r.dtype == np.float64
        for table, names in ((g.indices(["bias", "rmse", "corr"]), ["bias", "rmse", "corr"]), (g.distribution(["ks", "nb"]), ["ks", "nb"])):
            assert table.dims == ("index", gdim, "lat", "lon") and table.shape == (len(names), n, 3, 4) and list(table.coords["index"]) == names
    assert np.array_equal(spellings["month"].group, month - 1) and np.array_equal(spellings["season"].group, np.array([0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 3, 0])[month - 1])
    # the group dim replaces the compared dim in place
    mid = a.transpose("lat", "time", "lon").compare(b).groupby("time.season")
    assert mid.rmse().dims == ("lat", "season", "lon") and mid.rmse().shape == (3, 4, 4) and mid.ks().dims == ("lat", "season", "lon")
    assert mid.indices("bias").dims == ("index", "lat", "season", "lon") and mid.indices("bias")._field_order() == ("index", "season", "lat", "lon")
    assert "12 groups" in repr(spellings["month"]) and "month" in repr(spellings["month"].bias())
    # the coordinate of the other array serves where the first has none
    assert list(pair(coords_a=False)[0].compare(pair(coords_a=False)[1]).groupby("time.season").group_labels) == SEASONS


def test_isel_selects_from_both_sources():
    a, b = pair()
    g = a.compare(b).groupby("time.month")
    for r in (g.indices(["bias", "corr"]), g.distribution(["ks", "na"])):
        cut = r.isel(lat=slice(1, 3), lon=slice(0, 2))
        assert type(cut) is type(r) and not cut.computed and cut.shape == (2, 12, 2, 2)
        assert cut.source.shape == (730, 2, 2) and cut.other.shape == (730, 2, 2)
        assert cut.comparison.group_dim == "month" and np.array_equal(cut.comparison.group, g.group)


def test_refusals_of_the_surface():
    a, b = pair()
    cmp = a.compare(b)
    both = "a comparison is evaluated over the bins of resample() or over the groups of groupby(), not both"
    with pytest.raises(ValueError, match=both.replace("(", r"\(").replace(")", r"\)") + r": groupby\(\) after resample\(\)"):
        cmp.resample(time="YS").groupby("time.month")
    with pytest.raises(ValueError, match=both.replace("(", r"\(").replace(")", r"\)") + r": resample\(\) after groupby\(\)"):
        cmp.groupby("time.month").resample(time="YS")
    with pytest.raises(ValueError, match="grouped already"):
        cmp.groupby("time.month").groupby("time.season")
    with pytest.raises(ValueError, match=r"group='lat.month': expected 'time.<field>'"):
        cmp.groupby("lat.month")
    with pytest.raises(ValueError, match="groupby needs time=labels or time=callable, the dim of this comparison, got \\['lat'\\]"):
        cmp.groupby(lat=np.arange(3))
    bare_a, bare_b = pair(coords_a=False, coords_b=False)
    with pytest.raises(ValueError, match="the array has no coordinate for dim 'time'"):
        bare_a.compare(bare_b).groupby("time.month")
    assert bare_a.compare(bare_b).groupby(time=np.asarray(TIME.month)).bias().shape == (12, 3, 4)  # labels need no coordinate
    # the messages of GridGroupBy, as they are
    with pytest.raises(ValueError, match="groupby needs either '<dim>.<field>' or exactly one dim=labels"):
        cmp.groupby()
    with pytest.raises(ValueError, match="unknown group field 'fortnight'"):
        cmp.groupby("time.fortnight")
    with pytest.raises(ValueError, match="expected one label for each of the 730 steps"):
        cmp.groupby(time=np.arange(5))
    with pytest.raises(ValueError, match="the group dim 'lat' is already a dim"):
        cmp.groupby(time=np.asarray(TIME.month), name="lat")
    with pytest.raises(ValueError, match="the dim 'index' of indices"):
        cmp.groupby(time=np.asarray(TIME.month), name="index").indices("bias")


def test_the_ungrouped_and_resampled_spellings_are_what_they_were():
    a, b = pair()
    cmp = a.compare(b)
    assert cmp.group_dim is None and cmp.group is None and cmp.group_labels is None
    whole, years = cmp.rmse(), cmp.resample(time="YS").indices(["bias", "corr"])
    assert whole.dims == ("lat", "lon") and whole.sizes == dict(lat=3, lon=4) and whole._field_order() == ("lat", "lon") and "time" not in whole.coords
    assert years.dims == ("index", "time", "lat", "lon") and years.sizes == dict(index=2, time=2, lat=3, lon=4)
    assert years._field_order() == ("index", "time", "lat", "lon") and list(years.coords["time"]) == list(cmp.resample(time="YS").labels)
    assert "2 bins" in repr(cmp.resample(time="YS")) and "the whole axis" in repr(cmp)
    ks = a.transpose("lat", "time", "lon").compare(b).resample(time="YS").ks()
    assert ks.dims == ("lat", "time", "lon") and ks._field_order() == ("time", "lat", "lon") and cmp.ks().dims == ("lat", "lon")


# ---- how the sources come into HBM -----------------------------------------------------------------------------------------------------
class PairContext(OracleContext):
    """the stand-in engine with the four paired calls, computed by the oracles"""

    def _planes(self, name, a, b, M, res, nstat, out, plane_rows):
        assert a.shape == b.shape
        if plane_rows is None:
            return self.filled(out, res)
        for s in range(nstat):
            out.base.a[out.row0 + s * plane_rows:out.row0 + s * plane_rows + M] = res[s * M:(s + 1) * M]
        return out

    def skill(self, a, b, offsets, stats, out=None, plane_rows=None):
        M = len(offsets) - 1
        self.called("skill", a.shape[0], *((0, M) if out is None else out.span()))
        return self._planes("skill", a, b, M, sk.skill(a.a, b.a, offsets, stats), len(stats), out, plane_rows)

    def twosample(self, a, b, offsets, stats, width=None, origin=0.0, out=None, plane_rows=None):
        M = len(offsets) - 1
        self.called("twosample", a.shape[0], *((0, M) if out is None else out.span()))
        return self._planes("twosample", a, b, M, ts.twosample(a.a, b.a, offsets, stats, width, origin), len(stats), out, plane_rows)

    def skill_groups(self, a, b, group, G, stats, out=None, plane_rows=None):
        assert a.shape == b.shape and group.shape == (a.shape[0],) and plane_rows is None
        self.called("skill_groups", a.shape[0], G)
        return self.filled(out, gp.skill(a.a, b.a, group, G, stats))

    def twosample_groups(self, a, b, group, G, stats, width=None, origin=0.0, out=None, plane_rows=None):
        assert a.shape == b.shape and group.shape == (a.shape[0],) and plane_rows is None
        self.called("twosample_groups", a.shape[0], G)
        self.histogram = (width, origin)
        return self.filled(out, gp.twosample(a.a, b.a, group, G, stats, width, origin))


@pytest.fixture
def engine(monkeypatch):
    from skdownscale_amd import core, engine

    ctx = PairContext()
    monkeypatch.setattr(engine, "default_context", lambda: ctx)
    monkeypatch.setattr(core, "default_context", lambda: ctx)
    return ctx


T90 = pd.date_range("2001-01-15", periods=90, freq="D")  # January to April: four months, two seasons
C = 20


def small(dtype_a=np.float64, dtype_b=np.float64):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(3)
    va = 5.0 * rng.normal(size=(90, 4, 5))
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.05] = np.nan
    coords = dict(time=T90, lat=np.array([44.0, 42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0, -104.0, -102.0]))
    return GridArray(va.astype(dtype_a), ("time", "lat", "lon"), coords), GridArray(vb.astype(dtype_b), ("time", "lat", "lon"), coords)


@pytest.mark.parametrize("dtypes", [(F8, F8), (F4, F8)], ids=lambda d: f"{d[0].name}-{d[1].name}")
@pytest.mark.parametrize("scratch", [None, 1])
def test_both_sources_are_taken_whole(engine, dtypes, scratch):
    a, b = small(*dtypes)
    ids = np.asarray(T90.month) - 1
    va, vb = a.values.reshape(90, C), b.values.reshape(90, C)
    kw = {} if scratch is None else dict(scratch_bytes=scratch)
    lazy = a.compare(b, **kw).groupby("time.month").indices(["bias", "rmse", "corr"])
    assert engine.trace == [] and not lazy.computed
    field = lazy.device_field()
    assert engine.trace == [("upload", 90, dtypes[0]), ("upload", 90, dtypes[1]), ("skill_groups", 90, 4)]  # one block, whatever the room
    want = gp.skill(va, vb, ids, 4, ["bias", "rmse", "corr"])
    assert np.array_equal(field.to_host(), want, equal_nan=True)
    field.free()
    assert engine.live == 0
    assert np.array_equal(lazy.values, want.reshape(3, 4, 4, 5), equal_nan=True)
    engine.trace.clear()
    dist = a.compare(b, **kw).groupby("time.season").distribution(["ks", "perkins", "na", "nb"], width=2.0, origin=0.5)
    got = dist.values
    assert engine.trace == [("upload", 90, dtypes[0]), ("upload", 90, dtypes[1]), ("twosample_groups", 90, 2)] and engine.histogram == (2.0, 0.5)
    season = (np.asarray(T90.month) % 12) // 3  # DJF = 0, MAM = 1: the sorted labels of the two seasons present
    assert list(dist.coords["season"]) == ["DJF", "MAM"]
    assert np.array_equal(got, gp.twosample(va, vb, season, 2, ts.STATS, 2.0, 0.5).reshape(4, 2, 4, 5), equal_nan=True)
    # a single statistic in the middle of the dims, and a selection made on both sources
    mid = a.transpose("lat", "time", "lon").compare(b).groupby("time.month").rmse()
    assert np.array_equal(mid.values, np.moveaxis(gp.skill(va, vb, ids, 4, "rmse").reshape(4, 4, 5), 0, 1), equal_nan=True)
    cut = lazy.isel(lat=slice(1, 3))
    assert np.array_equal(cut.values, want.reshape(3, 4, 4, 5)[:, :, 1:3], equal_nan=True)
    assert engine.live == 0


def test_a_lazy_source_is_taken_whole_from_hbm(engine):
    a, b = small()
    lazy_b = b.rolling(time=3, center=True, min_periods=1).mean()
    vb = np.asarray(b.rolling(time=3, center=True, min_periods=1).mean().values).reshape(90, C)
    engine.trace.clear()
    engine.live = 0
    field = a.compare(lazy_b, scratch_bytes=1).groupby("time.month").bias().device_field()
    assert engine.trace == [("upload", 90, F8), ("rolling", 90, 0, 0, 90), ("upload", 90, F8), ("skill_groups", 90, 4)]
    assert not lazy_b.computed and np.array_equal(field.to_host(), gp.skill(a.values.reshape(90, C), vb, np.asarray(T90.month) - 1, 4, "bias"), equal_nan=True)
    field.free()
    assert engine.live == 0


@pytest.mark.parametrize("make", [lambda g: g.corr(), lambda g: g.ks()], ids=["skill", "distribution"])
def test_a_failing_engine_call_frees_every_buffer(engine, make):
    a, b = small()
    lazy = make(a.compare(b).groupby("time.month"))
    engine.live, engine.calls, engine.fail_at = 0, 0, 1
    with pytest.raises(EngineFailure):
        lazy.device_field()
    assert engine.live == 0
