"""CPU: the paired skill rule and the lazy surface of GridArray.compare (skdownscale_amd/skill.py) -- no device call.

The oracle (tests/_skill_oracle.py) in its two loop orders and on series written out by hand; dims, coords and sizes of every spelling;
every refusal of the Python surface with its message; and, on the stand-in engine of tests/_oracle_engine.py extended by ``skill``,
how ``timesource.walk_pair`` brings the two sources into HBM: the same runs of whole bins for both, together within ``scratch_bytes``,
and both whole where one of them is a lazy array taken from HBM."""
import numpy as np
import pandas as pd
import pytest

import _skill_oracle as sk
from _oracle_engine import EngineFailure, OracleContext

F4, F8 = np.dtype(np.float32), np.dtype(np.float64)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def test_the_two_loop_orders_of_the_oracle_agree_bit_for_bit():
    a, b = sk.field()
    a[7, 0], b[9, 0], a[11, 5] = np.inf, -np.inf, np.inf  # (IEEE arithmetic follows from them)
    for offsets in ([0, sk.T], sk.BINS, [0, 0, 1, 8, 16, 25, 42, 42, 400]):
        rows, cells = sk.sums_by_rows(a, b, offsets), sk.sums_by_cells(a, b, offsets)
        for k in rows:
            assert np.array_equal(rows[k], cells[k], equal_nan=True), k
        assert np.array_equal(sk.finish(rows), sk.finish(cells), equal_nan=True)
    # float32 sources are widened first: the same bits as the widened arrays
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert np.array_equal(sk.skill(a32, b, sk.BINS), sk.skill(a32.astype(np.float64), b, sk.BINS), equal_nan=True)
    assert np.array_equal(sk.skill(a32, b32, sk.BINS), sk.skill(a32.astype(np.float64), b32.astype(np.float64), sk.BINS), equal_nan=True)
    # one pass and two passes give the same pass-1 sums
    one, two = sk.sums_by_rows(a, b, sk.BINS, second=False), sk.sums_by_rows(a, b, sk.BINS)
    assert all(np.array_equal(one[k], two[k], equal_nan=True) for k in ("n", "sa", "sb", "sd", "sabs", "sq"))


def test_oracle_on_series_written_out_by_hand():
    nan, inf = np.nan, np.inf
    a = np.array([1.0, 2.0, nan, 4.0, 5.0, 7.0])[:, None]
    b = np.array([2.0, 2.0, 3.0, nan, 3.0, 3.0])[:, None]
    # valid pairs: (1, 2) (2, 2) (5, 3) (7, 3): d = -1 0 2 4
    got = dict(zip(sk.STATS, sk.skill(a, b, [0, 6])[:, 0]))
    assert got["count"] == 4 and got["bias"] == 1.25 and got["ratio"] == 1.5 and got["mae"] == 1.75 and got["rmse"] == np.sqrt(21 / 4)
    # means 3.75 and 2.5: qaa = 22.75, qbb = 1, qab = 4.5
    assert got["corr"] == 4.5 / (np.sqrt(22.75) * np.sqrt(1.0)) and got["std_ratio"] == np.sqrt(22.75)
    # an empty bin, an all-invalid bin, a bin of one pair
    three = sk.skill(a, b, [0, 0, 1, 2, 2, 4, 6]).reshape(7, 6)
    assert np.array_equal(three[0], [0, 1, 1, 0, 0, 2])
    assert np.isnan(three[1:, 0]).all() and np.isnan(three[1:, 3]).all() and np.isnan(three[1:, 4]).all()  # no pair: NaN but the count
    assert np.array_equal(three[1:, 1], [-1.0, 0.5, 1.0, 1.0, nan, nan], equal_nan=True)  # one pair: finite but corr and std_ratio
    assert np.array_equal(three[1:5, 2], [0.0, 1.0, 0.0, 0.0]) and np.isnan(three[5:, 2]).all()
    # constant series: corr is NaN, std_ratio 0 (a constant) or inf (b constant); a == b: 1; b == -a: -1
    # (deviations of +-1 around the mean 2: qaa = 4 has an exact root, so the quotient is exactly +-1; in general sqrt(q) * sqrt(q)
    # need not round back to q and the correlation of a series with itself is 1 or the double below it)
    x = np.array([1.0, 3.0, 1.0, 3.0])[:, None]
    const = np.full((4, 1), 2.5)
    assert np.array_equal(sk.skill(const, x, [0, 4], ["corr", "std_ratio"])[:, 0], [nan, 0.0], equal_nan=True)
    assert np.array_equal(sk.skill(x, const, [0, 4], ["corr", "std_ratio"])[:, 0], [nan, inf], equal_nan=True)
    assert np.array_equal(sk.skill(x, x, [0, 4], ["bias", "corr", "std_ratio", "ratio"])[:, 0], [0.0, 1.0, 1.0, 1.0])
    assert np.array_equal(sk.skill(x, -x, [0, 4], ["corr", "ratio"])[:, 0], [-1.0, -1.0])
    # an inf sample is an ordinary value
    y = x.copy()
    y[1] = inf
    assert np.array_equal(sk.skill(y, x, [0, 4])[:, 0], [4.0, inf, inf, inf, inf, nan, nan], equal_nan=True)
    # the ratio of a dry record: 0 / 0
    assert np.isnan(sk.skill(np.zeros((3, 1)), np.zeros((3, 1)), [0, 3], "ratio")[0, 0])


def test_the_measured_distance_to_numpy_is_within_the_recorded_tolerance():
    a, b = sk.field()
    assert a.shape == (400, 6) and np.isnan(a[120:160, 1]).all() and np.isnan(b[:, 2]).sum() > 5 and (a[:, 3] == 0.0).mean() > 0.5
    assert set(sk.TOLERANCE) == set(sk.STATS) and all(sk.TOLERANCE[s] == 8 * sk.MEASURED[s] for s in sk.STATS)
    for offsets in (np.array([0, sk.T]), sk.BINS):
        M = len(offsets) - 1
        got, want = sk.skill(a, b, offsets).reshape(7, M, 6), sk.numpy_skill(a, b, offsets).reshape(7, M, 6)
        for i, s in enumerate(sk.STATS):
            sk.check(got[i], want[i], a, b, s, s)
    assert np.isnan(sk.skill(a, b, sk.BINS, "bias").reshape(10, 6)[3, 1])  # the bin of the NaN run


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2003-12-31", freq="D")


def pair(dtype_a=np.float64, dtype_b=np.float64, shape=(3, 4)):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(7)
    va = 285.0 + 10.0 * rng.normal(size=(len(TIME),) + shape)
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.02] = np.nan
    vb[rng.random(vb.shape) < 0.02] = np.nan
    coords = dict(time=TIME, lat=np.arange(float(shape[0])), lon=np.arange(float(shape[1])))
    return (GridArray(va.astype(dtype_a), ("time", "lat", "lon"), coords, name="tasmax"),
            GridArray(vb.astype(dtype_b), ("time", "lat", "lon"), coords, name="obs"))


def test_every_spelling_is_lazy_with_the_right_dims():
    from skdownscale_amd import GridComparison, SkillGridArray

    a, b = pair()
    cmp = a.compare(b)
    assert isinstance(cmp, GridComparison) and cmp.labels is None and list(cmp.offsets) == [0, 1095]
    assert cmp.dim == "time" and cmp.source is a and cmp.other is b
    years = cmp.resample(time="YS")
    assert list(years.offsets) == [0, 365, 730, 1095] and list(years.labels) == list(pd.date_range("2001", periods=3, freq="YS"))
    for name in sk.STATS:
        r = getattr(years, name)()
        assert isinstance(r, SkillGridArray) and not r.computed and r.dims == ("time", "lat", "lon") and r.shape == (3, 3, 4)
        assert r.sizes == dict(time=3, lat=3, lon=4) and list(r.coords["time"]) == list(years.labels) and r.dtype == np.float64
        assert np.array_equal(r.coords["lat"], a.coords["lat"]) and r.name == "tasmax" and r.statistics == (name,)
        whole = getattr(cmp, name)()  # no resample: one bin, the dim is dropped
        assert not whole.computed and whole.dims == ("lat", "lon") and whole.shape == (3, 4) and "time" not in whole.coords
    table = years.indices(["bias", "rmse", "corr"])
    assert table.dims == ("index", "time", "lat", "lon") and table.shape == (3, 3, 3, 4) and list(table.coords["index"]) == ["bias", "rmse", "corr"]
    assert cmp.indices(sk.STATS).shape == (7, 3, 4) and cmp.indices("mae").dims == ("index", "lat", "lon")
    # pandas' keywords go to the resampler
    assert list(cmp.resample(time="YS", label="right").labels) == list(pd.date_range("2002", periods=3, freq="YS"))
    assert len(cmp.resample({"time": "MS"}).labels) == 36
    # time in the middle; the other array in another order of dims
    mid = a.transpose("lat", "time", "lon").compare(b).resample(time="YS").rmse()
    assert mid.dims == ("lat", "time", "lon") and mid.shape == (3, 3, 4)
    swapped = a.compare(b.transpose("lon", "time", "lat"))
    assert swapped.other.dims == a.dims and np.array_equal(swapped.other.values, b.values, equal_nan=True)
    assert "GridComparison" in repr(years) and "SkillGridArray" in repr(table)
    # a lazy other is accepted and stays lazy; only one coordinate is needed for the bins
    lazy = b.rolling(time=3, center=True, min_periods=1).mean()
    assert a.compare(lazy).other is lazy and not lazy.computed
    from skdownscale_amd import GridArray

    bare = GridArray(a.values, a.dims)
    assert list(bare.compare(b).resample(time="YS").offsets) == [0, 365, 730, 1095]


def test_isel_along_the_other_dims_stays_lazy_and_reaches_both_sources():
    from skdownscale_amd import SkillGridArray

    a, b = pair()
    r = a.compare(b).resample(time="YS").indices(["bias", "corr"])
    cut = r.isel(lat=slice(1, 3), lon=slice(0, 2))
    assert isinstance(cut, SkillGridArray) and not cut.computed and not r.computed and cut.shape == (2, 3, 2, 2)
    assert cut.source.shape == (1095, 2, 2) and cut.other.shape == (1095, 2, 2)
    assert np.array_equal(cut.source.values, a.values[:, 1:3, 0:2], equal_nan=True)
    assert np.array_equal(cut.other.values, b.values[:, 1:3, 0:2], equal_nan=True)
    assert np.array_equal(cut.coords["lat"], [1.0, 2.0]) and list(cut.comparison.offsets) == [0, 365, 730, 1095]


def test_refusals_of_the_surface():
    from skdownscale_amd import GridArray

    a, b = pair()
    with pytest.raises(ValueError, match="compare needs a GridArray with the dims"):
        a.compare(b.values)
    with pytest.raises(ValueError, match="dim 'day' is not a dim of this array"):
        a.compare(b, dim="day")
    with pytest.raises(ValueError, match=r"other has dims \('time', 'y', 'x'\); expected \('time', 'lat', 'lon'\) in any order"):
        a.compare(GridArray(b.values, ("time", "y", "x")))
    with pytest.raises(ValueError, match=r"other has dims \('lat', 'lon'\); expected \('time', 'lat', 'lon'\)"):
        a.compare(GridArray(b.values[0], ("lat", "lon")))  # nothing is broadcast
    with pytest.raises(ValueError, match=r"other has sizes \{'time': 1095, 'lat': 3, 'lon': 3\}; expected \{'time': 1095, 'lat': 3, 'lon': 4\}"):
        a.compare(b.isel(lon=slice(0, 3)))
    with pytest.raises(ValueError, match="other has sizes .*'time': 1094"):
        a.compare(b.isel(time=slice(1, None)))
    shifted = GridArray(b.values, b.dims, dict(b.coords, time=TIME[:100].append(TIME[100:] + pd.Timedelta(days=1))))
    with pytest.raises(ValueError, match=r"the time coordinates differ at step 100: 2001-04-11 00:00:00 and 2001-04-12 00:00:00"):
        a.compare(shifted)
    assert a.compare(GridArray(b.values, b.dims)).count().shape == (3, 4)  # a coordinate on one side only: nothing to compare
    cmp = a.compare(b)
    with pytest.raises(ValueError, match=r"skill statistic 'r2': expected one of 'count', 'bias', 'ratio', 'mae', 'rmse', 'corr', 'std_ratio'"):
        cmp.indices(["bias", "r2"])
    with pytest.raises(ValueError, match="indices\\(\\) takes 1 to 7 statistics, got 0"):
        cmp.indices([])
    with pytest.raises(ValueError, match="indices\\(\\) takes 1 to 7 statistics, got 8"):
        cmp.indices(["bias"] * 8)
    with pytest.raises(ValueError, match=r"resample needs exactly time=rule, the dim of this comparison, got \['lat'\]"):
        cmp.resample(lat="YS")
    with pytest.raises(ValueError, match="resample needs exactly time=rule"):
        cmp.resample()
    bare_a, bare_b = GridArray(a.values, a.dims), GridArray(b.values, b.dims)
    with pytest.raises(ValueError, match="neither array has a coordinate for dim 'time'"):
        bare_a.compare(bare_b).resample(time="YS")
    assert bare_a.compare(bare_b).rmse().shape == (3, 4)  # one bin needs no coordinate
    back = dict(a.coords, time=TIME[::-1])
    with pytest.raises(ValueError, match="the time coordinate is not monotonic non-decreasing: position 1"):
        GridArray(a.values, a.dims, back).compare(GridArray(b.values, b.dims, back)).resample(time="YS")
    with pytest.raises(ValueError, match="nothing to compare: dim 'time' has length 0"):
        GridArray(np.zeros((0, 3)), ("time", "cell")).compare(GridArray(np.zeros((0, 3)), ("time", "cell")))
    with pytest.raises(ValueError, match="the dim 'index' of indices\\(\\) is already a dim"):
        GridArray(np.zeros((5, 3)), ("time", "index")).compare(GridArray(np.zeros((5, 3)), ("time", "index"))).indices(["bias"])


def test_the_new_names_are_exported_and_bound():
    import skdownscale_amd
    from skdownscale_amd import _lib
    from skdownscale_amd.engine import Context

    assert {"GridComparison", "SkillGridArray"} <= set(skdownscale_amd.__all__) and hasattr(skdownscale_amd.GridArray, "compare")
    assert len(_lib.SIGNATURES["sd_skill_dev"]) == 16 and len(_lib.SIGNATURES["sd_skill"]) == 12
    assert _lib.SKILL_STATS == {s: i for i, s in enumerate(sk.STATS)} and _lib.ABI_VERSION == 105
    assert callable(Context.skill) and callable(Context.skill_host)


# ---- the pair walk on the stand-in engine ---------------------------------------------------------------------------------------------
class SkillContext(OracleContext):
    """the stand-in engine with ``Context.skill``, computed by the oracle: ``("skill", rows, first bin, behind the last bin)``"""

    def skill(self, a, b, offsets, stats, out=None, plane_rows=None):
        M = len(offsets) - 1
        assert a.shape == b.shape
        self.called("skill", a.shape[0], *((0, M) if out is None else out.span()))
        res = sk.skill(a.a, b.a, offsets, stats)
        if plane_rows is None:
            return self.filled(out, res)
        assert out.base is not None and out.shape[0] == M <= plane_rows and out.row0 + (len(stats) - 1) * plane_rows + M <= out.base.shape[0]
        for s in range(len(stats)):
            out.base.a[out.row0 + s * plane_rows:out.row0 + s * plane_rows + M] = res[s * M:(s + 1) * M]
        return out


@pytest.fixture
def engine(monkeypatch):
    from skdownscale_amd import core, engine

    ctx = SkillContext()
    monkeypatch.setattr(engine, "default_context", lambda: ctx)
    monkeypatch.setattr(core, "default_context", lambda: ctx)
    return ctx


T90 = pd.date_range("2001-01-01", periods=90, freq="D")  # "MS" bins of 31 / 28 / 31 steps
C = 20


def small(dtype_a=np.float64, dtype_b=np.float64):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(3)
    va = 5.0 * rng.normal(size=(90, 4, 5))
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.05] = np.nan
    coords = dict(time=T90, lat=np.array([44.0, 42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0, -104.0, -102.0]))
    return GridArray(va.astype(dtype_a), ("time", "lat", "lon"), coords), GridArray(vb.astype(dtype_b), ("time", "lat", "lon"), coords)


NAMES = ["count", "bias", "rmse", "corr"]
# rows both blocks together have room for -> the runs of bins (first, behind the last, first step, behind the last step), by hand:
# 31 + 28 fit into 60 rows, 28 + 31 do not; a bin is never cut
CUTS = {None: [(0, 3, 0, 90)], 90: [(0, 3, 0, 90)], 60: [(0, 2, 0, 59), (2, 3, 59, 90)], 40: [(0, 1, 0, 31), (1, 2, 31, 59), (2, 3, 59, 90)],
        1: [(0, 1, 0, 31), (1, 2, 31, 59), (2, 3, 59, 90)]}


@pytest.mark.parametrize("dtypes", [(F8, F8), (F4, F8), (F8, F4), (F4, F4)], ids=lambda d: f"{d[0].name}-{d[1].name}")
@pytest.mark.parametrize("room", list(CUTS))
def test_the_pair_walk_cuts_both_sources_at_the_same_bins(engine, dtypes, room):
    a, b = small(*dtypes)
    want = sk.skill(a.values.reshape(90, C), b.values.reshape(90, C), [0, 31, 59, 90], NAMES)
    # the two blocks together stay within scratch_bytes: ``room`` rows of both dtypes
    sb = None if room is None else 1 if room == 1 else room * C * (dtypes[0].itemsize + dtypes[1].itemsize)
    lazy = a.compare(b, **({} if sb is None else dict(scratch_bytes=sb))).resample(time="MS").indices(NAMES)
    assert engine.trace == [] and not lazy.computed
    field = lazy.device_field()
    trace = []
    for m0, m1, r0, r1 in CUTS[room]:
        trace += [("upload", r1 - r0, dtypes[0]), ("upload", r1 - r0, dtypes[1]), ("skill", r1 - r0, m0, m1)]
    assert engine.trace == trace
    assert np.array_equal(field.to_host(), want, equal_nan=True)
    field.free()
    assert engine.live == 0
    # the host field in the dims of the array
    assert np.array_equal(lazy.values, want.reshape(4, 3, 4, 5), equal_nan=True)


def test_the_pair_walk_one_byte_short_of_two_bins_takes_one(engine):
    a, b = small(F4, F8)
    for sb, runs in ((59 * C * 12, 2), (59 * C * 12 - 1, 3)):
        engine.trace.clear()
        a.compare(b, scratch_bytes=sb).resample(time="MS").bias().device_field().free()
        assert len([e for e in engine.trace if e[0] == "skill"]) == runs


def test_the_pair_walk_takes_both_whole_when_one_is_lazy(engine):
    a, b = small()
    want = sk.skill(a.values.reshape(90, C), np.asarray(b.rolling(time=3, center=True, min_periods=1).mean().values).reshape(90, C),
                    [0, 31, 59, 90], NAMES)
    for first in (False, True):
        lazy_b = b.rolling(time=3, center=True, min_periods=1).mean()
        engine.trace.clear()
        engine.live = 0
        cmp = (lazy_b.compare(a) if first else a.compare(lazy_b, scratch_bytes=1)).resample(time="MS")
        field = cmp.indices(NAMES).device_field()
        own = [("upload", 90, F8), ("rolling", 90, 0, 0, 90)]  # the lazy source makes its own field, whole
        whole = [("upload", 90, F8)]  # the host array goes up in one piece, whatever scratch_bytes
        assert engine.trace == own + whole + [("skill", 90, 0, 3)]  # (the lazy field is made on entry, the upload fills the block)
        assert not lazy_b.computed
        got = field.to_host().reshape(4, 3, C)
        if first:  # (a and b exchanged: the count, the rmse and the correlation are symmetric, the bias changes its sign)
            got[1] = -got[1]
        assert np.array_equal(got[[0, 1]], want.reshape(4, 3, C)[[0, 1]], equal_nan=True)
        field.free()
        assert engine.live == 0


def test_an_unchunked_interp_like_is_produced_block_by_block_beside_a_host_array(engine):
    from skdownscale_amd import GridArray

    a, b = small()
    rng = np.random.default_rng(5)
    coarse = GridArray(5.0 * rng.normal(size=(90, 2, 2)), ("time", "lat", "lon"), dict(time=T90, lat=np.array([45.0, 37.0]), lon=np.array([-111.0, -101.0])))
    want = sk.skill(np.asarray(coarse.interp_like(a).values).reshape(90, C), b.values.reshape(90, C), [0, 31, 59, 90], NAMES)
    engine.trace.clear()
    fine = coarse.interp_like(a)
    field = fine.compare(b, scratch_bytes=60 * C * 16).resample(time="MS").indices(NAMES).device_field()
    assert engine.trace == [("regrid", 0, 59), ("upload", 59, F8), ("skill", 59, 0, 2), ("regrid", 59, 90), ("upload", 31, F8), ("skill", 31, 2, 3)]
    assert not fine.computed and np.array_equal(field.to_host(), want, equal_nan=True)
    field.free()


@pytest.mark.parametrize("k", [1, 2])
def test_a_failing_engine_call_frees_every_buffer_of_both_walks(engine, k):
    a, b = small()
    lazy = a.compare(b, scratch_bytes=60 * C * 16).resample(time="MS").rmse()
    engine.live, engine.calls, engine.fail_at = 0, 0, k
    with pytest.raises(EngineFailure):
        lazy.device_field()
    assert engine.live == 0


def test_walk_with_a_row_budget_leaves_its_other_callers_alone(engine):
    from skdownscale_amd.timesource import walk

    a, _ = small()
    off = np.array([0, 31, 59, 90])
    with walk(a, "time", engine, 60 * C * 8, "any", bins=off) as w:
        assert [k[:2] for k in w._blocks] == [(0, 2), (2, 3)]
    with walk(a, "time", engine, 60 * C * 8, "any", bins=off, row_budget=40) as w:
        assert [k[:2] for k in w._blocks] == [(0, 1), (1, 2), (2, 3)]
    assert engine.live == 0
