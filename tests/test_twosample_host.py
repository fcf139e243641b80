"""CPU: the two-sample rule and the lazy surface of GridArray.compare(...).ks() / .perkins() / .distribution()
(skdownscale_amd/distribution.py) -- no device call.

The oracle (tests/_twosample_oracle.py) against scipy and np.histogram and on its exact properties; the NaN rule; dims, coords and sizes
of every spelling; every refusal of the Python surface with its message; and, on the stand-in engine of tests/_oracle_engine.py extended
by ``twosample``, how ``timesource.walk_pair`` brings the two sources into HBM."""
import numpy as np
import pandas as pd
import pytest

import _twosample_oracle as ts
from _oracle_engine import EngineFailure, OracleContext

F4, F8 = np.dtype(np.float32), np.dtype(np.float64)


def series(rng, tied):
    na, nb = rng.integers(1, 400, 2)
    a, b = rng.normal(size=na), rng.normal(0.2, 1.1, size=nb)
    return (np.round(a * 8.0) / 8.0, np.round(b * 8.0) / 8.0) if tied else (a, b)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [False, True], ids=["continuous", "tied in eighths"])
def test_ks_against_scipy(tied):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(11 + tied)
    worst = 0.0
    for _ in range(300):
        a, b = series(rng, tied)
        got = ts.one(a, b, ("ks",))[0]
        worst = max(worst, abs(got - stats.ks_2samp(a, b, method="asymp").statistic))
    print(f"largest difference to scipy: {worst:.3e} (allowed {ts.TOLERANCE_KS:.3e}, recorded {ts.MEASURED_KS:.3e})")
    assert worst <= ts.TOLERANCE_KS
    assert ts.TOLERANCE_KS == 4.5e-16 and ts.MEASURED_KS <= ts.TOLERANCE_KS


@pytest.mark.parametrize("tied", [False, True], ids=["continuous", "tied in eighths"])
def test_perkins_against_a_histogram_overlap(tied):
    rng = np.random.default_rng(21 + tied)
    for _ in range(200):
        a, b = series(rng, tied)
        for width, origin in ((0.5, 0.0625), (0.3, -0.01), (2.0, 0.0625)):  # (no multiple of 1 / 8 lies on an edge)
            got = ts.one(a, b, ("perkins",), width, origin)[0]
            assert abs(got - ts.histogram_overlap(a, b, width, origin)) <= ts.TOLERANCE_PERKINS
            assert 0.0 <= got <= 1.0


def test_exact_properties():
    rng = np.random.default_rng(5)
    for tied in (False, True):
        for _ in range(100):
            a, b = series(rng, tied)
            assert ts.one(a, a, ("ks", "perkins"), 0.5) == [0.0, 1.0]
            assert ts.one(a, b, ("ks", "perkins", "na", "nb"), 0.25, 0.1) == [ts.one(b, a, ("ks", "perkins", "nb", "na"), 0.25, 0.1)[i] for i in range(4)]
            # disjoint supports
            assert ts.one(a, b + 100.0, ("ks", "perkins"), 0.5) == [1.0, 0.0] and ts.one(a + 100.0, b, ("ks", "perkins"), 0.5) == [1.0, 0.0]
    # a one-sample series against three: the distribution function of a jumps from 0 to 1 at 2
    assert ts.one([2.0], [1.0, 2.0, 3.0], ("ks", "na", "nb")) == [1.0 / 3.0, 1.0, 3.0]
    assert ts.one([2.0], [2.0], ("ks", "perkins"), 1.0) == [0.0, 1.0] and ts.one([2.0], [2.5], ("ks", "perkins"), 1.0) == [1.0, 1.0]
    assert ts.one([0.0, 1.0, 2.0, 3.0], [0.5, 1.5], ("ks",)) == [0.5]  # just before 2: Fa = 2 / 4, Fb = 1
    # written out by hand: a = 1 1 2 4, b = 1 3 3 5 5; Fa - Fb at 1: 2/4 - 1/5, at 2: 3/4 - 1/5, at 4: 1 - 3/5; num = 15 - 4 = 11
    assert ts.one([4.0, 1.0, 2.0, 1.0], [5.0, 3.0, 1.0, 3.0, 5.0], ("ks",)) == [11.0 / 20.0]
    # bins of width 2 from 0: a has 3 in [0, 2) and 1 in [4, 6); b has 1, 2 ([2, 4)), 2: min(3 * 5, 1 * 4) + min(1 * 5, 2 * 4) = 9
    assert ts.one([4.0, 1.0, 1.5, 1.0], [5.0, 3.0, 1.0, 3.0, 5.0], ("perkins",), 2.0) == [9.0 / 20.0]
    assert ts.one([4.0, 1.0, 1.5, 1.0], [5.0, 3.0, 1.0, 3.0, 5.0], ("perkins",), 2.0, 1.0) == [(min(3 * 5, 1 * 4) + min(1 * 5, 2 * 4)) / 20.0]  # [1, 3): 3 and 1, [3, 5): 1 and 2
    assert ts.one([4.0, 1.0, 1.5, 1.0], [5.0, 3.0, 1.0, 3.0, 5.0], ("perkins",), 4.0, 1.0) == [min(4 * 5, 3 * 4) / 20.0]  # [1, 5): 4 and 3


def test_infinities_are_ordinary_values():
    inf = np.inf
    a, b = np.array([-inf, 0.0, 1.0, inf]), np.array([-inf, -inf, 0.5, 2.0])
    # Fa - Fb: at -inf 1/4 - 2/4; at 0 2/4 - 2/4; at 1 3/4 - 3/4; at inf 1 - 1; just before 0: 1/4 - 2/4
    assert ts.one(a, b, ("ks", "na", "nb")) == [0.25, 4.0, 4.0]
    # bins of width 1: a: -inf, 0, 1, inf; b: -inf x 2, 0, 2 -> min(1, 2) + min(1, 1) + 0 + 0 of 4
    assert ts.one(a, b, ("perkins",), 1.0) == [0.5]
    assert ts.one([inf, inf], [inf], ("ks", "perkins"), 1.0) == [0.0, 1.0] and ts.one([inf], [-inf], ("ks", "perkins"), 3.0) == [1.0, 0.0]
    assert list(ts.hist_bin([-inf, inf, -0.0], 2.0, 0.5)) == [-inf, inf, -1.0]


def test_the_nan_rule_is_unpaired():
    nan = np.nan
    a = np.array([1.0, nan, 3.0, 4.0, nan, 6.0])[:, None]
    b = np.array([nan, 2.0, 3.0, nan, nan, nan])[:, None]
    got = dict(zip(ts.STATS, ts.twosample(a, b, [0, 6], width=1.0)[:, 0]))
    assert got["na"] == 4 and got["nb"] == 2  # a paired count would be 1
    assert got["ks"] == ts.one([1.0, 3.0, 4.0, 6.0], [2.0, 3.0], ("ks",))[0] == 0.5 and got["perkins"] == 0.25
    # bins: an empty one, one where b is all NaN, one where both have samples
    table = ts.twosample(a, b, [0, 0, 1, 6], width=1.0).reshape(4, 3)
    assert np.array_equal(table[2:], [[0, 1, 3], [0, 0, 2]])
    assert np.isnan(table[:2, :2]).all() and np.isfinite(table[:2, 2]).all()
    # float32 is widened first: the bits of the widened arrays
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=(50, 3)).astype(np.float32), rng.normal(size=(50, 3))
    assert np.array_equal(ts.twosample(x, y, [0, 20, 50], width=0.1), ts.twosample(x.astype(np.float64), y, [0, 20, 50], width=0.1))


# ---- the lazy surface ------------------------------------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", "2003-12-31", freq="D")


def pair(shape=(3, 4)):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(7)
    va = 285.0 + 10.0 * rng.normal(size=(len(TIME),) + shape)
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.02] = np.nan
    coords = dict(time=TIME, lat=np.arange(float(shape[0])), lon=np.arange(float(shape[1])))
    return GridArray(va, ("time", "lat", "lon"), coords, name="tasmax"), GridArray(vb, ("time", "lat", "lon"), coords, name="obs")


def test_every_spelling_is_lazy_with_the_right_dims():
    from skdownscale_amd import DistributionGridArray

    a, b = pair()
    cmp = a.compare(b)
    years = cmp.resample(time="YS")
    for make, names in ((lambda c: c.ks(), ("ks",)), (lambda c: c.perkins(0.5), ("perkins",)), (lambda c: c.perkins(2, origin=-1), ("perkins",))):
        r = make(years)
        assert isinstance(r, DistributionGridArray) and not r.computed and r.dims == ("time", "lat", "lon") and r.shape == (3, 3, 4)
        assert r.sizes == dict(time=3, lat=3, lon=4) and list(r.coords["time"]) == list(years.labels) and r.dtype == np.float64
        assert np.array_equal(r.coords["lat"], a.coords["lat"]) and r.name == "tasmax" and r.statistics == names
        whole = make(cmp)  # no resample: one bin, the dim is dropped
        assert not whole.computed and whole.dims == ("lat", "lon") and whole.shape == (3, 4) and "time" not in whole.coords
    assert cmp.ks().width is None and cmp.perkins(2, origin=-1).width == 2.0 and cmp.perkins(2, origin=-1).origin == -1.0
    table = years.distribution(["ks", "perkins", "na"], width=0.5)
    assert table.dims == ("index", "time", "lat", "lon") and table.shape == (3, 3, 3, 4) and list(table.coords["index"]) == ["ks", "perkins", "na"]
    assert cmp.distribution(ts.STATS, 1.0).shape == (4, 3, 4) and cmp.distribution("ks").dims == ("index", "lat", "lon")
    assert cmp.distribution(["na", "nb"]).width is None  # no histogram is needed
    mid = a.transpose("lat", "time", "lon").compare(b).resample(time="YS").ks()
    assert mid.dims == ("lat", "time", "lon") and mid.shape == (3, 3, 4)
    assert "DistributionGridArray" in repr(table) and "ks, perkins, na" in repr(table)
    cut = table.isel(lat=slice(1, 3), lon=slice(0, 2))
    assert isinstance(cut, DistributionGridArray) and not cut.computed and cut.shape == (3, 3, 2, 2) and cut.width == 0.5
    assert cut.source.shape == (1095, 2, 2) and cut.other.shape == (1095, 2, 2) and list(cut.comparison.offsets) == [0, 365, 730, 1095]


def test_refusals_of_the_surface():
    from skdownscale_amd import GridArray

    a, b = pair()
    cmp = a.compare(b)
    with pytest.raises(ValueError, match="distribution statistic 'crps': expected one of 'ks', 'perkins', 'na', 'nb'"):
        cmp.distribution(["ks", "crps"])
    with pytest.raises(ValueError, match="distribution statistic 'bias'"):
        cmp.distribution("bias")  # the paired statistics stay with indices()
    with pytest.raises(ValueError, match=r"distribution\(\) takes 1 to 4 statistics, got 0"):
        cmp.distribution([])
    with pytest.raises(ValueError, match=r"distribution\(\) takes 1 to 4 statistics, got 5"):
        cmp.distribution(["ks"] * 5)
    with pytest.raises(ValueError, match="perkins needs the width of the histogram bins"):
        cmp.distribution(["ks", "perkins"])
    with pytest.raises(TypeError):
        cmp.perkins()
    for bad in (0, -1.0, np.nan, np.inf, "1", None, [1.0], True):
        with pytest.raises(ValueError, match="perkins needs the width" if bad is None else "width: expected a positive finite number, got"):
            cmp.perkins(bad)
    for bad in (np.nan, -np.inf, "0", [0.0]):
        with pytest.raises(ValueError, match="origin: expected a finite number, got"):
            cmp.perkins(1.0, origin=bad)
    with pytest.raises(ValueError, match=r"the dim 'index' of distribution\(\) is already a dim"):
        GridArray(np.zeros((5, 3)), ("time", "index")).compare(GridArray(np.zeros((5, 3)), ("time", "index"))).distribution(["ks"])
    assert GridArray(np.zeros((5, 3)), ("time", "index")).compare(GridArray(np.zeros((5, 3)), ("time", "index"))).ks().dims == ("index",)


def test_the_paired_statistics_are_untouched():
    import _skill_oracle as sk
    from skdownscale_amd import skill

    a, b = pair()
    assert skill.STATS == sk.STATS == ("count", "bias", "ratio", "mae", "rmse", "corr", "std_ratio")
    with pytest.raises(ValueError, match="skill statistic 'ks': expected one of 'count', 'bias', 'ratio', 'mae', 'rmse', 'corr', 'std_ratio'"):
        a.compare(b).indices(["ks"])
    with pytest.raises(ValueError, match=r"indices\(\) takes 1 to 7 statistics, got 8"):
        a.compare(b).indices(["bias"] * 8)
    assert a.compare(b).indices(sk.STATS).shape == (7, 3, 4)


def test_the_new_names_are_exported_and_bound():
    import skdownscale_amd
    from skdownscale_amd import _lib, distribution
    from skdownscale_amd.engine import Context

    assert "DistributionGridArray" in skdownscale_amd.__all__ and distribution.STATS == ts.STATS
    assert all(hasattr(skdownscale_amd.GridComparison, m) for m in ("ks", "perkins", "distribution"))
    assert len(_lib.SIGNATURES["sd_twosample_dev"]) == 18 and len(_lib.SIGNATURES["sd_twosample"]) == 14
    assert _lib.TWOSAMPLE_STATS == {s: i for i, s in enumerate(ts.STATS)} and _lib.ABI_VERSION == 105
    assert callable(Context.twosample) and callable(Context.twosample_host)
    assert "distribution scores" not in skdownscale_amd.skill.__doc__.split("Out of scope")[1]


# ---- the pair walk on the stand-in engine ---------------------------------------------------------------------------------------------
class TwosampleContext(OracleContext):
    """the stand-in engine with ``Context.twosample``, computed by the oracle: ``("twosample", rows, first bin, behind the last bin)``"""

    def twosample(self, a, b, offsets, stats, width=None, origin=0.0, out=None, plane_rows=None):
        M = len(offsets) - 1
        assert a.shape == b.shape
        self.called("twosample", a.shape[0], *((0, M) if out is None else out.span()))
        self.histogram = (width, origin)
        res = ts.twosample(a.a, b.a, offsets, stats, width, origin)
        if plane_rows is None:
            return self.filled(out, res)
        assert out.base is not None and out.shape[0] == M <= plane_rows and out.row0 + (len(stats) - 1) * plane_rows + M <= out.base.shape[0]
        for s in range(len(stats)):
            out.base.a[out.row0 + s * plane_rows:out.row0 + s * plane_rows + M] = res[s * M:(s + 1) * M]
        return out


@pytest.fixture
def engine(monkeypatch):
    from skdownscale_amd import core, engine

    ctx = TwosampleContext()
    monkeypatch.setattr(engine, "default_context", lambda: ctx)
    monkeypatch.setattr(core, "default_context", lambda: ctx)
    return ctx


T90 = pd.date_range("2001-01-01", periods=90, freq="D")  # "MS" bins of 31 / 28 / 31 steps
C = 20
NAMES = ["ks", "perkins", "na", "nb"]
CUTS = {None: [(0, 3, 0, 90)], 60: [(0, 2, 0, 59), (2, 3, 59, 90)], 1: [(0, 1, 0, 31), (1, 2, 31, 59), (2, 3, 59, 90)]}


def small(dtype_a=np.float64, dtype_b=np.float64):
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(3)
    va = 5.0 * rng.normal(size=(90, 4, 5))
    vb = va + rng.normal(size=va.shape)
    va[rng.random(va.shape) < 0.05] = np.nan
    coords = dict(time=T90, lat=np.array([44.0, 42.0, 40.0, 38.0]), lon=np.array([-110.0, -108.0, -106.0, -104.0, -102.0]))
    return GridArray(va.astype(dtype_a), ("time", "lat", "lon"), coords), GridArray(vb.astype(dtype_b), ("time", "lat", "lon"), coords)


@pytest.mark.parametrize("dtypes", [(F8, F8), (F4, F8), (F4, F4)], ids=lambda d: f"{d[0].name}-{d[1].name}")
@pytest.mark.parametrize("room", list(CUTS))
def test_the_pair_walk_cuts_both_sources_at_the_same_bins(engine, dtypes, room):
    a, b = small(*dtypes)
    want = ts.twosample(a.values.reshape(90, C), b.values.reshape(90, C), [0, 31, 59, 90], NAMES, 2.0, 0.5)
    sb = None if room is None else 1 if room == 1 else room * C * (dtypes[0].itemsize + dtypes[1].itemsize)
    lazy = a.compare(b, **({} if sb is None else dict(scratch_bytes=sb))).resample(time="MS").distribution(NAMES, width=2.0, origin=0.5)
    assert engine.trace == [] and not lazy.computed
    field = lazy.device_field()
    trace = []
    for m0, m1, r0, r1 in CUTS[room]:
        trace += [("upload", r1 - r0, dtypes[0]), ("upload", r1 - r0, dtypes[1]), ("twosample", r1 - r0, m0, m1)]
    assert engine.trace == trace and engine.histogram == (2.0, 0.5)
    assert np.array_equal(field.to_host(), want, equal_nan=True)
    field.free()
    assert engine.live == 0
    assert np.array_equal(lazy.values, want.reshape(4, 3, 4, 5), equal_nan=True)  # the host field in the dims of the array
    # one statistic, the whole axis: the dim is dropped
    engine.trace.clear()
    ks = a.compare(b).ks()
    assert np.array_equal(ks.values, ts.twosample(a.values.reshape(90, C), b.values.reshape(90, C), [0, 90], "ks").reshape(4, 5))
    assert engine.trace[-1] == ("twosample", 90, 0, 1) and engine.histogram == (None, 0.0)


def test_the_pair_walk_takes_both_whole_when_one_is_lazy(engine):
    a, b = small()
    lazy_b = b.rolling(time=3, center=True, min_periods=1).mean()
    want = ts.twosample(a.values.reshape(90, C), np.asarray(b.rolling(time=3, center=True, min_periods=1).mean().values).reshape(90, C),
                        [0, 31, 59, 90], NAMES, 1.0)
    engine.trace.clear()
    engine.live = 0
    field = a.compare(lazy_b, scratch_bytes=1).resample(time="MS").distribution(NAMES, 1.0).device_field()
    assert engine.trace == [("upload", 90, F8), ("rolling", 90, 0, 0, 90), ("upload", 90, F8), ("twosample", 90, 0, 3)]
    assert not lazy_b.computed and np.array_equal(field.to_host(), want, equal_nan=True)
    field.free()
    assert engine.live == 0


@pytest.mark.parametrize("k", [1, 2])
def test_a_failing_engine_call_frees_every_buffer_of_both_walks(engine, k):
    a, b = small()
    lazy = a.compare(b, scratch_bytes=60 * C * 16).resample(time="MS").ks()
    engine.live, engine.calls, engine.fail_at = 0, 0, k
    with pytest.raises(EngineFailure):
        lazy.device_field()
    assert engine.live == 0
