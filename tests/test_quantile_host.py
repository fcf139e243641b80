"""CPU, no engine: the oracle of GridArray.quantile / .median (tests/_quantile_oracle.py) against the installed NumPy, bit for bit, and
the host side of the feature (skdownscale_amd/order_stats.py): the lazy surface, the dims of every spelling and the refusals.

The oracle restates np.nanquantile(method=...) / np.nanmedian / np.quantile / np.median (NumPy 2) as single IEEE operations; NumPy
evaluates the same operations, so the comparison is ``==`` (the sign of a zero is not pinned), NaN where NaN."""
import warnings

import numpy as np
import pandas as pd
import pytest

import _quantile_oracle as qo

LENGTHS = (1, 2, 3, 4, 5, 64, 65, 1240)
QS = (0.0, 0.01, 0.05, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.75, 0.9, 0.95, 0.99, 1.0)


def series(rng, n, kind):
    x = 285.0 + 10.0 * rng.normal(size=n)
    if kind == "nan":
        x[rng.random(n) < 0.05] = np.nan
    elif kind == "all-nan":
        x[:] = np.nan
    elif kind == "ties":  # precipitation: 30 % exact zeros
        x = np.where(rng.random(n) < 0.3, 0.0, rng.gamma(0.7, 4.0, size=n))
    return x


def numpy_says(x, q, method, skipna):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "All-NaN slice encountered"
        if method == "median":
            return float(np.nanmedian(x) if skipna else np.median(x))
        return float(np.nanquantile(x, q, method=method) if skipna else np.quantile(x, q, method=method))


@pytest.mark.parametrize("kind", ["plain", "nan", "all-nan", "ties"])
@pytest.mark.parametrize("n", LENGTHS)
def test_oracle_is_numpy_bit_for_bit(n, kind):
    rng = np.random.default_rng(100 * n + len(kind))
    x = series(rng, n, kind)
    for skipna in (True, False):
        for method in qo.METHODS + ("median",):
            for q in (QS if method != "median" else (0.5,)):
                want = numpy_says(x, q, method, skipna)
                got = qo.quantile_1d(x, q, method, skipna)
                assert got == want or (np.isnan(got) and np.isnan(want)), f"n={n} {kind} {method} q={q} skipna={skipna}: {got!r} != {want!r}"


def test_the_field_oracle_is_the_scalar_one():
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 7, 0, 64, 65, 31]
    group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = np.stack([series(rng, len(group), k) for k in ("plain", "nan", "ties", "nan", "all-nan")], axis=1)
    x[group == 5, 1] = np.nan  # an all-NaN (group, cell)
    G, qs = len(sizes), [0.0, 1.0 / 3.0, 0.5, 0.95, 1.0]
    for dtype in (np.float64, np.float32):
        f = x.astype(dtype)
        for skipna in (True, False):
            for method in qo.METHODS + ("median",):
                got = qo.quantile_field(f, qs, group, G, method, skipna)
                Q = 1 if method == "median" else len(qs)
                assert got.shape == (Q * G, x.shape[1])
                for k in range(Q):
                    for g in range(G):
                        for c in range(x.shape[1]):
                            want = qo.quantile_1d(f[group == g, c], qs[k], method, skipna)
                            assert qo.same(got[k * G + g, c], want), (dtype, skipna, method, k, g, c)
                assert np.isnan(got[4::G]).all()  # the group without a row
    whole = qo.quantile_field(x, 0.5)
    assert whole.shape == (1, 5) and qo.same(whole[0, 0], np.nanquantile(x[:, 0], 0.5))


# ---- the surface ----
@pytest.fixture()
def grid():
    from skdownscale_amd import GridArray

    time = pd.date_range("2001-01-01", periods=800, freq="D")
    rng = np.random.default_rng(3)
    return GridArray(rng.normal(size=(3, 800, 4)), ("lat", "time", "lon"), {"time": time, "lat": np.arange(3.0), "lon": np.arange(4.0)}, name="tas")


def test_exported():
    import skdownscale_amd

    assert "TimeQuantileGridArray" in skdownscale_amd.__all__ and hasattr(skdownscale_amd, "TimeQuantileGridArray")
    assert "sd_quantile_dev" in skdownscale_amd._lib.SIGNATURES and "sd_quantile" in skdownscale_amd._lib.SIGNATURES


def test_scalar_and_array_q_with_dim_in_the_middle(grid):
    from skdownscale_amd import TimeQuantileGridArray

    a = grid.quantile(0.9)
    assert isinstance(a, TimeQuantileGridArray) and not a.computed
    assert a.dims == ("lat", "lon") and a.sizes == {"lat": 3, "lon": 4} and a.shape == (3, 4) and a.dtype == np.float64
    assert set(a.coords) == {"lat", "lon"} and a.name == "tas" and a.q == 0.9 and a.method == "linear" and a.group_dim is None
    b = grid.quantile([0.1, 0.5], "time", method="nearest")
    assert b.dims == ("quantile", "lat", "lon") and b.shape == (2, 3, 4) and np.array_equal(b.coords["quantile"], [0.1, 0.5]) and not b.computed
    m = grid.median()
    assert m.dims == ("lat", "lon") and m.method == "median" and not m.computed
    c = grid.quantile(0.5, dim="lon")
    assert c.dims == ("lat", "time") and c.sizes == {"lat": 3, "time": 800} and "time" in c.coords
    cut = a.isel(lat=slice(1, 3))
    assert isinstance(cut, TimeQuantileGridArray) and not cut.computed and cut.sizes == {"lat": 2, "lon": 4} and np.array_equal(cut.coords["lat"], [1.0, 2.0])


@pytest.mark.parametrize("by,gdim,G,first", [("time.month", "month", 12, 1), ("time.dayofyear", "dayofyear", 365, 1), ("time.season", "season", 4, "DJF"),
                                             ("labels", "group", 3, 0), ("callable", "group", 12, 1), ("named", "mon", 12, 1)])
def test_by_in_every_spelling(grid, by, gdim, G, first):
    from skdownscale_amd import MONTH_GROUPER

    kw = {}
    if by == "labels":
        by = np.arange(800) % 3
    elif by == "callable":
        by = MONTH_GROUPER
    elif by == "named":
        by, kw = MONTH_GROUPER, {"name": "mon"}
    a = grid.quantile(0.9, "time", by=by, **kw)
    assert a.dims == ("lat", gdim, "lon") and a.sizes == {"lat": 3, gdim: G, "lon": 4} and a.group_dim == gdim and not a.computed
    assert a.coords[gdim][0] == first and len(a.coords[gdim]) == G and "time" not in a.coords
    assert a.group.dtype == np.int32 and a.group.shape == (800,)
    gb = grid.groupby(by) if isinstance(by, str) else grid.groupby(time=by)
    assert np.array_equal(a.coords[gdim], gb.labels) and np.array_equal(a.group, gb.group)  # the sorted-unique-labels rule of groupby
    b = grid.quantile([0.05, 0.5, 0.95], "time", by=by, **kw)
    assert b.dims == ("quantile", "lat", gdim, "lon") and b.shape == (3, 3, G, 4)
    m = grid.median("time", by=by, **kw)
    assert m.dims == a.dims and m.sizes == a.sizes
    # a selection along the other dims stays lazy
    cut = a.isel(lon=slice(0, 2))
    assert not cut.computed and cut.sizes == {"lat": 3, gdim: G, "lon": 2}


def test_refusals(grid):
    for q in (-0.01, 1.5, np.nan, [0.5, 1.0000001], [0.2, np.nan]):
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            grid.quantile(q)
    with pytest.raises(ValueError, match="q must be one quantile or a non-empty 1-D sequence"):
        grid.quantile([])
    with pytest.raises(ValueError, match="quantile method 'hazen': expected one of 'linear', 'lower', 'higher', 'nearest', 'midpoint'"):
        grid.quantile(0.5, method="hazen")
    with pytest.raises(ValueError, match="dim 'date' is not a dim of this array"):
        grid.quantile(0.5, "date")
    with pytest.raises(ValueError, match="dim 'date' is not a dim of this array"):
        grid.median("date")
    with pytest.raises(ValueError, match="by='lat.month': expected 'time.<field>'"):
        grid.quantile(0.5, "time", by="lat.month")
    labels = np.arange(800, dtype=np.float64)
    labels[17] = np.nan
    with pytest.raises(ValueError, match="label 17 of dim 'time' is NaN / NaT"):
        grid.quantile(0.5, "time", by=labels)
    with pytest.raises(ValueError, match="the group dim 'lat' is already a dim of this array"):
        grid.quantile(0.5, "time", by=np.arange(800) % 3, name="lat")
    with pytest.raises(ValueError, match="expected one label for each of the 800 steps"):
        grid.quantile(0.5, "time", by=np.arange(10))
    with pytest.raises(ValueError, match="unknown group field 'fortnight'"):
        grid.quantile(0.5, "time", by="time.fortnight")


def test_the_grouped_spellings_stay_refused(grid):
    with pytest.raises(NotImplementedError, match="only mean\\(\\) and sum\\(\\)"):
        grid.groupby("time.month").quantile(0.5)
    with pytest.raises(NotImplementedError, match="only mean\\(\\) and sum\\(\\)"):
        grid.groupby("time.month").median()
    with pytest.raises(NotImplementedError, match="only mean\\(\\), sum\\(\\), var\\(\\) and std\\(\\)"):
        grid.rolling(time=5).quantile(0.5)


def test_a_grouped_quantile_is_taken_where_a_lazy_reduction_is(grid):
    """as ``other`` of ``gb - other`` and as the source of a rolling window over the group dim: nothing is computed when the chain is made"""
    from skdownscale_amd.timesource import TAKEN_WHOLE, takes_whole

    a = grid.transpose("time", "lat", "lon")
    thr = a.quantile(0.9, "time", by="time.dayofyear")
    with_reductions = [c for c, kinds in TAKEN_WHOLE.items() if "group_reduced" in kinds]  # (who takes a lazy reduction takes this)
    assert thr._row_dim() == "dayofyear" and all(takes_whole(thr, c, "dayofyear") for c in with_reductions)
    assert not any(takes_whole(thr, c, "dayofyear") for c in TAKEN_WHOLE if c not in with_reductions)
    assert a.quantile([0.9], "time", by="time.dayofyear")._row_dim() is None  # [Q * G, C]: not a [G, C] table
    assert a.quantile(0.9)._row_dim() is None
    smooth = thr.rolling(dayofyear=5, center=True, wrap=True).mean()
    anom = a.groupby("time.month") - a.median("time", by="time.month")
    assert not thr.computed and not smooth.computed and not anom.computed
    assert smooth.sizes == {"dayofyear": 365, "lat": 3, "lon": 4} and anom.sizes == a.sizes
