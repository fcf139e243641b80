"""The definition of GridArray.quantile / .median (include/sd_downscale.h: sd_quantile), restated from NumPy 2's np.nanquantile /
np.nanmedian / np.quantile / np.median.

One cell and one group: v = the samples without NaN, ascending, n = len(v).  n == 0 gives NaN; with ``skipna=False`` any NaN among
the samples gives NaN.  Otherwise h = float(n - 1) * q, lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1), a = v[lo], b = v[hi],
d = b - a and
    linear    g >= 0.5 ? b - d * (1 - g) : a + d * g        (NumPy's _lerp, evaluated at g = 0 too)
    lower     v[floor(h)]
    higher    v[ceil(h)]
    nearest   v[rint(h)], half to even
    midpoint  v[lo] if h is whole, else b - d * 0.5
    median    v[n // 2] for odd n, (v[n // 2 - 1] + v[n // 2]) / 2 for even n
Every operation is one IEEE double operation; ``quantile_1d`` is the definition on Python floats, ``quantile_field`` the same operations
elementwise on whole [T, C] fields (NumPy's elementwise float64 arithmetic is IEEE arithmetic), in the layout of the engine: row
``q * G + g`` of the result is quantile q of group g.  tests/test_quantile_host.py holds both against NumPy bit for bit."""
import math

import numpy as np

METHODS = ("linear", "lower", "higher", "nearest", "midpoint")
CODES = {"linear": 0, "lower": 1, "higher": 2, "nearest": 3, "midpoint": 4, "median": 5}


def quantile_1d(x, q, method="linear", skipna=True):
    """one quantile of one series, on Python floats"""
    x = [float(t) for t in np.asarray(x, dtype=np.float64).ravel()]
    v = sorted(t for t in x if not math.isnan(t))
    n = len(v)
    if n == 0 or (not skipna and n < len(x)):
        return math.nan
    if method == "median":
        return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0
    h = float(n - 1) * float(q)
    lo = math.floor(h)
    g = h - lo
    hi = min(lo + 1, n - 1)
    a, b = v[lo], v[hi]
    d = b - a
    if method == "linear":
        return b - d * (1.0 - g) if g >= 0.5 else a + d * g
    if method == "lower":
        return v[lo]
    if method == "higher":
        return v[math.ceil(h)]
    if method == "nearest":
        return v[round(h)]  # (Python rounds half to even)
    if method == "midpoint":
        return v[lo] if g == 0.0 else b - d * 0.5
    raise ValueError(method)


def sorted_groups(field, group=None, G=None):
    """per group: (the [n_g, C] float64 samples sorted per cell with NaN last, the [C] counts of non-NaN samples): what every method and
    every q of one field share"""
    x = np.asarray(field)
    x = x.astype(np.float64)  # (widening float32 is exact)
    T, C = x.shape
    if group is None:
        group, G = np.zeros(T, dtype=np.int64), 1
    group = np.asarray(group)
    G = int(group.max()) + 1 if G is None else int(G)
    out = []
    for g in range(G):
        sub = np.sort(x[group == g], axis=0)  # (NaN sort last)
        out.append((sub, np.count_nonzero(~np.isnan(sub), axis=0)))
    return out


def quantile_sorted(groups, q, method="linear", skipna=True):
    """[Q * G, C] from ``sorted_groups``: row q * G + g"""
    qs = np.array([0.5]) if method == "median" else np.atleast_1d(np.asarray(q, dtype=np.float64))
    G, C = len(groups), groups[0][0].shape[1]
    out = np.full((len(qs) * G, C), np.nan)
    cells = np.arange(C)
    for g, (sub, nv) in enumerate(groups):
        n = sub.shape[0]
        ok = (nv > 0) if skipna else (nv == n) & (n > 0)
        if n == 0 or not ok.any():
            continue
        m = np.where(ok, nv, 1)  # (cells without a result evaluate in bounds and are dropped)

        def at(i):
            return sub[np.asarray(i, dtype=np.int64), cells]

        for k, qq in enumerate(qs):
            if method == "median":
                odd = at(m // 2)
                even = (at(np.maximum(m // 2 - 1, 0)) + at(m // 2)) / 2.0
                res = np.where(m % 2 == 1, odd, even)
            else:
                h = (m - 1).astype(np.float64) * qq
                lo = np.floor(h)
                gam = h - lo
                hi = np.minimum(lo + 1, m - 1)
                a, b = at(lo), at(hi)
                with np.errstate(invalid="ignore"):
                    d = b - a
                    if method == "linear":
                        res = np.where(gam >= 0.5, b - d * (1.0 - gam), a + d * gam)
                    elif method == "lower":
                        res = a
                    elif method == "higher":
                        res = at(np.ceil(h))
                    elif method == "nearest":
                        res = at(np.rint(h))
                    elif method == "midpoint":
                        res = np.where(gam == 0.0, a, b - d * 0.5)
                    else:
                        raise ValueError(method)
            out[k * G + g] = np.where(ok, res, np.nan)
    return out


def quantile_field(field, q, group=None, G=None, method="linear", skipna=True):
    return quantile_sorted(sorted_groups(field, group, G), q, method, skipna)


def same(got, want):
    """equal with ``==`` (the sign of a zero is not pinned), NaN where NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
