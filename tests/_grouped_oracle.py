"""NumPy restatement of the reference's GroupedRegressor(LinearRegression, PaddedDOYGrouper, ...) (grouping.py:12-138): per
group np.linalg.lstsq on centred data, like the lstsq inside sklearn's LinearRegression.  tests/test_grouped_host.py pins it to
the goldens recorded from the reference (tests/golden/g22_grouped.npz); the GPU tests use it on larger random grids."""
import numpy as np


def doy_keys(index):
    """(key [T] in [0, n), n): day of year - 1 and the largest day of year"""
    doy = np.asarray(index.dayofyear, dtype=np.int64)
    return doy - 1, int(doy.max())


def members(key, n, window):
    """[n, T] membership table of the circular windows, every sample once per group (grouping.py:125-134)"""
    dist = np.abs(np.arange(n)[:, None] - np.asarray(key)[None, :])
    return np.minimum(dist, n - dist) <= window


def fit(X, y, key, n, window):
    """X [T, F], y [T] -> coef [n, F], intercept [n], fitted [n] (False, NaN: a group without samples)"""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    F = X.shape[1]
    coef, icpt, fitted = np.full((n, F), np.nan), np.full(n, np.nan), np.zeros(n, dtype=bool)
    for g, m in enumerate(members(key, n, window)):
        if not m.any():
            continue
        xm, ym = X[m].mean(axis=0), y[m].mean()
        coef[g] = np.linalg.lstsq(X[m] - xm, y[m] - ym, rcond=None)[0]
        icpt[g] = ym - xm @ coef[g]
        fitted[g] = True
    return coef, icpt, fitted


def predict(coef, icpt, Xq, key_q):
    return icpt[key_q] + (coef[key_q] * np.asarray(Xq, dtype=np.float64)).sum(axis=1)


def grid(X, y, key, n, window, Xq, key_q, skip=()):
    """X [T, F, C], y [T, C], Xq [Tq, F, C] -> out [Tq, C], coef [n, F, C], intercept [n, C]; cells in ``skip`` stay NaN"""
    T, F, C = X.shape
    out, coef, icpt = np.full((Xq.shape[0], C), np.nan), np.full((n, F, C), np.nan), np.full((n, C), np.nan)
    for c in range(C):
        if c in skip:
            continue
        cf, ic, _ = fit(X[:, :, c], y[:, c], key, n, window)
        coef[:, :, c], icpt[:, c] = cf, ic
        out[:, c] = predict(cf, ic, Xq[:, :, c], key_q)
    return out, coef, icpt
