"""NumPy + pandas restatement of ZScoreRegressor (skdownscale/pointwise_models/zscore.py) for the tests.

The reference needs xarray for its fit; this helper spells the same steps out with NumPy instead:
  1. pivot the samples into a [day of year, year] grid (missing where a year lacks a day; two samples on one cell fail),
  2. extend the day axis with its last ceil(w/2) and first w//2 rows (Python slices, clipped to the grid),
  3. centred windows of width w -- w//2 missing rows in front, (w-1)//2 behind --, mean and population std of every
     non-missing entry over (window, year),
  4. keep the positions n .. L-n-1, n = w//2 + 1, labelled with their day of year.
Predict calls pandas' own rolling mean / std and positional .iloc, so pandas pins those rules.
"""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd
from numpy.lib.stride_tricks import sliding_window_view


def fit_stats(values, index, w):
    """(labels, mean, std) of one series over the kept day windows"""
    values = np.asarray(values, dtype=np.float64)
    doy, yr = np.asarray(index.dayofyear), np.asarray(index.year)
    days, years = np.unique(doy), np.unique(yr)
    di, yi = np.searchsorted(days, doy), np.searchsorted(years, yr)
    if len(set(zip(di.tolist(), yi.tolist()))) != len(values):
        raise ValueError("two samples on one (year, day of year)")
    grid = np.full((len(days), len(years)), np.nan)
    grid[di, yi] = values
    ext = np.concatenate([grid[-w // 2:], grid, grid[:w // 2]])
    lab = np.concatenate([days[-w // 2:], days, days[:w // 2]])
    padded = np.concatenate([np.full((w // 2, len(years)), np.nan), ext, np.full(((w - 1) // 2, len(years)), np.nan)])
    win = sliding_window_view(padded, w, axis=0)  # [L, years, w]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # empty windows -> NaN
        mean = np.nanmean(win, axis=(1, 2))
        std = np.nanstd(win, axis=(1, 2))
    n = w // 2 + 1
    L = len(ext)
    return lab[n:L - n], mean[n:L - n], std[n:L - n]


def fit(X, y, index, w=31):
    """dict of pd.Series: X_mean, X_std, y_mean, y_std, shift, scale (index 'day')"""
    lab, xm, xs = fit_stats(X, index, w)
    _, ym, ys = fit_stats(y, index, w)
    idx = pd.Index(lab.astype(np.int64), name="day")
    out = {k: pd.Series(v, index=idx) for k, v in (("X_mean", xm), ("X_std", xs), ("y_mean", ym), ("y_std", ys))}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["shift"] = out["y_mean"] - out["X_mean"]
        out["scale"] = out["y_std"] / out["X_std"]
    return out


def predict(Xp, index, shift, scale, w=31):
    """(out, dict meani / stdi / meanf / stdf) as pd.Series on ``index``"""
    s = pd.Series(np.asarray(Xp, dtype=np.float64), index=index)
    mean = s.rolling(w, center=True).mean()
    std = s.rolling(w, center=True).std()
    z = (s - mean) / std
    inds = np.arange(len(s)) % min(len(s), 364)
    sh = pd.Series(shift).iloc[inds]
    sc = pd.Series(scale).iloc[inds]
    sh.index = index
    sc.index = index
    meanf = mean + sh
    stdf = std * sc
    return z * stdf + meanf, {"meani": mean, "stdi": std, "meanf": meanf, "stdf": stdf}
