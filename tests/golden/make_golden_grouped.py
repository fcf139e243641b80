#!/usr/bin/env python
"""Generate tests/golden/g22_grouped.npz FROM THE REAL REFERENCE (skdownscale/pointwise_models/grouping.py).

Needs a checkout of the reference (``SKDOWNSCALE_REFERENCE``) + pandas + scikit-learn:

    python tests/golden/make_golden_grouped.py

``oracle/ref_shim.load()`` registers the package stubs; ``grouping.py`` then imports unmodified (no xarray needed).  The file
holds inputs and recorded results only: per case ``<c>_start`` / ``<c>_window`` / ``<c>_X`` / ``<c>_y``, the reference's
``<c>_pred`` and the ``coef_`` / ``intercept_`` of every group (``<c>_coef`` [n, n_targets, F], ``<c>_icpt`` [n, n_targets]).
"""
from __future__ import annotations

import importlib
import os
import sys
import warnings

import numpy as np
import pandas as pd
from sklearn.linear_model import LinearRegression, Ridge

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle")]

import ref_shim  # noqa: E402

warnings.filterwarnings("ignore")
ref_shim.load()
grouping = importlib.import_module("skdownscale.pointwise_models.grouping")


def predict_grouper(x):
    return x.dayofyear


def run(X, y, window, Xq=None, estimator=LinearRegression):
    m = grouping.GroupedRegressor(estimator, grouping.PaddedDOYGrouper, predict_grouper, fit_grouper_kwargs={"window": window})
    m.fit(X, y)
    try:
        pred = m.predict(X if Xq is None else Xq)
    except ValueError as e:  # recorded, not hidden: the caller asserts which cases may end here
        pred = str(e)
    keys = sorted(m.estimators_)
    assert keys == list(range(1, len(keys) + 1))
    coef = np.stack([np.asarray(m.estimators_[k].coef_, dtype=np.float64).reshape(y.shape[1], X.shape[1]) for k in keys])
    icpt = np.stack([np.asarray(m.estimators_[k].intercept_, dtype=np.float64).reshape(y.shape[1]) for k in keys])
    return m, pred, coef, icpt


def seasonal(rng, index, F, base=0.0, noise=3.0):
    doy = np.asarray(index.dayofyear)
    seas = 10.0 * np.sin(2 * np.pi * doy / 365.25)
    X = np.stack([base + seas + rng.normal(size=len(index)) * noise for _ in range(F)], axis=1)
    y = base + 2.0 + 1.1 * seas + 0.5 * X.sum(axis=1) / F + rng.normal(size=len(index))
    return X, y[:, None]


def store(out, c, start, window, X, y, pred, coef, icpt):
    out[f"{c}_start"], out[f"{c}_window"] = np.array(start), np.array(window)
    out[f"{c}_X"], out[f"{c}_y"], out[f"{c}_pred"], out[f"{c}_coef"], out[f"{c}_icpt"] = X, y, pred, coef, icpt


def frames(index, X, y):
    return (pd.DataFrame(X, index=index, columns=[f"f{i}" for i in range(X.shape[1])]),
            pd.DataFrame(y, index=index, columns=[f"t{i}" for i in range(y.shape[1])]))


def main():
    rng = np.random.default_rng(22)
    out = {}
    # 1: the reference's own test (test/test_grouping.py): y = X + 2
    start, n, w = "2019-01-01", 1234, 5
    index = pd.date_range(start, periods=n)
    X = rng.random((n, 1))
    y = X + 2.0
    Xd, yd = frames(index, X, y)
    _, pred, coef, icpt = run(Xd, yd, w)
    sizes = [len(v) for v in grouping.PaddedDOYGrouper(index, w).groups.values()]
    assert (min(sizes), max(sizes), len(sizes)) == (31, 44, 366), (min(sizes), max(sizes), len(sizes))
    store(out, "c1", start, w, X, y, pred, coef, icpt)
    # 10: the same data through Ridge() (the host loop of the meta-estimator).  With the scikit-learn this file was generated
    # with, Ridge predicts (k,) for a one-column DataFrame y, so the reference's fit completes and its predict fails on
    # ``result[inds, ...] = ...`` (grouping.py:101); the fitted numbers and the message are recorded
    _, pred, coef, icpt = run(Xd, yd, w, estimator=Ridge)
    assert isinstance(pred, str) and pred.startswith("shape mismatch"), pred
    out["c10_error"], out["c10_coef"], out["c10_icpt"] = np.array(pred), coef, icpt
    # 2 .. 5: noisy seasonal data
    for c, start, n, w, F, base in (("c2", "1980-01-01", 4000, 15, 2, 280.0), ("c3", "2019-01-01", 300, 5, 1, 280.0),
                                    ("c4", "2019-03-01", 800, 5, 1, 280.0), ("c5", "2001-06-01", 2000, 200, 1, 280.0)):
        index = pd.date_range(start, periods=n)
        X, y = seasonal(rng, index, F, base)
        Xd, yd = frames(index, X, y)
        _, pred, coef, icpt = run(Xd, yd, w)
        store(out, c, start, w, X, y, pred, coef, icpt)
    sizes = [len(v) for v in grouping.PaddedDOYGrouper(pd.date_range("1980-01-01", periods=4000), 15).groups.values()]
    assert (min(sizes), max(sizes)) == (315, 341), (min(sizes), max(sizes))
    assert len(grouping.PaddedDOYGrouper(pd.date_range("2019-01-01", periods=300), 5).groups) == 300
    # 6: a constant feature next to a live one, two targets
    start, n, w = "2001-01-01", 1500, 5
    index = pd.date_range(start, periods=n)
    a = rng.normal(size=n)
    X = np.stack([a, np.full(n, 3.5)], axis=1)
    y = np.stack([2 * a + 1 + rng.normal(size=n) * 0.1, -a + rng.normal(size=n) * 0.1], axis=1)
    Xd, yd = frames(index, X, y)
    _, pred, coef, icpt = run(Xd, yd, w)
    assert pred.shape == (n, 2) and np.all(coef[:, :, 1] == 0.0)
    store(out, "c6", start, w, X, y, pred, coef, icpt)
    # 10b: case 6 through Ridge(): two target columns predict (k, 2), so the reference completes
    _, pred, coef, icpt = run(Xd, yd, w, estimator=Ridge)
    assert pred.shape == (n, 2)
    out["c10b_pred"], out["c10b_coef"], out["c10b_icpt"] = pred, coef, icpt
    # 7: predict on another period; fit 2019, predict 2020 -> KeyError: 366
    start, n, w = "2001-01-01", 1461, 7
    index = pd.date_range(start, periods=n)
    X, y = seasonal(rng, index, 1, 5.0)
    index_q = pd.date_range("2031-05-17", periods=500)
    Xq, _ = seasonal(rng, index_q, 1, 6.0)
    Xd, yd = frames(index, X, y)
    _, pred, coef, icpt = run(Xd, yd, w, Xq=pd.DataFrame(Xq, index=index_q, columns=["f0"]))
    store(out, "c7", start, w, X, y, pred, coef, icpt)
    out["c7_qstart"], out["c7_Xq"] = np.array("2031-05-17"), Xq
    index = pd.date_range("2019-01-01", periods=365)
    X, y = seasonal(rng, index, 1)
    Xd, yd = frames(index, X, y)
    m, _, _, _ = run(Xd, yd, 5)
    index_q = pd.date_range("2020-01-01", periods=366)
    try:
        m.predict(pd.DataFrame(np.zeros((366, 1)), index=index_q, columns=["f0"]))
        raise AssertionError("the reference predicted a day it has no model for")
    except KeyError as e:
        out["c7_keyerror"] = np.array(str(e))
    # 8: PaddedDOYGrouper.groups
    for i, (start, n, w) in enumerate((("1980-01-01", 3000, 2), ("2019-03-01", 800, 5), ("2003-07-15", 1700, 30))):
        groups = grouping.PaddedDOYGrouper(pd.date_range(start, periods=n), w).groups
        out[f"c8_{i}_start"], out[f"c8_{i}_n"], out[f"c8_{i}_window"] = np.array(start), np.array(n), np.array(w)
        out[f"c8_{i}_keys"] = np.array(list(groups), dtype=np.int64)
        out[f"c8_{i}_sizes"] = np.array([len(v) for v in groups.values()], dtype=np.int64)
        out[f"c8_{i}_inds"] = np.concatenate(list(groups.values())).astype(np.int32)
    # 9: a small grid, cell by cell like core.py:86-96 (cell 2 is masked: its first sample is NaN)
    start, n, w, C, F = "1990-01-01", 1100, 10, 6, 2
    index = pd.date_range(start, periods=n)
    Xg, yg = np.empty((n, F, C)), np.empty((n, C))
    pred_g, coef_g, icpt_g = np.full((n, C), np.nan), np.full((366, F, C), np.nan), np.full((366, C), np.nan)
    for c in range(C):
        X, y = seasonal(rng, index, F, 270.0 + c)
        Xg[:, :, c], yg[:, c] = X, y[:, 0]
        if c == 2:
            Xg[0, :, c] = np.nan
            continue
        Xd, yd = frames(index, X, y)
        _, pred, coef, icpt = run(Xd, yd, w)
        pred_g[:, c], coef_g[:, :, c], icpt_g[:, c] = pred[:, 0], coef[:, 0, :], icpt[:, 0]
    store(out, "c9", start, w, Xg, yg, pred_g, coef_g, icpt_g)
    path = os.path.join(HERE, "g22_grouped.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
