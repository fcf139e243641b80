#!/usr/bin/env python
"""Generate tests/golden/g23_arrm.npz: breakpoints FROM THE REAL REFERENCE (skdownscale/pointwise_models/arrm.py).

Needs a checkout of the reference (``SKDOWNSCALE_REFERENCE``) + scikit-learn + scipy:

    python tests/golden/make_golden_arrm.py [--time]

``oracle/ref_shim.load()`` registers the package stubs; ``arrm.py`` then imports unmodified (pwlf is optional there).
g23_arrm.npz holds per case ``<c>``: ``<c>_mb`` (max_breakpoints), the reference's ``<c>_breaks`` [B, C] and their positions in
the sorted X ``<c>_index`` [B, C]; from the NumPy restatement (tests/_arrm_oracle.py, whose picks must equal the reference's on
every cell): ``<c>_margin`` [C], ``<c>_beta`` [B, C], ``<c>_ssr`` [C], ``<c>_cond`` [C] (and ``<c>_Xq`` [Tq, C] where the queries
are not the training data).  No committed file may exceed 1 MiB, so the fields of a case live in files of their own:
g23_arrm_<c>_in.npz holds ``X`` / ``y`` [T, C] as float32 (the inputs are float32 values, widened exactly), g23_arrm_<c>_r2.npz
the restatement's ``r2`` [T, C]; the expected predictions are ``design(Xq) @ beta`` of the stored beta, formed by the tests.
pwlf is not installed, so beta is the documented model solved by scipy.linalg.lstsq (gelsd), not a pwlf run.  ``--time`` prints
the reference's per-cell time of arrm_breakpoints at T = 14 600.

g24_arrm_breaks.npz (``main_breaks``, a seed of its own) holds the same per case for the break counts, series lengths and window
widths that g23 leaves out, with ``<c>_margin_computed`` [C] (the margin without the picks on the sentinels 1.0 / 2.0),
``<c>_start2`` [C] (the start of the lower loop), ``<c>_sentinel`` [C] (picks on a sentinel) and ``<c>_raises`` [C]: the real
reference raised ``ValueError: attempt to get argmin of an empty sequence`` on that cell, whose other arrays hold NaN / -1.  The
inputs of all its cases are in g24_arrm_breaks_in.npz (``<c>_X`` / ``<c>_y``), the r2 series in g24_arrm_breaks_r2.npz (``<c>_r2``).
"""
from __future__ import annotations

import importlib
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import ref_shim  # noqa: E402
import _arrm_oracle as ao  # noqa: E402

warnings.filterwarnings("ignore")
ref_shim.load()
arrm = importlib.import_module("skdownscale.pointwise_models.arrm")

CELLS = 67
MARGIN = 1e-6  # cells below it are left out of the break-index assertion of the GPU test
MAX_EXCLUDED = 0.05
EMPTY_ARGMIN = "attempt to get argmin of an empty sequence"  # the reference on a cell whose lower range r2[:0] is empty


def gaussian(rng, T, C, offset=15.0, spread=8.0):
    X = offset + spread * rng.normal(size=(T, C))
    y = 13.0 + 0.9 * X + 0.05 * X * X + 3.0 * rng.normal(size=(T, C))
    return X, y


def half_zero_gamma(rng, T, C):
    X = 15.0 + 8.0 * rng.normal(size=(T, C))
    y = rng.gamma(0.8, 4.0, size=(T, C))
    y[rng.random(size=(T, C)) < 0.5] = 0.0
    return X, y


def offset_small_spread(rng, T, C):
    X = 288.0 + 0.05 * rng.normal(size=(T, C))
    g = (X - 288.0) / 0.05
    y = 13.0 + 0.9 * g + 0.05 * g * g + 0.3 * rng.normal(size=(T, C))
    return X, y


def f32(a):
    """float32 values as float64: stored at half the size, widened exactly by the tests"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def reference_indices(x, y, mb):
    """the real arrm_breakpoints; its picks recovered as positions in the sorted x (ties: the oracle's, checked equal in value)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return arrm.arrm_breakpoints(x.reshape(-1, 1), y, 0.05, mb)


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < (1 << 20), f"{name}: {os.path.getsize(path)} bytes"


def case(out, name, X, y, mb, Xq=None):
    X, y = f32(X), f32(y)
    T, C = X.shape
    B = 2 * (mb // 2)
    Xq = X if Xq is None else f32(Xq)
    rec = {k: [] for k in ("breaks", "index", "r2", "margin", "beta", "ssr", "cond", "pred")}
    for c in range(C):
        ref = reference_indices(X[:, c], y[:, c], mb)
        o = ao.breakpoints(X[:, c], y[:, c], 0.05, mb)
        xs = np.sort(X[:, c])
        assert ref.shape == (B,) and np.array_equal(ref, xs[o["index"]]), f"{name} cell {c}: the restatement's picks differ from the reference"
        beta, ssr, cond = ao.fit_on_breaks(X[:, c], y[:, c], ref)
        for k, v in (("breaks", ref), ("index", o["index"]), ("r2", o["r2"]), ("margin", o["margin"]), ("beta", beta), ("ssr", ssr),
                     ("cond", cond), ("pred", ao.predict(Xq[:, c], ref, beta))):
            rec[k].append(v)
    margin = np.asarray(rec["margin"])
    excluded = float((margin < MARGIN).mean())
    assert excluded <= MAX_EXCLUDED, f"{name}: {excluded:.1%} of the cells have an argmin margin below {MARGIN}"
    out[f"{name}_mb"] = np.int64(mb)
    save(f"g23_arrm_{name}_in.npz", X=X.astype(np.float32), y=y.astype(np.float32))
    r2 = np.stack(rec["r2"], axis=1)
    save(f"g23_arrm_{name}_r2.npz", r2=r2)
    if Xq is not X:
        out[f"{name}_Xq"] = Xq.astype(np.float32)
    for k in ("breaks", "beta"):
        out[f"{name}_{k}"] = np.stack(rec[k], axis=1)
    out[f"{name}_index"] = np.stack(rec["index"], axis=1).astype(np.int32)
    for k in ("margin", "ssr", "cond"):
        out[f"{name}_{k}"] = np.asarray(rec[k])
    dup = sum(len(np.unique(b)) < len(b) for b in rec["breaks"])
    print(f"{name}: T={T} C={C} mb={mb} excluded={excluded:.3f} duplicate-break cells={dup} nan-r2 cells="
          f"{int(np.isnan(r2).any(axis=0).sum())} cond max={max(rec['cond']):.3g}")


def case24(out, fields, series, name, X, y, mb):
    """one case of g24_arrm_breaks*.npz: as ``case`` with the cells on which the real reference raises recorded (``raises``; their
    other arrays hold NaN / -1), ``start2`` per cell, and the share of left-out cells taken on ``margin_computed``"""
    X, y = f32(X), f32(y)
    T, C = X.shape
    B = 2 * (mb // 2)
    keys = ("breaks", "index", "r2", "margin", "margin_computed", "beta", "ssr", "cond", "raises", "start2", "sentinel")
    rec = {k: [] for k in keys}
    for c in range(C):
        try:
            ref = reference_indices(X[:, c], y[:, c], mb)
        except ValueError as e:
            assert str(e) == EMPTY_ARGMIN, f"{name} cell {c}: the reference raised {e!r}"
            try:
                ao.breakpoints(X[:, c], y[:, c], 0.05, mb)
            except ValueError as e2:
                assert str(e2) == EMPTY_ARGMIN
            else:
                raise AssertionError(f"{name} cell {c}: the reference raises, the restatement does not")
            nan = np.full(B, np.nan)
            for k, v in (("breaks", nan), ("index", np.full(B, -1)), ("r2", np.full(T, np.nan)), ("margin", np.nan), ("margin_computed", np.nan),
                         ("beta", nan), ("ssr", np.nan), ("cond", np.nan), ("raises", True), ("start2", 0), ("sentinel", -1)):
                rec[k].append(v)
            continue
        o = ao.breakpoints(X[:, c], y[:, c], 0.05, mb)
        xs = np.sort(X[:, c])
        assert ref.shape == (B,) and np.array_equal(ref, xs[o["index"]]), f"{name} cell {c}: the restatement's picks differ from the reference"
        assert o["start2"] != 0
        beta, ssr, cond = ao.fit_on_breaks(X[:, c], y[:, c], ref)
        for k, v in (("breaks", ref), ("index", o["index"]), ("r2", o["r2"]), ("margin", o["margin"]), ("margin_computed", o["margin_computed"]),
                     ("beta", beta), ("ssr", ssr), ("cond", cond), ("raises", False), ("start2", o["start2"]), ("sentinel", o["sentinel_picks"])):
            rec[k].append(v)
    raises = np.asarray(rec["raises"], dtype=bool)
    assert not raises.all()
    excluded = float((np.asarray(rec["margin_computed"])[~raises] < MARGIN).mean())
    assert excluded <= MAX_EXCLUDED, f"{name}: {excluded:.1%} of the cells have an argmin margin below {MARGIN}"
    out[f"{name}_mb"] = np.int64(mb)
    fields[f"{name}_X"], fields[f"{name}_y"] = X.astype(np.float32), y.astype(np.float32)
    series[f"{name}_r2"] = np.stack(rec["r2"], axis=1)
    for k in ("breaks", "beta"):
        out[f"{name}_{k}"] = np.stack(rec[k], axis=1)
    out[f"{name}_index"] = np.stack(rec["index"], axis=1).astype(np.int32)
    for k in ("margin", "margin_computed", "ssr", "cond"):
        out[f"{name}_{k}"] = np.asarray(rec[k], dtype=np.float64)
    out[f"{name}_raises"] = raises
    out[f"{name}_start2"] = np.asarray(rec["start2"], dtype=np.int32)
    out[f"{name}_sentinel"] = np.asarray(rec["sentinel"], dtype=np.int32)
    index = out[f"{name}_index"][:, ~raises]
    triple = int(sum(np.unique(index[:, k], return_counts=True)[1].max() >= 3 for k in range(index.shape[1])))
    print(f"{name}: T={T} C={C} mb={mb} raising={int(raises.sum())} excluded={excluded:.3f} start2<0 cells={int((out[f'{name}_start2'] < 0).sum())} "
          f"sentinel-pick cells={int((out[f'{name}_sentinel'] > 0).sum())} cells with 3 equal breaks={triple} nan-r2 cells="
          f"{int(np.isnan(series[f'{name}_r2'][:, ~raises]).any(axis=0).sum())} cond max={np.nanmax(out[f'{name}_cond']):.3g}")
    return dict(raises=raises, start2=out[f"{name}_start2"], sentinel=out[f"{name}_sentinel"], triple=triple)


# (max_breakpoints, T, cells) per case of g24: tests/_arrm_oracle.py lists the names
G24 = [("short50_mb8", 50, 8, 24), ("short50_mb16", 50, 16, 24), ("short51_mb12", 51, 12, 24), ("short59_mb17", 59, 17, 24),
       ("short64_mb16", 64, 16, 24), ("w210_mb8", 210, 8, 16), ("w230_mb12", 230, 12, 16), ("w250_mb16", 250, 16, 16),
       ("w270_mb9", 270, 9, 16), ("w220_mb8", 220, 8, 16), ("w260_mb8", 260, 8, 16), ("mb2_300", 300, 2, 16), ("mb3_300", 300, 3, 16),
       ("mb17_1000", 1000, 17, 16), ("quant300_mb8", 300, 8, 16)]


def main_breaks():
    """g24_arrm_breaks*.npz: every break count, short series (the wrap of the mask, a negative start of the lower loop, picks on
    the sentinels, cells on which the reference raises), half-to-even and odd window widths, quantised predictors"""
    rng = np.random.default_rng(2402)
    out, fields, series, short = {}, {}, {}, []
    for name, T, mb, C in G24:
        X, y = gaussian(rng, T, C)
        if name.startswith("quant"):
            X = 2.0 * np.round(X / 2.0)
        info = case24(out, fields, series, name, X, y, mb)
        if name.startswith("quant"):
            assert np.isnan(series[f"{name}_r2"]).any(axis=0).all()
        if name.startswith("short"):
            assert info["raises"].mean() <= 0.5, f"{name}: more than half of the cells raise"
            short.append(info)
    assert sum(int(i["raises"].sum()) for i in short) >= 1, "no raising cell in the short cases"
    assert any((i["start2"] < 0).any() for i in short), "no cell with a negative start of the lower loop"
    assert any((i["sentinel"] > 0).any() for i in short), "no cell with a pick on a sentinel"
    assert sum(i["triple"] for i in short) >= 1, "no cell with three or more equal breaks"
    out["cases"] = np.array([g[0] for g in G24])
    save("g24_arrm_breaks.npz", **out)
    save("g24_arrm_breaks_in.npz", **fields)
    save("g24_arrm_breaks_r2.npz", **series)


def main():
    rng = np.random.default_rng(2301)
    out = {}
    for T in (200, 365, 500, 1200):
        case(out, f"gauss{T}", *gaussian(rng, T, CELLS), 7)
    case(out, "halfzero600", *half_zero_gamma(rng, 600, CELLS), 7)
    case(out, "offset288", *offset_small_spread(rng, 400, CELLS), 7)
    case(out, "mb4", *gaussian(rng, 300, CELLS), 4)
    X, y = gaussian(rng, 260, CELLS)
    Xq = np.concatenate([X.min(axis=0)[None] - 20.0, 15.0 + 8.0 * rng.normal(size=(99, CELLS)), X.max(axis=0)[None] + 20.0])
    case(out, "query101", X, y, 7, Xq=Xq)
    out["cases"] = np.array(["gauss200", "gauss365", "gauss500", "gauss1200", "halfzero600", "offset288", "mb4", "query101"])
    save("g23_arrm.npz", **out)
    main_breaks()
    if "--time" in sys.argv:
        X, y = gaussian(np.random.default_rng(5), 14600, 3)
        t0 = time.perf_counter()
        for c in range(3):
            reference_indices(X[:, c], y[:, c], 7)
        print(f"reference arrm_breakpoints, T = 14600, one core: {(time.perf_counter() - t0) / 3:.3f} s per cell")


if __name__ == "__main__":
    main()
