"""Writes tests/golden/g27_rolling.npz: the fixture cases of the rolling tests, inputs plus what pandas makes of them.

Fields, T = 400 days by 6 cells: ``tas`` -- temperatures with 5 % NaN, and in cell 5 a run of 40 NaN (longer than every window here)
--, ``pr`` -- zero-inflated precipitation (60 % dry days, gamma amounts) with 3 % NaN -- and ``tas32``, a float32 copy of ``tas``
whose results are expected on the widened values (the engine returns float64 whatever the source).

Cases: ``pd.DataFrame(x).rolling(w, center=..., min_periods=...).mean()`` / ``.sum()`` / ``.var(ddof)`` / ``.std(ddof)``, among them
the reference's own three calls -- ``rolling(9, center=True, min_periods=1).mean()`` (bcsd.py), ``rolling(31, center=True).mean()``
and ``.std()`` (zscore.py) --, trailing and centred windows, even windows, ``min_periods=0`` and ``ddof=0``.  A wrap case is pandas on
the series padded by ``w // 2`` rows from its other end, cut back to its length (zscore.py pads its day-of-year axis that way); those
run on the first 366 rows.

Only data goes into the file.  Run from the repository root: ``python tests/golden/make_golden_rolling.py`` (written with pandas 2.3.3).
"""
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))

# (field, window, op, center, min_periods (None: pandas' default, the window), ddof, wrap); few enough to keep the file small
CASES = [
    # the reference's own three calls
    ("tas", 9, "mean", True, 1, 1, False), ("tas", 31, "mean", True, None, 1, False), ("tas", 31, "std", True, None, 1, False),
    # trailing windows: w = 1, even and odd, an n-day accumulation
    ("tas", 1, "mean", False, None, 1, False), ("pr", 1, "sum", False, 1, 1, False), ("tas", 2, "mean", False, None, 1, False),
    ("pr", 5, "mean", False, None, 1, False), ("tas", 9, "var", False, 1, 1, False), ("tas", 30, "sum", False, 3, 1, False),
    ("pr", 30, "sum", False, 1, 1, False), ("pr", 31, "std", False, 3, 1, False),
    # centred windows: even and odd, w = 1 (no variance of one sample)
    ("tas", 1, "var", True, 1, 1, False), ("tas", 2, "std", True, 1, 1, False), ("pr", 2, "sum", True, 1, 1, False),
    ("tas", 30, "mean", True, 3, 1, False), ("pr", 30, "var", True, None, 1, False), ("pr", 9, "mean", True, 1, 1, False),
    ("pr", 31, "var", True, 3, 1, False), ("pr", 5, "std", True, None, 1, False),
    # min_periods=0: the sum of a window without a sample (the run of NaN) is 0.0
    ("tas", 31, "sum", True, 0, 1, False), ("tas", 31, "mean", False, 0, 1, False), ("pr", 2, "var", True, 0, 1, False),
    ("tas", 9, "std", False, 0, 1, False),
    # ddof=0
    ("tas", 31, "var", True, 2, 0, False), ("pr", 30, "std", True, 2, 0, False), ("tas", 2, "std", False, 1, 0, False),
    # float32
    ("tas32", 9, "mean", True, 1, 1, False), ("tas32", 30, "std", True, 1, 1, False), ("tas32", 31, "sum", False, 1, 1, False),
    ("tas32", 5, "var", False, None, 1, False),
    # wrap: pandas on the padded series
    ("tas366", 31, "mean", True, None, 1, True), ("tas366", 31, "std", True, 1, 1, True), ("pr366", 31, "sum", True, 1, 1, True),
    ("pr366", 30, "var", True, 1, 1, True), ("tas366", 9, "mean", True, 1, 1, True)]


def pandas_rolling(x, window, op, center, min_periods, ddof, wrap):
    x = np.asarray(x, dtype=np.float64)
    T, pad = len(x), window // 2
    if wrap:
        assert center and pad > 0
        x = np.concatenate([x[-pad:], x, x[:pad]])
    r = pd.DataFrame(x).rolling(window, center=center, min_periods=min_periods)
    res = (getattr(r, op)(ddof=ddof) if op in ("var", "std") else getattr(r, op)()).to_numpy(dtype=np.float64)
    return res[pad:pad + T] if wrap else res


def main():
    rng = np.random.default_rng(27)
    T, C = 400, 6
    day = np.arange(T)
    tas = 285.0 + 10.0 * np.sin(2 * np.pi * day / 365.25)[:, None] + 3.0 * rng.normal(size=(T, C))
    tas[rng.random((T, C)) < 0.05] = np.nan
    tas[150:190, 5] = np.nan
    pr = np.where(rng.random((T, C)) < 0.6, 0.0, rng.gamma(0.7, 8.0, size=(T, C)))
    pr[rng.random((T, C)) < 0.03] = np.nan
    fields = {"tas": tas, "pr": pr, "tas32": tas.astype(np.float32), "tas366": tas[:366].copy(), "pr366": pr[:366].copy()}
    flat = dict(fields)
    keys = []
    for f, w, op, center, mp, ddof, wrap in CASES:
        key = f"{f}.w{w}.{op}.{'c' if center else 't'}.mp{'d' if mp is None else mp}.ddof{ddof}{'.wrap' if wrap else ''}"
        assert key not in flat, key
        flat[key] = pandas_rolling(fields[f], w, op, center, mp, ddof, wrap)
        keys.append(key)
    flat["case.key"] = np.array(keys)
    flat["case.field"] = np.array([c[0] for c in CASES])
    flat["case.window"] = np.array([c[1] for c in CASES], dtype=np.int64)
    flat["case.op"] = np.array([c[2] for c in CASES])
    flat["case.center"] = np.array([c[3] for c in CASES])
    flat["case.min_periods"] = np.array([-1 if c[4] is None else c[4] for c in CASES], dtype=np.int64)
    flat["case.ddof"] = np.array([c[5] for c in CASES], dtype=np.int64)
    flat["case.wrap"] = np.array([c[6] for c in CASES])
    path = os.path.join(HERE, "g27_rolling.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases, pandas", pd.__version__)


if __name__ == "__main__":
    main()
