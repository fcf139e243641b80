"""Writes tests/golden/g26_groupby.npz: the fixture cases of the groupby tests, inputs plus what pandas and the reference make of them.

Pandas cases: ``pd.DataFrame(values, index=time).groupby(key).mean()`` / ``.sum()``, the calls the reference's BCSD classes make
(``df.groupby(MONTH_GROUPER).mean()``), on 3 years of daily data (1 096 days, one leap year) by 6 cells with 5 % NaN.  A float32 case is
expected on the widened values (the engine returns float64 whatever the source).

Reference cases, from the reference itself through oracle/ref_shim.py (``SKDOWNSCALE_REFERENCE``): ``BcsdTemperature().fit(X, y)`` per
cell gives ``y_climo_`` and ``_x_climo`` [12, 4], and ``_remove_climatology(X, _x_climo)`` gives [T, 4].

Only data goes into the file.  Run from the repository root: ``python tests/golden/make_golden_groupby.py`` (written with pandas 2.3.3).
"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

KEYS = ("month", "dayofyear", "year", "season", "month_grouper")
SEASON = np.array(["DJF", "MAM", "JJA", "SON"])


def pandas_key(time, key):
    if key == "season":
        return SEASON[(time.month.to_numpy() % 12) // 3]
    if key == "month_grouper":
        return lambda x: x.month  # the reference's MONTH_GROUPER
    return getattr(time, key)


def main():
    rng = np.random.default_rng(26)
    time = pd.date_range("2003-01-01", "2005-12-31", freq="D")  # 2004 is a leap year: day of year 366 has one sample
    assert len(time) == 1096
    values = 285.0 + 10.0 * rng.normal(size=(len(time), 6))
    values[rng.random(values.shape) < 0.05] = np.nan
    values[time.month == 2, 5] = np.nan  # a cell with an all-NaN group (February; seasons and years keep samples)
    flat = {"time": time.values.astype("datetime64[ns]"), "values": values, "values32": values.astype(np.float32)}
    for name, v in (("f64", values), ("f32", values.astype(np.float32))):
        frame = pd.DataFrame(v.astype(np.float64), index=time)
        for key in KEYS:
            g = frame.groupby(pandas_key(time, key))
            mean = g.mean()
            labels = np.asarray(mean.index)
            flat[f"{name}.{key}.labels"] = labels.astype(str) if labels.dtype == object else labels  # (no pickled objects in the file)
            flat[f"{name}.{key}.mean"] = mean.to_numpy(dtype=np.float64)
            flat[f"{name}.{key}.sum"] = g.sum().to_numpy(dtype=np.float64)

    import ref_shim

    ref = ref_shim.load()
    T, C = 730, 4
    rtime = pd.date_range("2001-01-01", periods=T, freq="D")
    season = 8.0 * np.cos(2 * np.pi * (rtime.dayofyear.to_numpy() - 200) / 365.25)[:, None]
    X = 283.0 + season + 3.0 * rng.normal(size=(T, C))
    y = 285.0 + 1.1 * season + 3.0 * rng.normal(size=(T, C))
    y_climo, x_climo, anoms = np.empty((12, C)), np.empty((12, C)), np.empty((T, C))
    for c in range(C):
        Xc, yc = pd.DataFrame({"x": X[:, c]}, index=rtime), pd.DataFrame({"y": y[:, c]}, index=rtime)
        est = ref.BcsdTemperature().fit(Xc, yc)
        assert list(est.y_climo_.index) == list(range(1, 13))
        y_climo[:, c] = est.y_climo_.to_numpy().ravel()
        x_climo[:, c] = est._x_climo.to_numpy().ravel()
        anoms[:, c] = est._remove_climatology(Xc, est._x_climo).to_numpy().ravel()
    flat.update({"ref.time": rtime.values.astype("datetime64[ns]"), "ref.X": X, "ref.y": y, "ref.y_climo": y_climo, "ref.x_climo": x_climo,
                 "ref.anoms": anoms})
    path = os.path.join(HERE, "g26_groupby.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes, pandas", pd.__version__)


if __name__ == "__main__":
    main()
