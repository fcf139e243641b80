"""Writes tests/golden/g25_resample.npz: the fixture cases of the resampling tests, inputs plus what pandas makes of them.

The expected outputs come from pandas alone: ``pd.DataFrame(values, index=time).resample(rule).mean()`` / ``.sum()``, the calls the
reference's BCSD examples make, with the bin sizes of ``.size()`` beside them.  A float32 case is expected on the widened values (the
engine returns float64 whatever the source; pandas would keep float32).

Run from the repository root: ``python tests/golden/make_golden_resample.py`` (written with pandas 2.3.3).
"""
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    rng = np.random.default_rng(25)
    out = {}

    def add(name, time, values, rule):
        out[name] = dict(time=pd.DatetimeIndex(time), values=values, rule=rule)

    # 330 days of daily data starting mid-month with a 70-day gap: 14 'MS' bins, 2 of them empty (June and July)
    days = pd.date_range("2001-01-17", periods=400, freq="D")
    gap = days[:130].append(days[200:])
    tas = 285.0 + 10.0 * rng.normal(size=(len(gap), 5))
    add("ms_gap", gap, tas, "MS")
    add("me", days[:200], 285.0 + 10.0 * rng.normal(size=(200, 3)), "ME")
    add("ys", pd.date_range("1999-11-03", periods=500, freq="D"), rng.gamma(0.7, 4.0, size=(500, 2)), "YS")
    add("7d", days[:100], rng.normal(size=(100, 8)), "7D")
    add("1d_subdaily", pd.date_range("2001-03-01 06:00", periods=150, freq="6h"), 280.0 + rng.normal(size=(150, 4)), "1D")
    # a NaN run inside a bin (some samples left) and an all-NaN bin, next to untouched cells
    holed = 285.0 + 10.0 * rng.normal(size=(120, 4))
    holed[10:17, 0] = np.nan     # inside January
    holed[31:59, 1] = np.nan     # all of February
    holed[59:90, 2] = np.nan     # all of March
    holed[100, 2] = np.nan
    add("nan_run_and_all_nan_bin", pd.date_range("2001-01-01", periods=120, freq="D"), holed, "MS")
    # float32 input: expected on the widened values
    add("float32", days[:150], (285.0 + 10.0 * rng.normal(size=(150, 6))).astype(np.float32), "MS")
    return out


def main():
    flat = {}
    for name, c in cases().items():
        frame = pd.DataFrame(c["values"].astype(np.float64), index=c["time"])
        r = frame.resample(c["rule"])
        size = r.size()
        flat[f"{name}.time"] = c["time"].values.astype("datetime64[ns]")
        flat[f"{name}.values"] = c["values"]
        flat[f"{name}.rule"] = np.array(c["rule"])
        flat[f"{name}.labels"] = size.index.values.astype("datetime64[ns]")
        flat[f"{name}.size"] = size.to_numpy(dtype=np.int64)
        flat[f"{name}.mean"] = r.mean().to_numpy(dtype=np.float64)
        flat[f"{name}.sum"] = r.sum().to_numpy(dtype=np.float64)
    path = os.path.join(HERE, "g25_resample.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes,", len(cases()), "cases, pandas", pd.__version__)


if __name__ == "__main__":
    main()
