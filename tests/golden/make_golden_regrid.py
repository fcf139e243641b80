"""Writes tests/golden/g24_regrid.npz: the fixture cases of the regridding tests, inputs plus what scipy makes of them.

The expected outputs come from scipy alone: one ``scipy.interpolate.interp1d(x, field, kind, axis, bounds_error=False,
fill_value=nan, assume_sorted=False)`` per spatial dimension, the first before the second, on the whole N-D field -- the calls
xarray's ``interp_like`` / ``interp`` make for 1-D orthogonal coordinates.  xarray itself is not installable where this project is
developed, so no golden can come from ``xarray.interp_like`` directly; the decomposition above is read off xarray's
``core/missing.py`` (``interp_func`` -> ``_interp1d`` per dimension).

Run from the repository root: ``python tests/golden/make_golden_regrid.py`` (needs scipy; written with 1.15.3).
"""
import os

import numpy as np
from scipy.interpolate import interp1d

HERE = os.path.dirname(os.path.abspath(__file__))


def scipy_regrid(src, src_y, src_x, dst_y, dst_x, kind):
    a = interp1d(src_y, src, kind=kind, axis=-2, bounds_error=False, fill_value=np.nan, assume_sorted=False)(dst_y)
    return interp1d(src_x, a, kind=kind, axis=-1, bounds_error=False, fill_value=np.nan, assume_sorted=False)(dst_x)


def cases():
    rng = np.random.default_rng(24)
    out = {}

    def add(name, src, sy, sx, dy, dx, kind="linear"):
        out[name] = dict(src=src, src_y=np.asarray(sy, float), src_x=np.asarray(sx, float), dst_y=np.asarray(dy, float),
                         dst_x=np.asarray(dx, float), kind=kind)

    # irregular ascending source, targets inside and outside the hull on all four sides
    sy, sx = np.sort(rng.uniform(30.0, 50.0, 5)), np.sort(rng.uniform(-120.0, -100.0, 6))
    src = 280.0 + 10.0 * rng.normal(size=(2, 5, 6))
    dy = np.concatenate([[sy[0] - 0.5], rng.uniform(sy[0], sy[-1], 5), [sy[-1] + 0.5]])
    dx = np.concatenate([[sx[0] - 1e-9], rng.uniform(sx[0], sx[-1], 6), [sx[-1] + 1e-9]])
    add("inside_outside", src, sy, sx, dy, dx)
    # descending source latitude (gridMET), ascending and shuffled targets
    add("descending_lat", src[:, ::-1, :].copy(), sy[::-1].copy(), sx, np.sort(dy), dx)
    add("shuffled_target", src[:, ::-1, :].copy(), sy[::-1].copy(), sx[::-1].copy(), rng.permutation(dy), rng.permutation(dx))
    # targets exactly on every source node (node 0 uses the interval above it, every other node the one below)
    add("exact_nodes", src, sy, sx, sy.copy(), sx.copy())
    # one NaN node at one time step: NaN wherever it is a bracket node, weight 0 on an exact hit included
    holed = src.copy()
    holed[1, 2, 3] = np.nan
    add("nan_node", holed, sy, sx, np.concatenate([sy, rng.uniform(sy[0], sy[-1], 3)]), np.concatenate([sx, rng.uniform(sx[0], sx[-1], 3)]))
    # float32 source
    add("float32", src.astype(np.float32), sy, sx, dy, dx)
    # nearest: midpoints go to the lower neighbour; regular grid so that the midpoints are exact
    ry, rx = np.arange(4.0), np.arange(0.0, 10.0, 2.0)
    rsrc = rng.normal(size=(2, 4, 5))
    add("nearest", rsrc, ry, rx, [-0.25, 0.0, 0.5, 0.75, 1.5, 2.5, 3.0, 3.25], [-1.0, 0.0, 1.0, 3.0, 4.5, 7.0, 8.0, 8.5], "nearest")
    add("nearest_descending", rsrc[:, ::-1, ::-1].copy(), ry[::-1].copy(), rx[::-1].copy(), [0.5, 1.5, 2.5, 2.9], [1.0, 3.0, 5.0, 7.0, 6.9], "nearest")
    return out


def main():
    flat = {}
    for name, c in cases().items():
        want = scipy_regrid(c["src"], c["src_y"], c["src_x"], c["dst_y"], c["dst_x"], c["kind"])
        for k in ("src", "src_y", "src_x", "dst_y", "dst_x"):
            flat[f"{name}.{k}"] = c[k]
        flat[f"{name}.kind"] = np.array(c["kind"])
        flat[f"{name}.want"] = want
    path = os.path.join(HERE, "g24_regrid.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes,", len(cases()), "cases")


if __name__ == "__main__":
    main()
