"""NumPy restatement of the regridding rule (csrc/sd_regrid_plan.h, sd_regrid.hip): what xarray's ``interp_like`` evaluates for 1-D
coordinates, one ``scipy.interpolate.interp1d(bounds_error=False, fill_value=nan, assume_sorted=False)`` per dimension, the first
spatial dim of the field before the second.  tests/test_regrid_host.py pins it to scipy bit for bit."""
import numpy as np


def _ascending(x, v, axis):
    x = np.asarray(x, dtype=np.float64)
    if x[-1] < x[0]:  # interp1d(assume_sorted=False) sorts the coordinate and the values with it
        return x[::-1], np.flip(v, axis)
    return x, v


def interp_axis(x, v, xn, axis, method="linear"):
    """values ``v`` with coordinate ``x`` (strictly monotonic) along ``axis`` -> values at ``xn`` along that axis"""
    v = np.asarray(v)
    v = v.astype(np.float64) if v.dtype != np.float64 else v
    x, v = _ascending(x, v, axis)
    xn = np.asarray(xn, dtype=np.float64)
    n = len(x)
    v = np.moveaxis(v, axis, 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if method == "nearest":
            mid = x[1:] / 2.0 + x[:-1] / 2.0  # a target on a midpoint goes to the lower neighbour (side='left')
            out = v[np.clip(np.searchsorted(mid, xn, side="left"), 0, n - 1)].copy()
        elif method == "linear":
            hi = np.clip(np.searchsorted(x, xn, side="left"), 1, n - 1)  # a target on node k >= 1 uses the interval below it
            lo = hi - 1
            shape = (-1,) + (1,) * (v.ndim - 1)
            slope = (v[hi] - v[lo]) / (x[hi] - x[lo]).reshape(shape)  # a NaN node gives a NaN slope: NaN also at weight 0
            out = slope * (xn - x[lo]).reshape(shape) + v[lo]
        else:
            raise NotImplementedError(method)
    out[(xn < x[0]) | (xn > x[-1])] = np.nan  # no extrapolation
    return np.moveaxis(out, 0, axis)


def regrid(src, src_y, src_x, dst_y, dst_x, method="linear"):
    """src [..., ny, nx] -> [..., Ny, Nx] float64"""
    a = interp_axis(src_y, src, dst_y, -2, method)
    return interp_axis(src_x, a, dst_x, -1, method)
