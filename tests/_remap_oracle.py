"""NumPy restatement of the first-order conservative remap (GridArray.remap_like, csrc/sd_remap_plan.h and sd_remap.hip), in exactly
the order the engine uses, so that the engine can be compared bit for bit:

* ``axis_table``: per target cell the contiguous run of source cells (in stored order) whose overlap
  ``min(sb_hi, db_hi) - max(sb_lo, db_lo)`` on the ascending-ordered bounds is > 0, the overlaps themselves and ``full``, their
  running sum from +0.0.  Found by brute force over all pairs (the header searches; the tables must be equal).
* ``remap``: per target row the rows of its run are added in stored order into ``cn`` (values, NaN as 0) and ``cd`` (1 where the value
  is not NaN), each product rounded on its own; per target column the columns of its run likewise; ``num / den`` where
  ``den > 0`` and ``den >= min_valid * (full_y * full_x) * (1 - 2**-30)``, NaN elsewhere.
"""
import numpy as np

SLACK = 1.0 - 2.0 ** -30


def axis_table(src_bounds, dst_bounds):
    """-> first int [m], count int [m], weights list of m float64 arrays, full float64 [m]"""
    sb, db = np.asarray(src_bounds, dtype=np.float64), np.asarray(dst_bounds, dtype=np.float64)
    slo, shi = np.minimum(sb[:-1], sb[1:]), np.maximum(sb[:-1], sb[1:])
    dlo, dhi = np.minimum(db[:-1], db[1:]), np.maximum(db[:-1], db[1:])
    m = len(db) - 1
    first, count, weights, full = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), [], np.zeros(m)
    for j in range(m):
        w = np.minimum(shi, dhi[j]) - np.maximum(slo, dlo[j])
        ks = np.flatnonzero(w > 0)
        if len(ks):
            assert np.array_equal(ks, np.arange(ks[0], ks[0] + len(ks))), "the run of a target cell is contiguous"
            first[j], count[j] = ks[0], len(ks)
        weights.append(w[ks].copy())
        acc = 0.0
        for x in w[ks]:
            acc = acc + x
        full[j] = acc
    return first, count, weights, full


def remap(v, src_yb, src_xb, dst_yb, dst_xb, min_valid=0.5):
    """v [T, ny, nx] float32 / float64 -> [T, Ny, Nx] float64"""
    v = np.asarray(v)
    assert v.ndim == 3
    v = v.astype(np.float64)  # (exact for float32)
    T = v.shape[0]
    fy, ky, wy, fully = axis_table(src_yb, dst_yb)
    fx, kx, wx, fullx = axis_table(src_xb, dst_xb)
    assert v.shape[1:] == (len(src_yb) - 1, len(src_xb) - 1)
    Ny, Nx = len(fy), len(fx)
    out = np.full((T, Ny, Nx), np.nan)
    isnan = np.isnan(v)
    val, one = np.where(isnan, 0.0, v), np.where(isnan, 0.0, 1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(Ny):
            cn, cd = np.zeros((T, v.shape[2])), np.zeros((T, v.shape[2]))
            for r in range(ky[j]):
                cn = cn + wy[j][r] * val[:, fy[j] + r, :]
                cd = cd + wy[j][r] * one[:, fy[j] + r, :]
            for i in range(Nx):
                num, den = np.zeros(T), np.zeros(T)
                for c in range(kx[i]):
                    num = num + wx[i][c] * cn[:, fx[i] + c]
                    den = den + wx[i][c] * cd[:, fx[i] + c]
                thr = min_valid * (fully[j] * fullx[i]) * SLACK
                ok = (den > 0) & (den >= thr)
                out[:, j, i] = np.where(ok, num / den, np.nan)
    return out


def cell_bounds(centres):
    """midpoints between neighbouring centres, the two ends extrapolated by half the end spacing"""
    c = np.asarray(centres, dtype=np.float64)
    mid = 0.5 * (c[:-1] + c[1:])
    return np.concatenate([[c[0] - 0.5 * (c[1] - c[0])], mid, [c[-1] + 0.5 * (c[-1] - c[-2])]])


def area_bounds(lat_bounds):
    return np.sin(np.deg2rad(np.clip(np.asarray(lat_bounds, dtype=np.float64), -90.0, 90.0)))
