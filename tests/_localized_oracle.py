"""The rule of the localized-analog calls (include/sd_downscale.h: sd_ca_local_dev, sd_ca_local_apply_dev) restated with plain loops.
Every sum is a Python loop over its terms in the order of the rule, every term one IEEE operation after the other on Python floats
(float64), so no pairwise or fused sum enters, and the kernels must give the same bits.  This file is normative for the order of every
operation.  The regional stage (``select``) and step 1 (``used_columns``) are those of tests/_constructed_oracle.py."""
import numpy as np

from _constructed_oracle import select, used_columns  # noqa: F401  (``select`` is part of this oracle's surface)

ADJUST_NONE, ADJUST_SHIFT, ADJUST_SCALE = 0, 1, 2


def local_distance(L, Qrow, wc, used, t, i, j, ny, nx, ry, rx):
    """L2: the distance of library day ``t`` around coarse cell (i, j); ``used``: the set of used columns"""
    dl = 0.0
    with np.errstate(all="ignore"):
        for ii in range(max(0, i - ry), min(ny - 1, i + ry) + 1):
            for jj in range(max(0, j - rx), min(nx - 1, j + rx) + 1):
                c = ii * nx + jj
                if c not in used:
                    continue  # skipped, not weighted 0: its e may be NaN
                e = np.float64(Qrow[c]) - np.float64(L[t, c])
                dl = dl + np.float64(wc[c]) * (e * e)
    return dl


def local(L, Q, wc, idx, ny, nx, ry, rx):
    """L1 to L3 -> slot int32 [Tq, Cc], local_idx int32 [Tq, Cc], local_dist float64 [Tq, Cc]; slot is -1 where local_idx is"""
    L, Q, wc = np.asarray(L, np.float64), np.asarray(Q, np.float64), np.asarray(wc, np.float64)
    Tq, k = idx.shape
    Cc = ny * nx
    assert L.shape[1] == Cc and Q.shape[1] == Cc and wc.shape == (Cc,)
    used = set(used_columns(L, wc))
    if not used:
        raise ValueError("no column is used")
    slot = np.full((Tq, Cc), -1, np.int32)
    lidx = np.full((Tq, Cc), -1, np.int32)
    ldist = np.full((Tq, Cc), np.nan)
    for q in range(Tq):
        if idx[q, 0] < 0 or not ((idx[q] >= 0) & (idx[q] < L.shape[0])).all():
            continue
        for i in range(ny):
            for j in range(nx):
                best, at = None, 0
                for a in range(k):
                    dl = local_distance(L, Q[q], wc, used, int(idx[q, a]), i, j, ny, nx, ry, rx)
                    if a == 0 or dl < best:
                        best, at = dl, a
                c = i * nx + j
                slot[q, c], lidx[q, c], ldist[q, c] = at, idx[q, at], best
    return slot, lidx, ldist


def local_apply(F, cell_of, lidx, L=None, Q=None, adjust=ADJUST_NONE, max_scale=0.0, q0=0, q1=None):
    """L4 for the rows [q0, q1) -> float64 [q1 - q0, Cf]"""
    q1 = lidx.shape[0] if q1 is None else q1
    F = np.asarray(F)
    Tl, Cf = F.shape
    Cc = lidx.shape[1]
    out = np.full((q1 - q0, Cf), np.nan)
    with np.errstate(all="ignore"):
        for q in range(q0, q1):
            for f in range(Cf):
                c = int(cell_of[f])
                if not 0 <= c < Cc:
                    continue
                t = int(lidx[q, c])
                if not 0 <= t < Tl:
                    continue
                v = np.float64(F[t, f])
                if adjust == ADJUST_SHIFT:
                    v = v + (np.float64(Q[q, c]) - np.float64(L[t, c]))
                elif adjust == ADJUST_SCALE:
                    r = np.float64(Q[q, c]) / np.float64(L[t, c]) if L[t, c] > 0 else np.float64(1.0)
                    if max_scale > 0 and r > max_scale:
                        r = np.float64(max_scale)
                    v = v * r
                out[q - q0, f] = v
    return out
