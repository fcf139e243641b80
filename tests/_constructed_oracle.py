"""The rule of the constructed-analog calls (include/sd_downscale.h: sd_ca_select_dev, sd_ca_weights_dev, sd_ca_apply_dev) restated with
plain NumPy loops.  Every sum is a Python loop over its terms; NumPy is used for elementwise steps only (one IEEE operation per element
and step), so no pairwise or fused sum enters, and the kernels must give the same bits.  This file is normative for the order of every
operation.

How far the regression weights of the rule may lie from an independent formulation (``np.linalg.solve`` on the same ``G`` and ``b``: LU
with partial pivoting in place of the Cholesky factor) was measured on the inputs of tests/test_constructed_host.py (``coarse_case`` with
seeds 0, 1, 2: 280 K fields, Tl = 120, Tq = 9, Cc = 12 with 10 used columns) as the largest ``max|w - w_solve| / max|w_solve|`` over all
targets:

    ridge = 1e-6:  k = 1: 2.2e-16   k = 5: 6.2e-12   k = 30: 1.5e-9 (cond 3.0e7)    k = 32: 1.6e-9 (cond 3.2e7)
    ridge = 1e-9:  k = 1: 2.3e-16   k = 5: 5.2e-12   k = 30: 1.3e-6 (cond 3.0e10)   k = 32: 1.7e-6 (cond 3.2e10)

With k > 10 the Gram matrix has rank 10 and only the ridge makes it definite, so the difference scales with cond * eps.  ``SOLVE_RTOL`` is,
per ridge, 10 times the largest measurement.  No Cholesky failure occurred with k > Cc or with exact duplicate library rows at these
ridges; at ridge = 0 duplicates give a pivot that is not > 0 (SINGULAR).
"""
import numpy as np

OK, QUERY_NONFINITE, FEW_CANDIDATES, SINGULAR = 0, 1, 2, 3
REGRESSION, MEAN = 0, 1
SOLVE_RTOL = {1e-6: 1.6e-8, 1e-9: 1.7e-5}


def used_columns(L, wc):
    """step 1: ascending indices of the columns with a library that is finite in every row and wc > 0"""
    return [c for c in range(L.shape[1]) if wc[c] > 0 and np.isfinite(L[:, c]).all()]


def candidates(key_l, key_q, period, window, excl_l, excl_q):
    """step 2 -> bool [Tq, Tl]"""
    a = np.asarray(key_q, dtype=np.int64)[:, None]
    b = np.asarray(key_l, dtype=np.int64)[None, :]
    diff = np.abs(a - b)
    near = np.ones(diff.shape, bool) if window < 0 else np.minimum(diff, period - diff) <= window
    xq = np.asarray(excl_q, dtype=np.int64)[:, None]
    return near & ((xq < 0) | (np.asarray(excl_l, dtype=np.int64)[None, :] != xq))


def distances(L, Q, wc, cols):
    """step 3 -> float64 [Tq, Tl]: one column after the other, each step elementwise"""
    d = np.zeros((Q.shape[0], L.shape[0]))
    with np.errstate(all="ignore"):
        for c in cols:
            e = Q[:, c][:, None] - L[:, c][None, :]
            d = d + wc[c] * (e * e)
    return d


def select(L, Q, wc, k, key_l, key_q, period, window, excl_l, excl_q):
    """steps 1 to 4 and the status of step 7 -> idx int32 [Tq, k], dist [Tq, k], status int32 [Tq]"""
    L, Q, wc = np.asarray(L, np.float64), np.asarray(Q, np.float64), np.asarray(wc, np.float64)
    cols = used_columns(L, wc)
    if not cols:
        raise ValueError("no column is used")
    Tq, Tl = Q.shape[0], L.shape[0]
    cand = candidates(key_l, key_q, period, window, excl_l, excl_q)
    d = distances(L, Q, wc, cols)
    idx = np.full((Tq, k), -1, np.int32)
    dist = np.full((Tq, k), np.nan)
    status = np.zeros(Tq, np.int32)
    for q in range(Tq):
        if not np.isfinite(Q[q, cols]).all():
            status[q] = QUERY_NONFINITE
            continue
        pairs = sorted((d[q, t], t) for t in range(Tl) if cand[q, t])  # (d, t) in lexicographic order
        if len(pairs) < k:
            status[q] = FEW_CANDIDATES
            continue
        for i in range(k):
            dist[q, i], idx[q, i] = pairs[i]
    return idx, dist, status


def gram(L, Qrow, wc, cols, rows):
    """G [k, k] (lower triangle mirrored) and b [k] of step 6, before the ridge"""
    k = len(rows)
    G, b = np.zeros((k, k)), np.zeros(k)
    for i in range(k):
        for j in range(i + 1):
            s = 0.0
            for c in cols:
                s = s + wc[c] * (L[rows[i], c] * L[rows[j], c])
            G[i, j] = G[j, i] = s
        s = 0.0
        for c in cols:
            s = s + wc[c] * (L[rows[i], c] * Qrow[c])
        b[i] = s
    return G, b


def add_ridge(G, ridge):
    k = len(G)
    trace = G[0, 0]
    for i in range(1, k):
        trace = trace + G[i, i]
    lam = ridge * (trace / float(k))
    G = G.copy()
    for i in range(k):
        G[i, i] = G[i, i] + lam
    return G


def cholesky_solve(G, b):
    """the prototype of step 6 -> w [k], or None where a pivot is not > 0"""
    k = len(b)
    C = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i + 1):
                s = G[i, j]
                for p in range(j):
                    s = s - C[i, p] * C[j, p]
                if j < i:
                    C[i, j] = s / C[j, j]
                else:
                    if not s > 0:
                        return None
                    C[i, i] = np.sqrt(s)
        y = np.zeros(k)
        for i in range(k):
            s = b[i]
            for p in range(i):
                s = s - C[i, p] * y[p]
            y[i] = s / C[i, i]
        w = np.zeros(k)
        for i in range(k - 1, -1, -1):
            s = y[i]
            for p in range(i + 1, k):
                s = s - C[p, i] * w[p]
            w[i] = s / C[i, i]
    return w


def weights(L, Q, wc, idx, dist, status, kind, ridge):
    """steps 5 to 7 from the tables of ``select`` -> (weights [Tq, k], idx, dist, status): copies, a singular target cleared"""
    L, Q, wc = np.asarray(L, np.float64), np.asarray(Q, np.float64), np.asarray(wc, np.float64)
    cols = used_columns(L, wc)
    idx, dist, status = idx.copy(), dist.copy(), status.copy()
    Tq, k = idx.shape
    w = np.full((Tq, k), np.nan)
    for q in range(Tq):
        if status[q] != OK:
            continue
        if kind == MEAN:
            w[q] = 1.0 / float(k)
            continue
        G, b = gram(L, Q[q], wc, cols, idx[q])
        sol = cholesky_solve(add_ridge(G, ridge), b)
        if sol is None:
            status[q], idx[q], dist[q] = SINGULAR, -1, np.nan
        else:
            w[q] = sol
    return w, idx, dist, status


def apply(F, idx, w, q0=0, q1=None):
    """step 8 for the rows [q0, q1) -> float64 [q1 - q0, Cf]"""
    q1 = idx.shape[0] if q1 is None else q1
    F = np.asarray(F)
    out = np.empty((q1 - q0, F.shape[1]))
    with np.errstate(all="ignore"):
        for q in range(q0, q1):
            if idx[q, 0] < 0:
                out[q - q0] = np.nan
                continue
            acc = np.zeros(F.shape[1])
            for i in range(idx.shape[1]):
                acc = acc + w[q, i] * F[idx[q, i]].astype(np.float64)
            out[q - q0] = acc
    return out


def constructed(L, Q, wc, F, k, kind, ridge, key_l, key_q, period, window, excl_l, excl_q):
    """the whole rule -> idx, dist, weights, status, out"""
    idx, dist, status = select(L, Q, wc, k, key_l, key_q, period, window, excl_l, excl_q)
    w, idx, dist, status = weights(L, Q, wc, idx, dist, status, kind, ridge)
    return idx, dist, w, status, apply(F, idx, w)
