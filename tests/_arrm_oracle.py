"""NumPy restatement of PiecewiseLinearRegression(fit_option='arrm') of the reference (skdownscale/pointwise_models/arrm.py), per
cell: ``breakpoints`` follows ``arrm_breakpoints`` (arrm.py:19-105) line by line and also returns what the tests need besides
the picks (the r2 series without the masks, the argmin margin); ``fit_on_breaks`` is pwlf's documented model for
``PiecewiseLinFit(x, y).fit_with_breaks(b)`` (degree 1, no weights): least squares on the columns 1, x - b[0] and
max(x - b[j], 0) for j = 1 .. len(b) - 2, solved with LAPACK gelsd (minimum norm when rank deficient).  pwlf is not installed
where the goldens are made, so that step is pinned to the documented model and not to a pwlf run."""
import numpy as np
import scipy.linalg

MIN_WIDTH = 10


def plotting_positions(n, alpha=0.4, beta=0.4):
    return (np.arange(1, n + 1) - alpha) / (n + 1.0 - alpha - beta)


def window_r2(xs, ys):
    """engine rule for arrm.py:67: a window of equal xs or equal ys has no correlation (NaN)"""
    if xs[0] == xs[-1] or ys[0] == ys[-1]:
        return np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.corrcoef(xs, ys)[0, 1] ** 2


def breakpoints(X, y, window_width=0.05, max_breakpoints=7):
    """-> dict(index [B] sorted picks, breaks [B], r2 [n] as last written by the two loops without the masks (2: never written),
    margin: over all picks the smallest gap between the chosen r2 and the lowest r2 outside that pick's mask, in the range the
    pick was taken from (a NaN pick, the first NaN by rule, does not count), margin_computed: the same minimum without the picks
    whose chosen value is one of the sentinels, exactly 1.0 (masked) or 2.0 (never written): those tie exactly with every other
    sentinel and argmin's lowest-index rule decides them as exactly as it decides a NaN pick, start2: the start of the lower loop,
    min(upper picks) - 6, negative when an upper pick lies below 6 (no lower windows, the lower picks come from r2[:n + start2]),
    sentinel_picks: how many picks landed on a sentinel).

    When start2 == 0 the lower picks are taken from r2[:0] and the reference fails with ``ValueError: attempt to get argmin of an
    empty sequence``; so does this function, with the same text, through the same np.argmin."""
    npoints = len(X)
    X = np.sort(np.asarray(X, dtype=np.float64).reshape(npoints))
    y = np.sort(np.asarray(y, dtype=np.float64).reshape(npoints))
    quantiles = plotting_positions(npoints)
    r2 = np.zeros_like(X) + 2
    raw = r2.copy()
    picks = []
    margin = margin_computed = np.inf
    sentinel_picks = 0

    def pick(limit):
        nonlocal margin, margin_computed, sentinel_picks
        view = r2[:limit]
        mind = int(np.argmin(view))
        picks.append(mind)
        lo, hi = mind - MIN_WIDTH, mind + MIN_WIDTH + 1
        outside = np.ones(len(view), dtype=bool)
        outside[slice(lo, hi)] = False  # Python's slice rules, like the mask itself
        outside[mind] = False
        rest = view[outside]
        # a NaN pick is the first NaN whatever the other values are; any other pick competes with the lowest value left
        sentinel = view[mind] == 1.0 or view[mind] == 2.0
        sentinel_picks += int(sentinel)
        if len(rest) and not np.isnan(view[mind]):
            margin = min(margin, float(rest.min() - view[mind]))
            if not sentinel:
                margin_computed = min(margin_computed, float(rest.min() - view[mind]))
        r2[lo:hi] = 1

    start = int(np.argmin(np.absolute(quantiles - 0.4)))
    width = max(round(window_width * npoints), MIN_WIDTH)
    for right in range(start, npoints + 1):
        left = right - width
        mid = round((left + right) / 2)
        r2[mid] = raw[mid] = window_r2(X[left:right], y[left:right])
    for _ in range(max_breakpoints // 2):
        pick(npoints)
    start = min(picks, default=start)
    start -= (MIN_WIDTH // 2) + 1
    for left in range(start, -1, -1):
        right = left + width
        mid = round((left + right) / 2)
        r2[mid] = raw[mid] = window_r2(X[left:right], y[left:right])
    for _ in range(max_breakpoints // 2):
        pick(start)
    index = np.sort(np.asarray(picks, dtype=np.int64))
    return dict(index=index, breaks=X[index], r2=raw, margin=margin, margin_computed=margin_computed, start2=start,
                sentinel_picks=sentinel_picks)


def design(x, b):
    """pwlf's regression matrix of degree 1 on the sorted breaks b"""
    x = np.asarray(x, dtype=np.float64)
    cols = [np.ones_like(x), x - b[0]]
    for j in range(1, len(b) - 1):
        cols.append(np.where(x > b[j], x - b[j], 0.0))
    return np.stack(cols, axis=1)


def fit_on_breaks(x, y, b):
    """-> beta (minimum norm), ssr, cond(A)"""
    A = design(x, b)
    beta, _, _, sv = scipy.linalg.lstsq(A, np.asarray(y, dtype=np.float64), lapack_driver="gelsd")
    e = A @ beta - y
    sv = sv[sv > sv[0] * max(A.shape) * np.finfo(np.float64).eps]
    return beta, float(e @ e), float(sv[0] / sv[-1])


def predict(xq, b, beta):
    return design(xq, b) @ beta


def golden_case(name):
    """one case of tests/golden/g23_arrm*.npz (make_golden_arrm.py) with the expected predictions formed from the stored beta"""
    import os

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "g23_arrm.npz"), allow_pickle=False)
    fields = np.load(os.path.join(gold, f"g23_arrm_{name}_in.npz"), allow_pickle=False)
    c = {k: g[f"{name}_{k}"] for k in ("breaks", "index", "margin", "beta", "ssr", "cond")}
    c["mb"] = int(g[f"{name}_mb"])
    c["X"], c["y"] = fields["X"].astype(np.float64), fields["y"].astype(np.float64)
    c["Xq"] = g[f"{name}_Xq"].astype(np.float64) if f"{name}_Xq" in g.files else c["X"]
    c["r2"] = np.load(os.path.join(gold, f"g23_arrm_{name}_r2.npz"), allow_pickle=False)["r2"]
    c["pred"] = np.stack([predict(c["Xq"][:, k], c["breaks"][:, k], c["beta"][:, k]) for k in range(c["X"].shape[1])], axis=1)
    return c


CASES = ["gauss200", "gauss365", "gauss500", "gauss1200", "halfzero600", "offset288", "mb4", "query101"]

EMPTY_ARGMIN = "attempt to get argmin of an empty sequence"  # the reference's ValueError on a cell with start2 == 0
CASES_BREAKS = ["short50_mb8", "short50_mb16", "short51_mb12", "short59_mb17", "short64_mb16", "w210_mb8", "w230_mb12", "w250_mb16",
                "w270_mb9", "w220_mb8", "w260_mb8", "mb2_300", "mb3_300", "mb17_1000", "quant300_mb8"]


def breaks_case(name):
    """one case of tests/golden/g24_arrm_breaks*.npz (make_golden_arrm.py, main_breaks): as ``golden_case`` with ``raises`` [C]
    (the real reference raised EMPTY_ARGMIN on the cell; its other arrays hold NaN / -1), ``start2`` [C], ``margin_computed`` [C] and
    ``sentinel`` [C]; the queries are the training X"""
    import os

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "g24_arrm_breaks.npz"), allow_pickle=False)
    fields = np.load(os.path.join(gold, "g24_arrm_breaks_in.npz"), allow_pickle=False)
    keys = ("breaks", "index", "margin", "margin_computed", "beta", "ssr", "cond", "raises", "start2", "sentinel")
    c = {k: g[f"{name}_{k}"] for k in keys}
    c["mb"] = int(g[f"{name}_mb"])
    c["X"], c["y"] = fields[f"{name}_X"].astype(np.float64), fields[f"{name}_y"].astype(np.float64)
    c["Xq"] = c["X"]
    c["r2"] = np.load(os.path.join(gold, "g24_arrm_breaks_r2.npz"), allow_pickle=False)[f"{name}_r2"]
    c["pred"] = np.full(c["X"].shape, np.nan)
    for k in np.flatnonzero(~c["raises"]):
        c["pred"][:, k] = predict(c["X"][:, k], c["breaks"][:, k], c["beta"][:, k])
    return c


def predict_longdouble(x, y, b, xq):
    """predictions of the least-squares fit of ``design(x, b)`` in np.longdouble (64-bit mantissa on x86): Gram-Schmidt with
    reorthogonalisation on the independent columns (a hinge that repeats an earlier break, or lies at or outside the ends of the
    data, is dropped: the fitted values do not depend on how a rank-deficient solution is chosen).  The yardstick of how far
    ``fit_on_breaks`` / ``predict`` (float64 gelsd) can be trusted at a given condition number."""
    x, xq = np.asarray(x, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    keep, seen = [0, 1] if x.max() > x.min() else [0], set()
    for j in range(1, len(b) - 1):
        if x.min() < b[j] < x.max() and b[j] not in seen:
            keep.append(j + 1)
            seen.add(b[j])
    A = design(x, b)[:, keep].astype(np.longdouble)
    Aq = design(xq, b)[:, keep].astype(np.longdouble)
    Q = np.zeros_like(A)
    R = np.zeros((A.shape[1], A.shape[1]), dtype=np.longdouble)
    for k in range(A.shape[1]):
        v = A[:, k].copy()
        for _ in range(2):
            for i in range(k):
                r = Q[:, i] @ v
                R[i, k] += r
                v -= r * Q[:, i]
        R[k, k] = np.sqrt(v @ v)
        Q[:, k] = v / R[k, k]
    z = Q.T @ np.asarray(y, dtype=np.longdouble)
    coef = np.zeros(A.shape[1], dtype=np.longdouble)
    for k in range(A.shape[1] - 1, -1, -1):
        coef[k] = (z[k] - R[k, k + 1:] @ coef[k + 1:]) / R[k, k]
    return Aq @ coef
