"""NumPy restatement of the rolling rule (csrc/sd_rolling.hip): every window of a [T, C] field evaluated directly, in time order, by an
explicit loop over the rows and the positions of their windows, vectorised over the cells.  It is the definition, so the kernel is
compared with it bit for bit:

    window of row t    rows t - back .. t - back + w - 1, clipped to [0, T) or, with wrap, taken modulo T
    n                  the non-NaN samples of the window
    sum                s = ((+0.0 + x_a) + x_b) + ... over them, in that order
    mean               s / n, NaN where n == 0
    var(ddof)          q / (n - ddof) with q = ((+0.0 + (x_a - mean)^2) + (x_b - mean)^2) + ..., NaN where n - ddof <= 0
    std(ddof)          sqrt(var)
    all four           NaN where n < min_periods

One IEEE operation per step.  Skipped samples add +0.0, which changes no bit: s and q start at +0.0 and no sum of two doubles is -0.0
unless both are.

Against pandas (``DataFrame.rolling(w, center=..., min_periods=...)``) the NaN pattern is identical and the values agree within a
measured bound: pandas updates its sums online -- add the entering sample, remove the leaving one, Kahan-compensated --, so its error
depends on the history of the series and not on the window, and cannot be derived from the window alone.  Measured against pandas 2.3.3
on tests/golden/g27_rolling.npz (T = 400, 6 cells; ``python tests/_rolling_oracle.py`` prints them), as multiples of the largest |x| of
the field (of its square for var and for std, which is compared through its square: relative to a variance itself the difference
reaches 4e-5 on zero-inflated precipitation, where a window's variance is tiny beside the field's scale):

    mean    measured 1.6e-15 * max|x|      tolerance 8 x = 1.28e-14 * max|x|
    sum     measured 1.9e-14 * max|x|      tolerance 8 x = 1.52e-13 * max|x|    (windows of up to 31 samples: 6e-16 of a sum)
    var     measured 3.7e-16 * max|x|^2    tolerance 8 x = 2.96e-15 * max|x|^2
    std     measured 4.0e-16 * max|x|^2    tolerance 8 x = 3.2e-15 * max|x|^2   (on std^2)

The largest differences follow the run of 40 NaN in one cell, where pandas' running sums have just been emptied.  The factor 8
covers a pandas other than 2.3.3.
"""
import numpy as np

OPS = ("mean", "sum", "var", "std")
MEASURED = {"mean": 1.6e-15, "sum": 1.9e-14, "var": 3.7e-16, "std": 4.0e-16}  # of max|x| (mean, sum) or max|x|^2 (var, std^2)
TOLERANCE = {op: 8 * m for op, m in MEASURED.items()}


def back_of(window, center):
    return window // 2 if center else window - 1


def moments_by_rows(field, window, back, wrap=False):
    """field [T, C] (float32 is widened first) -> (s, n, q) [T, C]: per window the running sum of its non-NaN samples, their number and
    the running sum of their squared deviations from s / n, each in time order.  The definition: a loop over the rows and, per row, over
    the positions of its window, vectorised over the cells"""
    x = np.asarray(field).astype(np.float64)
    assert x.ndim == 2 and window >= 1 and 0 <= back < window and not (wrap and window > x.shape[0])
    T, C = x.shape
    S, N, Q = np.empty((T, C)), np.empty((T, C), dtype=np.int64), np.empty((T, C))
    with np.errstate(all="ignore"):
        for t in range(T):
            pos = range(t - back, t - back + window)
            rows = [p % T for p in pos] if wrap else [p for p in pos if 0 <= p < T]
            s, n, q = np.zeros(C), np.zeros(C, dtype=np.int64), np.zeros(C)
            for r in rows:  # time order
                take = x[r] == x[r]
                s = s + np.where(take, x[r], 0.0)
                n += take
            mean = np.where(n > 0, s / np.maximum(n, 1), np.nan)
            for r in rows:
                d = x[r] - mean
                q = q + np.where(x[r] == x[r], d * d, 0.0)
            S[t], N[t], Q[t] = s, n, q
    return S, N, Q


def moments(field, window, back, wrap=False):
    """``moments_by_rows`` with the loops exchanged -- over the positions of the window, every row at once --, for long windows: each
    (row, cell) still adds its samples in time order, one operation per step, and a position outside the array adds +0.0, so the bits
    are those of the definition (tests/test_rolling_host.py compares them)"""
    x = np.asarray(field).astype(np.float64)
    assert x.ndim == 2 and window >= 1 and 0 <= back < window and not (wrap and window > x.shape[0])
    T, C = x.shape
    s, n, q = np.zeros((T, C)), np.zeros((T, C), dtype=np.int64), np.zeros((T, C))
    with np.errstate(all="ignore"):
        for second in (False, True):
            for k in range(window):  # time order
                p = np.arange(T) - back + k
                xk = x[p % T]
                take = (xk == xk) & (np.ones(T, dtype=bool) if wrap else (p >= 0) & (p < T))[:, None]
                if second:
                    d = xk - mean
                    q = q + np.where(take, d * d, 0.0)
                else:
                    s = s + np.where(take, xk, 0.0)
                    n += take
            mean = np.where(n > 0, s / np.maximum(n, 1), np.nan)
    return s, n, q


def finish(m, op="mean", min_periods=1, ddof=1):
    s, n, q = m
    with np.errstate(all="ignore"):
        if op == "sum":
            res = s
        elif op == "mean":
            res = np.where(n > 0, s / np.maximum(n, 1), np.nan)
        else:
            res = np.where(n - ddof > 0, q / np.maximum(n - ddof, 1), np.nan)
            if op == "std":
                res = np.sqrt(res)
        return np.where(n >= min_periods, res, np.nan)


def rolling(field, window, op="mean", center=False, min_periods=None, ddof=1, wrap=False, back=None):
    """field [T, C] -> [T, C] float64"""
    assert op in OPS and ddof >= 0
    back = back_of(window, center) if back is None else back
    min_periods = window if min_periods is None else min_periods
    assert 0 <= min_periods <= window
    return finish(moments(field, window, back, wrap), op, min_periods, ddof)


def scale(field, op):
    """what the pandas tolerances are multiples of: the largest |x| of the field, squared for var and std"""
    a = float(np.nanmax(np.abs(np.asarray(field, dtype=np.float64))))
    return a * a if op in ("var", "std") else a


def distance(got, want, field, op):
    """max |got - want| (through the squares for std) in units of ``scale``, over the entries that are not NaN in both"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = ~(np.isnan(got) & np.isnan(want))
    if op == "std":
        got, want = got * got, want * want
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)[both]
    return float(d.max() / scale(field, op)) if d.size else 0.0


def check(got, want, field, op, what=""):
    """NaN pattern identical, everything else within TOLERANCE[op] of the field's scale"""
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    d = distance(got, want, field, op)
    assert d <= TOLERANCE[op], f"{what}: differs by {d:.3e} of the scale, allowed {TOLERANCE[op]:.3e}"
    return d


def golden_cases(g):
    """the cases of tests/golden/g27_rolling.npz: (key, field name, window, op, center, min_periods, ddof, wrap)"""
    return [(str(k), str(f), int(w), str(op), bool(c), None if mp < 0 else int(mp), int(dd), bool(wr))
            for k, f, w, op, c, mp, dd, wr in zip(g["case.key"], g["case.field"], g["case.window"], g["case.op"], g["case.center"],
                                                  g["case.min_periods"], g["case.ddof"], g["case.wrap"])]


if __name__ == "__main__":  # the measured distances of the docstring
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_rolling.npz"))
    worst = dict.fromkeys(OPS, 0.0)
    for key, f, w, op, center, mp, ddof, wrap in golden_cases(g):
        d = distance(rolling(g[f], w, op, center, mp, ddof, wrap), g[key], g[f], op)
        worst[op] = max(worst[op], d)
        print(f"{key:60s} {d:.3e}")
    print({op: f"{v:.2e}" for op, v in worst.items()})
