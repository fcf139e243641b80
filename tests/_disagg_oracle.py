"""NumPy restatement of the temporal disaggregation rule (csrc/sd_disagg.hip): a loop over the bins of the output, the borrowed samples
of a bin added in time order, NaN samples skipped by a select, then one add (shift) or one multiply (scale) per sample.  Every
operation is a single IEEE add, subtract, multiply or divide in float64, so the kernel must give the same bits;
tests/test_disagg_host.py pins this file to a per-month pandas formulation and to the closed loop through pandas' resampler."""
import numpy as np

OPS = ("shift", "scale_mean", "scale_sum")


def resolve_target(target, op, climo=None, group=None):
    """the monthly value a bin is brought to: the target, or climatology + anomaly (shift) / climatology * anomaly (scale)"""
    target = np.asarray(target, dtype=np.float64)
    if climo is None:
        return target
    base = np.asarray(climo, dtype=np.float64)[np.asarray(group)]
    with np.errstate(invalid="ignore", over="ignore"):
        return base + target if op == "shift" else base * target


def statistic(obs, src_row, offsets):
    """(acc, cnt) [M, C] of the borrowed rows: the plain running sum of the non-NaN samples in time order, and their number"""
    x = np.asarray(obs).astype(np.float64)
    M, C = len(offsets) - 1, x.shape[1]
    acc, cnt = np.zeros((M, C)), np.zeros((M, C), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(M):
            for t in range(offsets[m], offsets[m + 1]):  # time order
                row = x[src_row[t]]
                take = row == row
                acc[m] = acc[m] + np.where(take, row, 0.0)
                cnt[m] += take
    return acc, cnt


def disaggregate(target, obs, src_row, offsets, op="shift", climo=None, group=None):
    """target [M, C], obs [To, C] (float32 is widened first), src_row int [Tout], offsets int [M + 1] -> [Tout, C] float64"""
    assert op in OPS
    x = np.asarray(obs).astype(np.float64)
    src_row, offsets = np.asarray(src_row, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    Tout, M, C = len(src_row), len(offsets) - 1, x.shape[1]
    assert offsets[0] == 0 and offsets[-1] == Tout and (np.diff(offsets) >= 0).all()
    assert ((src_row >= 0) & (src_row < len(x))).all()
    tgt = resolve_target(target, op, climo, group)
    assert tgt.shape == (M, C)
    acc, cnt = statistic(x, src_row, offsets)
    out = np.empty((Tout, C))
    with np.errstate(all="ignore"):
        for m in range(M):
            rows = x[src_row[offsets[m]:offsets[m + 1]]]
            n = cnt[m].astype(np.float64)
            if op == "shift":
                res = rows + (tgt[m] - acc[m] / n)
            else:
                s = acc[m] / n if op == "scale_mean" else acc[m]
                fill = tgt[m] if op == "scale_mean" else tgt[m] / n
                # a dry borrowed month: every non-NaN day gets the same share
                res = np.where(s == 0.0, np.where(rows == rows, fill, rows), rows * (tgt[m] / s))
            out[offsets[m]:offsets[m + 1]] = res
    return out


def bound(out, target, obs, src_row, offsets, op="shift", climo=None, group=None):
    """the derived bound [M, C] on |statistic of the output - target| when the statistic (mean for 'shift' and 'scale_mean', sum for
    'scale_sum') is taken again by plain or compensated float64 summation (pandas' resampler).  With u = 2^-53, n the
    non-NaN samples of the bin, Sx = sum|x_t| of the borrowed samples, S their computed sum and So = sum|out_t|:
      the statistic of the borrowed month is within n u Sx of exact, the addend or factor adds one rounding on the target's scale, every
      output sample one rounding of its own (u So in the sum), and the check's own summation (n + 2) u So plus one ulp of the result;
      shift: u ((n + 2) Sx / n + |tgt| + (n + 3) So / n) + ulp(tgt)
      scale: u |tgt| (2 + (n + 2) Sx / |S|) + u (n + 3) So [/ n for the mean] + ulp(tgt), the Sx / |S| term absent for a dry month."""
    x = np.asarray(obs).astype(np.float64)
    out = np.asarray(out, dtype=np.float64)
    tgt = np.abs(resolve_target(target, op, climo, group))
    acc, cnt = statistic(x, src_row, offsets)
    M = len(offsets) - 1
    u = 2.0 ** -53
    b = np.zeros_like(tgt)
    with np.errstate(all="ignore"):
        for m in range(M):
            rows, res = np.abs(x[src_row[offsets[m]:offsets[m + 1]]]), np.abs(out[offsets[m]:offsets[m + 1]])
            n = np.maximum(cnt[m], 1).astype(np.float64)
            Sx, So = np.where(rows == rows, rows, 0.0).sum(axis=0), np.where(res == res, res, 0.0).sum(axis=0)
            if op == "shift":
                b[m] = u * ((n + 2) * Sx / n + tgt[m] + (n + 3) * So / n)
            else:
                spread = np.where(acc[m] == 0.0, 0.0, Sx / np.abs(acc[m]))
                b[m] = u * tgt[m] * (2 + (n + 2) * spread) + u * (n + 3) * So / (n if op == "scale_mean" else 1.0)
            b[m] = b[m] + np.spacing(tgt[m])
    return b
