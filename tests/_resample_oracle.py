"""NumPy restatement of the resampling rule (csrc/sd_resample.hip): a loop over the bins of a [T, C] field, NaN samples skipped,
the samples of a bin added in time order.  ``mean`` of a bin without a non-NaN sample is NaN, ``sum`` of it 0.0 (pandas'
``DataFrame.resample(rule).mean()`` / ``.sum()``); tests/test_resample_host.py pins it to pandas' results in the golden file."""
import numpy as np


def resample(field, offsets, op="mean"):
    """field [T, C] (float32 is widened first), offsets int [M + 1] -> [M, C] float64"""
    x = np.asarray(field).astype(np.float64)
    T, C = x.shape
    offsets = np.asarray(offsets, dtype=np.int64)
    assert offsets[0] == 0 and offsets[-1] == T and (np.diff(offsets) >= 0).all()
    M = len(offsets) - 1
    out = np.empty((M, C))
    for m in range(M):
        acc, cnt = np.zeros(C), np.zeros(C, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for t in range(offsets[m], offsets[m + 1]):  # time order
                take = x[t] == x[t]
                acc = acc + np.where(take, x[t], 0.0)
                cnt += take
            out[m] = acc if op == "sum" else np.where(cnt > 0, acc / np.maximum(cnt, 1), np.nan)
    return out


def bound(field, offsets, op="mean"):
    """the derived bound on |got - want| per bin and cell for either plain or compensated float64 summation:
    sum: (n + 2) * 2^-53 * sum|x_i| over the n non-NaN samples; mean: that divided by n, plus one ulp of the result for the division"""
    x = np.asarray(field).astype(np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    M = len(offsets) - 1
    out = np.zeros((M, x.shape[1]))
    for m in range(M):
        seg = x[offsets[m]:offsets[m + 1]]
        n = (seg == seg).sum(axis=0)
        with np.errstate(invalid="ignore"):
            mag = np.where(seg == seg, np.abs(seg), 0.0).sum(axis=0)
        b = (n + 2) * 2.0 ** -53 * mag
        if op == "mean":
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(n > 0, mag / np.maximum(n, 1), 0.0)
            b = b / np.maximum(n, 1) + np.spacing(mean)
        out[m] = b
    return out


def check(got, want, field, offsets, op, what=""):
    """NaN pattern and exact zeros of empty bins identical, everything else within ``bound``; returns the largest |err| / bound"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    b = bound(field, offsets, op)
    nosample = b == 0.0  # no non-NaN sample (or all of them zero): the result is exact
    assert np.array_equal(got[nosample], want[nosample], equal_nan=True), f"{what}: bins without a sample differ"
    with np.errstate(invalid="ignore"):
        err = np.nan_to_num(np.abs(got - want), nan=0.0)
    ratio = float(np.max(np.where(nosample, 0.0, err / np.where(nosample, 1.0, b)), initial=0.0))
    print(f"{what}: max |got - want| / bound = {ratio:.3f}")
    assert (err <= b).all(), (what, ratio)
    return ratio
