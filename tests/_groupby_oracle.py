"""NumPy restatement of the groupby rule (csrc/sd_groupby.hip): an explicit loop over the rows of a [T, C] field, every row added
onto the accumulator of its group, NaN samples skipped.  It is the definition, so the kernel is compared with it bit for bit.  ``mean``
of a group without a non-NaN sample is NaN, ``sum`` of it 0.0 (pandas' ``DataFrame.groupby(key).mean()`` / ``.sum()``);
tests/test_groupby_host.py pins it to pandas' results in the golden file, within ``bound``."""
import numpy as np

import _resample_oracle

APPLY = {"sub": np.subtract, "add": np.add, "mul": np.multiply, "div": np.divide}


def accumulate(field, group, G, acc=None):
    """the rows of field [T, C] (float32 is widened first) added in row order onto (sum [G, C] float64, count [G, C] int32);
    ``acc``: the pair an earlier call returned (continued, not changed in place), None: zeros"""
    x = np.asarray(field).astype(np.float64)
    group = np.asarray(group)
    assert x.ndim == 2 and group.shape == (x.shape[0],) and ((group >= 0) & (group < G)).all()
    s, n = (np.zeros((G, x.shape[1])), np.zeros((G, x.shape[1]), dtype=np.int32)) if acc is None else (acc[0].copy(), acc[1].copy())
    with np.errstate(invalid="ignore"):
        for t in range(x.shape[0]):  # row order
            take = x[t] == x[t]
            s[group[t]] = s[group[t]] + np.where(take, x[t], 0.0)
            n[group[t]] += take
    return s, n


def finish(acc, op="mean"):
    s, n = acc
    with np.errstate(invalid="ignore", divide="ignore"):
        return s.copy() if op == "sum" else np.where(n > 0, s / np.maximum(n, 1), np.nan)


def reduce(field, group, G, op="mean"):
    """field [T, C], group int [T] in [0, G) -> [G, C] float64"""
    return finish(accumulate(field, group, G), op)


def apply(field, group, table, op):
    """field [T, C] (float32 is widened first) (op) table[group]: one IEEE operation per element -> [T, C] float64"""
    with np.errstate(all="ignore"):
        return APPLY[op](np.asarray(field).astype(np.float64), np.asarray(table, dtype=np.float64)[np.asarray(group)])


def tables(group, G):
    """(rows [T], offsets [G + 1]): the rows grouped by id, in row order inside a group (csrc/sd_groupby_plan.h: groupby_tables)"""
    group = np.asarray(group)
    rows = np.argsort(group, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=G))]).astype(np.int64)
    return rows, offsets


def bound(field, group, G, op="mean"):
    """the bound of tests/_resample_oracle.py on |got - want| per group and cell, for either plain or compensated float64 summation:
    sum: (n + 2) * 2^-53 * sum|x_i| over the n non-NaN samples of the group; mean: that divided by n, plus one ulp for the division"""
    rows, offsets = tables(group, G)
    return _resample_oracle.bound(np.asarray(field)[rows], offsets, op)


def check(got, want, field, group, G, op, what=""):
    """NaN pattern and the exact results of groups without a sample identical, everything else within ``bound``"""
    rows, offsets = tables(group, G)
    return _resample_oracle.check(got, want, np.asarray(field)[rows], offsets, op, what)
