"""The grouped oracle of compare(...).groupby(...): the rule of include/sd_downscale.h said in NumPy.  Group g of two [T, C] fields is
evaluated exactly as the binned oracles (tests/_skill_oracle.py, tests/_twosample_oracle.py) evaluate one bin whose steps are the rows t
with group[t] == g in ascending t: gather each group's rows in time order, then call ``sk.skill`` / ``ts.twosample`` on the gathered
series as bins.  An id that never occurs is an empty bin."""
import numpy as np

import _skill_oracle as sk
import _twosample_oracle as ts


def tables(group, G):
    """group [T] with every id in [0, G) -> (rows [T]: the row numbers grouped by id, ascending inside a group; offsets [G + 1])"""
    group = np.asarray(group)
    assert group.ndim == 1 and ((group >= 0) & (group < G)).all()
    rows = np.argsort(group, kind="stable").astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=G))]).astype(np.int64)
    return rows, offsets


def skill(a, b, group, G, stats=sk.STATS):
    """a, b [T, C], group [T] -> float64 [len(stats) * G, C], row s * G + g"""
    rows, offsets = tables(group, G)
    return sk.skill(np.asarray(a)[rows], np.asarray(b)[rows], offsets, stats)


def twosample(a, b, group, G, stats=ts.STATS, width=None, origin=0.0):
    """a, b [T, C], group [T] -> float64 [len(stats) * G, C], row s * G + g"""
    rows, offsets = tables(group, G)
    return ts.twosample(np.asarray(a)[rows], np.asarray(b)[rows], offsets, stats, width, origin)
