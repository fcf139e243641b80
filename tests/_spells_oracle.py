"""NumPy restatement of the threshold / spell rule (include/sd_downscale.h, csrc/sd_spells.hip), vectorised over the cells: a loop over
the bins and the steps of a [T, C] field.

Per cell, over the steps of one bin in time order: x is the sample widened to double, t the threshold as double.  A step is valid when
neither is NaN, a hit when it is valid and ``x op t`` holds (one IEEE comparison; +-inf are ordinary values).  An invalid step is no hit
and ends a spell; spells are cut at the bin's ends.  The state (valid, hits, run, longest, days, spells) starts at zero and is updated
per step for the minimum spell length L >= 1:

    valid += is_valid;  hits += hit;  run = hit ? run + 1 : 0;  longest = max(longest, run)
    if run == L: days += L; spells += 1      elif run > L: days += 1

``fraction`` is one division hits / valid, NaN without a valid step; everything else of an empty or all-NaN bin is 0.  All values are
integers or one division of integers: the engine has to match bit for bit.

``brute`` is the independent check of the recurrence: the runs of one series found by ``itertools.groupby``
(tests/test_spells_host.py)."""
import itertools

import numpy as np

STATS = ("valid", "count", "fraction", "longest_spell", "spell_days", "spell_count")
COMPARE = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal}


def thresholds(threshold, T, C, group=None):
    """the threshold of every (step, cell) as float64 [T, C]: a number, [C], [1, C], or [G, C] with group [T]"""
    t = np.asarray(threshold, dtype=np.float64)
    if t.ndim == 2 and group is not None:
        t = t[np.asarray(group)]
    return np.broadcast_to(t, (T, C))


def spells(field, offsets, op, threshold, stats=STATS, min_length=1, group=None):
    """field [T, C] (float32 is widened first), offsets int [M + 1] -> float64 [len(stats) * M, C], row s * M + m"""
    x = np.asarray(field).astype(np.float64)
    T, C = x.shape
    offsets = np.asarray(offsets, dtype=np.int64)
    assert offsets[0] == 0 and offsets[-1] == T and (np.diff(offsets) >= 0).all() and min_length >= 1
    t = thresholds(threshold, T, C, group)
    M, L = len(offsets) - 1, int(min_length)
    res = {s: np.zeros((M, C)) for s in STATS}
    for m in range(M):
        valid, hits, run, longest, days, count = (np.zeros(C, dtype=np.int64) for _ in range(6))
        for r in range(offsets[m], offsets[m + 1]):  # time order
            ok = ~np.isnan(x[r]) & ~np.isnan(t[r])
            with np.errstate(invalid="ignore"):
                hit = ok & COMPARE[op](x[r], t[r])
            valid += ok
            hits += hit
            run = np.where(hit, run + 1, 0)
            longest = np.maximum(longest, run)
            days += np.where(run == L, L, np.where(run > L, 1, 0))
            count += run == L
        res["valid"][m], res["count"][m], res["longest_spell"][m], res["spell_days"][m], res["spell_count"][m] = valid, hits, longest, days, count
        with np.errstate(invalid="ignore", divide="ignore"):
            res["fraction"][m] = np.where(valid > 0, hits.astype(np.float64) / valid.astype(np.float64), np.nan)
    return np.concatenate([res[s] for s in ([stats] if isinstance(stats, str) else stats)])


def brute(series, threshold, op, min_length):
    """one bin of one cell by run lengths: series [n] float64, threshold a number or [n] -> dict of the six statistics"""
    x = np.asarray(series, dtype=np.float64)
    t = np.broadcast_to(np.asarray(threshold, dtype=np.float64), x.shape)
    valid = [not (np.isnan(a) or np.isnan(b)) for a, b in zip(x, t)]
    py = {">": lambda a, b: a > b, ">=": lambda a, b: a >= b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b}[op]
    hit = [v and bool(py(float(a), float(b))) for v, a, b in zip(valid, x, t)]
    runs = [len(list(g)) for k, g in itertools.groupby(hit) if k]
    long_runs = [n for n in runs if n >= min_length]
    return dict(valid=float(sum(valid)), count=float(sum(hit)), fraction=(sum(hit) / sum(valid) if sum(valid) else float("nan")),
                longest_spell=float(max(runs, default=0)), spell_days=float(sum(long_runs)), spell_count=float(len(long_runs)))
