"""NumPy restatement of the paired skill rule (include/sd_downscale.h, csrc/sd_skill.hip): an explicit loop over the bins and the rows
of a bin of two [T, C] fields, vectorised over the cells.  It is the definition, so the kernel is compared with it bit for bit.

Per cell, over the steps of one bin in time order: a float32 sample is widened to double first.  A step is a valid pair when neither a
nor b is NaN (+-inf are ordinary values).  Every sum starts at +0.0 and adds one term per valid pair, ((+0.0 + t1) + t2) + ...; an
invalid pair adds +0.0, which changes no bit (no sum of two doubles is -0.0 unless both are).  One IEEE operation per step, a product
and the addition of it are two.

    pass 1    n = the valid pairs, sa = sum a, sb = sum b, sd = sum (a - b), sabs = sum |a - b|, sq = sum (a - b) * (a - b)
    pass 2    ma = sa / n, mb = sb / n; qaa = sum (a - ma)^2, qbb = sum (b - mb)^2, qab = sum (a - ma) * (b - mb)

    count      n; 0 for an empty or all-invalid bin
    bias       sd / n
    ratio      sa / sb as IEEE gives it
    mae        sabs / n
    rmse       sqrt(sq / n)
    corr       qab / (sqrt(qaa) * sqrt(qbb)) clamped to [-1, 1], NaN staying NaN; NaN where n < 2, qaa == 0 or qbb == 0
    std_ratio  sqrt(qaa / qbb); NaN where n < 2
    all but count: NaN where n == 0

``sums_by_cells`` is the same rule with the loops exchanged -- one cell after the other, its rows in a plain Python loop over Python
floats --: tests/test_skill_host.py compares the two bit for bit.

Against plain NumPy over the valid pairs (``np.mean(d)``, ``np.sqrt(np.mean(d * d))``, ``np.corrcoef`` and their like: ``numpy_skill``)
the NaN pattern is identical and the values agree within a measured bound: NumPy sums pairwise, so the difference cannot be derived
from the rule.  Measured against NumPy 2 on ``field()`` (T = 400, 6 cells: a run of 40 NaN in one source, isolated NaN in the other, a
zero-inflated cell; the whole axis as one bin and ten bins of 40 rows, one of them without a valid pair in cell 1; ``python
tests/_skill_oracle.py`` prints them), as multiples of a scale: the largest |a - b| over the valid pairs of the field for bias, mae and
rmse; the largest |value| of the statistic over the field for ratio and std_ratio; 1 for corr; count is exact.

    bias       measured 2.5e-17 * max|a - b|      tolerance 8 x = 2.0e-16 * max|a - b|
    mae        measured 8.0e-17 * max|a - b|      tolerance 8 x = 6.4e-16 * max|a - b|
    rmse       measured 1.6e-16 * max|a - b|      tolerance 8 x = 1.28e-15 * max|a - b|
    ratio      measured 2.5e-15 * max|ratio|      tolerance 8 x = 2.0e-14 * max|ratio|
    corr       measured 5.6e-16                   tolerance 8 x = 4.48e-15
    std_ratio  measured 2.4e-15 * max|std_ratio|  tolerance 8 x = 1.92e-14 * max|std_ratio|

The factor 8 covers another NumPy and another summation blocking.
"""
import warnings

import numpy as np

STATS = ("count", "bias", "ratio", "mae", "rmse", "corr", "std_ratio")
CENTRED = ("corr", "std_ratio")
MEASURED = {"count": 0.0, "bias": 2.5e-17, "ratio": 2.5e-15, "mae": 8.0e-17, "rmse": 1.6e-16, "corr": 5.6e-16, "std_ratio": 2.4e-15}
TOLERANCE = {s: 8 * m for s, m in MEASURED.items()}


def _check(a, b, offsets):
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    assert a.ndim == 2 and a.shape == b.shape
    offsets = np.asarray(offsets, dtype=np.int64)
    assert offsets[0] == 0 and offsets[-1] == a.shape[0] and (np.diff(offsets) >= 0).all()
    return a, b, offsets


def sums_by_rows(a, b, offsets, second=True):
    """a, b [T, C], offsets [M + 1] -> dict of [M, C] arrays: n (int64) and sa, sb, sd, sabs, sq, qaa, qbb, qab.  The definition: a
    loop over the bins and the rows of a bin in time order, vectorised over the cells"""
    a, b, offsets = _check(a, b, offsets)
    M, C = len(offsets) - 1, a.shape[1]
    res = {k: np.zeros((M, C)) for k in ("sa", "sb", "sd", "sabs", "sq", "qaa", "qbb", "qab")}
    res["n"] = np.zeros((M, C), dtype=np.int64)
    with np.errstate(all="ignore"):
        for m in range(M):
            n = np.zeros(C, dtype=np.int64)
            sa, sb, sd, sabs, sq, qaa, qbb, qab = (np.zeros(C) for _ in range(8))
            for r in range(offsets[m], offsets[m + 1]):  # time order
                ok = (a[r] == a[r]) & (b[r] == b[r])
                d = a[r] - b[r]
                n += ok
                sa = sa + np.where(ok, a[r], 0.0)
                sb = sb + np.where(ok, b[r], 0.0)
                sd = sd + np.where(ok, d, 0.0)
                sabs = sabs + np.where(ok, np.abs(d), 0.0)
                sq = sq + np.where(ok, d * d, 0.0)
            if second:
                ma, mb = sa / n, sb / n  # (NaN for n == 0: nothing is added then)
                for r in range(offsets[m], offsets[m + 1]):
                    ok = (a[r] == a[r]) & (b[r] == b[r])
                    da, db = a[r] - ma, b[r] - mb
                    qaa = qaa + np.where(ok, da * da, 0.0)
                    qbb = qbb + np.where(ok, db * db, 0.0)
                    qab = qab + np.where(ok, da * db, 0.0)
            for k, v in dict(n=n, sa=sa, sb=sb, sd=sd, sabs=sabs, sq=sq, qaa=qaa, qbb=qbb, qab=qab).items():
                res[k][m] = v
    return res


def sums_by_cells(a, b, offsets):
    """``sums_by_rows`` with the loops exchanged: one cell after the other, the rows of each bin in a Python loop over Python floats
    (IEEE doubles: one rounding per operation)"""
    a, b, offsets = _check(a, b, offsets)
    M, C = len(offsets) - 1, a.shape[1]
    res = {k: np.zeros((M, C)) for k in ("sa", "sb", "sd", "sabs", "sq", "qaa", "qbb", "qab")}
    res["n"] = np.zeros((M, C), dtype=np.int64)
    nan = float("nan")
    for c in range(C):
        for m in range(M):
            pairs = [(float(x), float(y)) for x, y in zip(a[offsets[m]:offsets[m + 1], c], b[offsets[m]:offsets[m + 1], c]) if x == x and y == y]
            n, sa, sb, sd, sabs, sq = 0, 0.0, 0.0, 0.0, 0.0, 0.0
            for x, y in pairs:
                d = _sub(x, y)
                n, sa, sb, sd, sabs, sq = n + 1, sa + x, sb + y, sd + d, sabs + abs(d), sq + _mul(d, d)
            ma, mb = (sa / n, sb / n) if n else (nan, nan)
            qaa = qbb = qab = 0.0
            for x, y in pairs:
                da, db = _sub(x, ma), _sub(y, mb)
                qaa, qbb, qab = qaa + _mul(da, da), qbb + _mul(db, db), qab + _mul(da, db)
            for k, v in dict(n=n, sa=sa, sb=sb, sd=sd, sabs=sabs, sq=sq, qaa=qaa, qbb=qbb, qab=qab).items():
                res[k][m, c] = v
    return res


def _sub(x, y):  # (inf - inf is NaN, without Python's complaints)
    with np.errstate(all="ignore"):
        return float(np.float64(x) - np.float64(y))


def _mul(x, y):
    with np.errstate(all="ignore"):
        return float(np.float64(x) * np.float64(y))


def finish(s, stats=STATS):
    """the sums -> float64 [len(stats) * M, C], row i * M + m the statistic stats[i] of bin m"""
    n = s["n"]
    dn = n.astype(np.float64)
    nan = np.nan
    out = []
    with np.errstate(all="ignore"):
        for name in ([stats] if isinstance(stats, str) else stats):
            if name == "count":
                out.append(dn)
                continue
            if name == "bias":
                r = s["sd"] / dn
            elif name == "ratio":
                r = s["sa"] / s["sb"]
            elif name == "mae":
                r = s["sabs"] / dn
            elif name == "rmse":
                r = np.sqrt(s["sq"] / dn)
            elif name == "corr":
                r = s["qab"] / (np.sqrt(s["qaa"]) * np.sqrt(s["qbb"]))
                r = np.where(r > 1.0, 1.0, np.where(r < -1.0, -1.0, r))
                r = np.where((n < 2) | (s["qaa"] == 0.0) | (s["qbb"] == 0.0), nan, r)
            elif name == "std_ratio":
                r = np.where(n < 2, nan, np.sqrt(s["qaa"] / s["qbb"]))
            else:
                raise ValueError(name)
            out.append(np.where(n == 0, nan, r))
    return np.concatenate(out)


def skill(a, b, offsets, stats=STATS):
    """a, b [T, C] (float32 is widened first), offsets int [M + 1] -> float64 [len(stats) * M, C], row s * M + m"""
    names = [stats] if isinstance(stats, str) else list(stats)
    return finish(sums_by_rows(a, b, offsets, second=any(s in CENTRED for s in names)), names)


# ---- the measurement against plain NumPy ----------------------------------------------------------------------------------------------
T, CELLS = 400, 6
BINS = np.arange(0, T + 1, 40)


def field():
    """the deterministic pair (a, b) [400, 6] of the measurement, made with integer arithmetic alone (the same bits everywhere): cell 0
    plain; cell 1 a run of 40 NaN in a (rows 120 .. 159: bin 3 of BINS has no valid pair there); cell 2 isolated NaN in b; cell 3
    zero-inflated in both (precipitation); cell 4 NaN in both, partly at the same steps; cell 5 large offset (temperatures in K)"""
    t = np.arange(T, dtype=np.int64)[:, None]
    c = np.arange(CELLS, dtype=np.int64)[None, :]
    u = ((t * 7919 + c * 104729 + 12345) * 1103515245 + 12345) % 2147483648  # an LCG step per (row, cell)
    w = ((u // 7 + t * 31 + c * 17) * 1103515245 + 54321) % 2147483648
    a = (u % 20011).astype(np.float64) / 1000.0 - 10.0  # [-10, 10.01) in steps of 1e-3
    b = a + (w % 4001).astype(np.float64) / 2000.0 - 0.7  # a + [-0.7, 1.3]
    a[120:160, 1] = np.nan
    b[(u[:, 2] % 23) == 0, 2] = np.nan
    wet_a, wet_b = (u[:, 3] % 10) < 3, (w[:, 3] % 10) < 3
    a[:, 3] = np.where(wet_a, np.abs(a[:, 3]), 0.0)
    b[:, 3] = np.where(wet_b, np.abs(b[:, 3]), 0.0)
    a[(u[:, 4] % 11) == 0, 4] = np.nan
    b[(u[:, 4] % 22) == 0, 4] = np.nan
    b[(w[:, 4] % 13) == 0, 4] = np.nan
    a[:, 5] += 285.0
    b[:, 5] += 285.0
    return a, b


def numpy_skill(a, b, offsets, stats=STATS):
    """plain NumPy over the valid pairs of every bin and cell (pairwise sums) -> [len(stats) * M, C]"""
    a, b, offsets = _check(a, b, offsets)
    M, C = len(offsets) - 1, a.shape[1]
    names = [stats] if isinstance(stats, str) else list(stats)
    out = np.full((len(names), M, C), np.nan)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for m in range(M):
            for c in range(C):
                x, y = a[offsets[m]:offsets[m + 1], c], b[offsets[m]:offsets[m + 1], c]
                ok = ~np.isnan(x) & ~np.isnan(y)
                x, y = x[ok], y[ok]
                d = x - y
                for i, name in enumerate(names):
                    if name == "count":
                        out[i, m, c] = len(x)
                    elif len(x) == 0:
                        continue
                    elif name == "bias":
                        out[i, m, c] = np.mean(d)
                    elif name == "ratio":
                        out[i, m, c] = np.sum(x) / np.sum(y)
                    elif name == "mae":
                        out[i, m, c] = np.mean(np.abs(d))
                    elif name == "rmse":
                        out[i, m, c] = np.sqrt(np.mean(d * d))
                    elif len(x) < 2:
                        continue
                    elif name == "corr":
                        out[i, m, c] = np.corrcoef(x, y)[0, 1]
                    elif name == "std_ratio":
                        out[i, m, c] = np.std(x) / np.std(y)
    return out.reshape(len(names) * M, C)


def scale(a, b, stat, want):
    """what the NumPy tolerances are multiples of"""
    if stat in ("bias", "mae", "rmse"):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return float(np.nanmax(np.abs(a - b)))
    if stat in ("ratio", "std_ratio"):
        return float(np.nanmax(np.abs(want)))
    return 1.0


def distance(got, want, a, b, stat):
    """max |got - want| in units of ``scale``, over the entries that are not NaN in both"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = ~(np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)[both]
    return float(d.max() / scale(a, b, stat, want)) if d.size else 0.0


def check(got, want, a, b, stat, what=""):
    """NaN pattern identical, everything else within TOLERANCE[stat] of the scale"""
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    d = distance(got, want, a, b, stat)
    assert d <= TOLERANCE[stat], f"{what}: differs by {d:.3e} of the scale, allowed {TOLERANCE[stat]:.3e}"
    return d


if __name__ == "__main__":  # the measured distances of the docstring
    a, b = field()
    worst = dict.fromkeys(STATS, 0.0)
    for name, offsets in (("whole axis", np.array([0, T])), ("ten bins", BINS)):
        M = len(offsets) - 1
        got = skill(a, b, offsets).reshape(len(STATS), M, CELLS)
        want = numpy_skill(a, b, offsets).reshape(len(STATS), M, CELLS)
        for i, s in enumerate(STATS):
            assert np.array_equal(np.isnan(got[i]), np.isnan(want[i])), (name, s)
            d = distance(got[i], want[i], a, b, s)
            worst[s] = max(worst[s], d)
            print(f"{name:12s} {s:10s} {d:.3e}")
    print({s: f"{v:.2e}" for s, v in worst.items()})
