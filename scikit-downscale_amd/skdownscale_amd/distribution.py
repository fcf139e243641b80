"""Distribution scores per cell on the GPU: ``GridArray.compare(obs).ks()`` / ``.perkins(width)`` / ``.distribution(names)`` -- what a
quantile-mapped field is judged by: whether its distribution matches that of the observations.

``ks``: the two-sample Kolmogorov-Smirnov distance, the largest difference of the two empirical distribution functions (what
``scipy.stats.ks_2samp(a, b).statistic`` gives for the two series with NaN dropped).  ``perkins``: the Perkins skill score, the overlap
of the two histograms with bins ``floor((x - origin) / width)``: the sum over the bins of the smaller of the two relative frequencies,
1 for identical distributions and 0 for disjoint ones.  ``na``, ``nb``: the non-NaN samples of each field.

The rule, per cell and bin (include/sd_downscale.h, restated in tests/_twosample_oracle.py): float32 samples are widened to double;
+-inf are ordinary values.  **Unlike the paired statistics of** ``skill.py``, which drop a step where either sample is NaN, each field
contributes its own non-NaN samples: ``na`` and ``nb`` may differ, and a NaN in one field does not remove the other's sample at that
step.  ``ks`` and ``perkins`` are NaN where either field has no sample.  Both are one division of integers, so the result does not
depend on the layout or on ``scratch_bytes``, bit for bit.

``DistributionGridArray`` has the surface of ``SkillGridArray`` and is fed the same way (``timesource.walk_pair``, blocks of whole
bins).  Limits: a bin holds at most 19 456 steps (``NotImplementedError`` beyond: 53 years of daily data in one bin), and one bin over
the whole axis needs both whole [T, C] fields in HBM.

On a grouped comparison (``compare(obs).groupby("time.season").ks()``, ``skill.py``) a group -- the steps that carry one label, anywhere
on the axis -- is evaluated exactly as one bin of its steps (sd_twosample_groups; tests/_grouped_pair_oracle.py): the same kernels read
their rows through the group-sorted row table.  Both sources come into HBM whole: ``2 * T * C * itemsize`` bytes, plus ``16 * C * T``
bytes of sorted runs where a group exceeds 1 216 steps; a group holds at most 19 456 steps.

Out of scope: p-values, CRPS and the Wasserstein distance, weighted samples, cftime calendars.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeferredGridArray
from .timesource import walk_pair

STATS = tuple(_lib.TWOSAMPLE_STATS)
INDEX_DIM = "index"


def check_statistics(names, width=None, origin=0.0):
    """the names as a tuple, with the histogram (width, origin) they need: (None, 0.0) where 'perkins' is not among them"""
    names = [names] if isinstance(names, str) else list(names)
    for n in names:
        if n not in STATS:
            raise ValueError(f"distribution statistic {n!r}: expected one of {', '.join(repr(s) for s in STATS)}")
    if not 1 <= len(names) <= len(STATS):
        raise ValueError(f"distribution() takes 1 to {len(STATS)} statistics, got {len(names)}")
    if "perkins" not in names:
        return tuple(names), None, 0.0
    if width is None:
        raise ValueError("perkins needs the width of the histogram bins: perkins(width) or distribution(names, width=...)")
    for what, v in (("width", width), ("origin", origin)):
        if isinstance(v, (bool, str)) or np.ndim(v) != 0 or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{what}: expected a {'positive ' if what == 'width' else ''}finite number, got {v!r}")
    if not width > 0:
        raise ValueError(f"width: expected a positive finite number, got {width!r}")
    return tuple(names), float(width), float(origin)


class DistributionGridArray(DeferredGridArray):
    """Distribution scores of a ``GridComparison`` per bin and cell.  Dims: the first source's, with the compared dim at the number of
    bins and the bin labels as its coordinate -- or replaced in place by the group dim with the sorted labels where the comparison was
    grouped, or dropped where it was neither: the whole axis is one bin --, and behind a leading ``"index"`` dim for
    ``distribution``."""

    def __init__(self, cmp, stats, width=None, origin=0.0, indexed=False, ctx=None):
        self._cmp, self._indexed, self._ctx = cmp, indexed, ctx
        self._stats, self._width, self._origin = check_statistics(stats, width, origin)
        self.dims, self.coords, self._sizes, self._order = cmp._result_layout(indexed, "distribution")
        if indexed:
            self.coords[INDEX_DIM] = np.array(self._stats)
        self.name = cmp._a.name

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        return dict({INDEX_DIM: len(self._stats)} if self._indexed else {}, **self._sizes)

    @property
    def comparison(self):
        return self._cmp

    @property
    def source(self):
        return self._cmp._a

    @property
    def other(self):
        return self._cmp._b

    @property
    def statistics(self):
        return self._stats

    @property
    def width(self):
        return self._width

    @property
    def origin(self):
        return self._origin

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices along the sources' other dims select from both sources (the result stays lazy); a selection along the compared dim
        or the index dim is made on the computed field"""
        if any(d in indexers for d in (self._cmp._dim, self._cmp.group_dim, INDEX_DIM)):
            return self.compute().isel(**indexers)
        return DistributionGridArray(self._cmp._isel(**indexers), self._stats, self._width, self._origin, self._indexed, self._ctx)

    # ---- the field ----
    def device_field(self, ctx=None):
        """the statistics as a [nstat * M, C] float64 DeviceArray, row ``s * M + m`` the statistic s of bin m (M = 1 where the
        comparison was not resampled; C = cells of the other dims in the first source's order, the last fastest).  Both sources are
        walked in the same blocks of whole bins, together at most ``scratch_bytes`` (``timesource.walk_pair``); where one is a lazy
        source that gives its field through ``device_field``, both are taken whole.  A bin is always evaluated within one block: the
        result does not depend on the block size, and one bin over the whole axis needs both whole fields in HBM.  A grouped
        comparison gives [nstat * G, C], row ``s * G + g``, from one call on both whole fields: ``2 * T * C * itemsize`` bytes of HBM,
        plus ``16 * C * T`` bytes of sorted runs where a group exceeds 1 216 steps."""
        ctx = self._context(ctx)
        c = self._cmp
        off = np.asarray(c.offsets, dtype=np.int64)
        M = len(off) - 1
        if c._groups is not None:  # one block of both: the whole axis (off is its one bin)
            G = len(c.group_labels)
            with walk_pair(c._a, c._b, c._dim, ctx, c._scratch_bytes, "any", bins=off) as w:
                out = w.result((len(self._stats) * G, w.cells))
                for _, _, block_a, block_b, _ in w:
                    ctx.twosample_groups(block_a, block_b, c.group, G, self._stats, width=self._width, origin=self._origin, out=out)
            return out
        with walk_pair(c._a, c._b, c._dim, ctx, c._scratch_bytes, "any", bins=off) as w:
            out = w.result((len(self._stats) * M, w.cells))
            for i0, i1, block_a, block_b, r0 in w:
                ctx.twosample(block_a, block_b, off[i0:i1 + 1] - r0, self._stats, width=self._width, origin=self._origin,
                              out=out.rows(i0, i1), plane_rows=M)
        return out

    def _field_order(self):
        return self._order

    def __repr__(self):
        return f"<DistributionGridArray {self.sizes} {', '.join(self._stats)} of {self._cmp!r} computed={self.computed}>"
