"""Paired skill statistics per cell on the GPU: ``GridArray.compare`` -- what a downscaled field is checked with against the
observations: bias, relative bias of the totals, MAE, RMSE, correlation and the ratio of the standard deviations, for the whole record or
per period.

``GridComparison`` is what ``a.compare(b)`` returns: the two arrays, checked to have the same dims (in any order), the same sizes and,
where both carry one, the same coordinate along the compared dim.  Nothing is aligned or broadcast, and nothing is computed yet.
``resample(time=rule)`` adds pandas' bins (``resample.time_bins``); without it the whole axis is one bin and the dim is dropped.
``groupby("time.month")`` / ``"time.season"`` / ``"time.dayofyear"``, ``groupby(time=labels)`` or ``groupby(time=MONTH_GROUPER,
name="month")`` pools the steps that carry one label over the whole axis -- the forty Julys of forty years -- into one group: what
``GridArray.groupby`` accepts for the compared dim, resolved by ``GridGroupBy`` (its labels, their sorted order, the group dim's name
and its error messages); the compared dim is replaced in place by the group dim.  ``resample`` and ``groupby`` exclude each other.
``count()``, ``bias()``, ``ratio()``, ``mae()``, ``rmse()``, ``corr()``, ``std_ratio()`` and ``indices(names)`` give a lazy
``SkillGridArray``, computed when the field is asked for -- on the host through ``values``, or as a ``DeviceArray`` through
``device_field``.

The rule, per cell over the steps of one bin in time order (include/sd_downscale.h, restated in tests/_skill_oracle.py): float32
samples are widened to double; a step is a valid pair when neither sample is NaN; every sum starts at +0.0 and adds one term per valid
pair in time order.  ``count``: the valid pairs n; ``bias``: sum(a - b) / n; ``ratio``: sum(a) / sum(b); ``mae``: sum|a - b| / n;
``rmse``: sqrt(sum((a - b)^2) / n); ``corr``: Pearson's r from the sums centred on the two means in a second pass, clamped to [-1, 1],
NaN for fewer than two pairs or a constant series; ``std_ratio``: sqrt(qaa / qbb) of the same centred sums.  Everything but ``count``
is NaN for a bin without a valid pair.  The summation order is fixed, so the result does not depend on the layout or on
``scratch_bytes``, bit for bit.

Both sources come into HBM through ``timesource.walk_pair``: cut into the same runs of whole bins so that the two blocks together stay
within ``scratch_bytes`` -- a host array uploaded block by block (float32 as float32), an unchunked ``coarse.interp_like(obs)`` regridded
block by block --, or, where one of them is a lazy ``resample`` / ``groupby`` / ``rolling`` / ``disaggregate`` / ``remap_like`` result
taken whole from HBM, both whole.  A bin always lies within one block of both; one bin over the whole axis therefore needs both whole
[T, C] fields in HBM.

A group is evaluated exactly as one bin whose steps are the rows with its label in time order (sd_skill_groups; restated in
tests/_grouped_pair_oracle.py): the result is, bit for bit, that of the binned statistics on the fields gathered group by group.  The
steps of a group lie anywhere on the axis, so a grouped comparison brings both sources into HBM whole, whatever ``scratch_bytes``:
``2 * T * C * itemsize`` bytes, plus -- for the distribution scores -- ``16 * C * T`` bytes of sorted runs where a group exceeds 1 216
steps.  Pooling the per-year results on the host afterwards is not the same statistic.

The distribution scores of the same comparison -- ``ks()``, ``perkins(width)``, ``distribution(names)`` -- are in ``distribution.py``;
they do not go through ``indices`` and, unlike the statistics here, take each field's own non-NaN samples.

Out of scope: streaming a grouped comparison block by block (the centred statistics would need the sources twice), alignment of
differing time axes, weighted statistics, cftime calendars.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeferredGridArray, GridArray
from .resample import DEFAULT_SCRATCH_BYTES, time_bins
from .timesource import walk_pair

STATS = tuple(_lib.SKILL_STATS)
INDEX_DIM = "index"


def check_statistics(names):
    names = [names] if isinstance(names, str) else list(names)
    for n in names:
        if n not in STATS:
            raise ValueError(f"skill statistic {n!r}: expected one of {', '.join(repr(s) for s in STATS)}")
    if not 1 <= len(names) <= len(STATS):
        raise ValueError(f"indices() takes 1 to {len(STATS)} statistics, got {len(names)}")
    return tuple(names)


def _first_difference(x, y):
    """the first position where two coordinates of equal length differ, None where they are equal (NaT / NaN equal themselves)"""
    x, y = np.asarray(x), np.asarray(y)
    try:
        differ = ~((x == y) | ((x != x) & (y != y)))
    except TypeError:
        differ = np.array([p != q for p, q in zip(x, y)])
    differ = np.broadcast_to(differ, x.shape)
    return int(np.flatnonzero(differ)[0]) if differ.any() else None


class GridComparison:
    """``GridArray.compare(other, dim)``: the comparison is stated, nothing is computed yet.  ``resample(time=rule)`` -> the same
    comparison over pandas' bins; ``bias()``, ``rmse()``, ``corr()``, ... -> ``SkillGridArray``."""

    def __init__(self, a, b, dim="time", scratch_bytes=DEFAULT_SCRATCH_BYTES, bins=None, rule=None, groups=None):
        if not isinstance(b, GridArray):
            raise ValueError(f"compare needs a GridArray with the dims {a.dims}, got {type(b).__name__}")
        if dim not in a.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {a.dims}")
        if set(b.dims) != set(a.dims) or len(b.dims) != len(a.dims):
            raise ValueError(f"other has dims {b.dims}; expected {a.dims} in any order (nothing is broadcast)")
        if any(b.sizes[d] != a.sizes[d] for d in a.dims):
            raise ValueError(f"other has sizes {b.sizes}; expected {a.sizes} (nothing is aligned)")
        if a.sizes[dim] == 0:
            raise ValueError(f"nothing to compare: dim {dim!r} has length 0")
        if dim in a.coords and dim in b.coords:
            at = _first_difference(a.coords[dim], b.coords[dim])
            if at is not None:
                raise ValueError(f"the {dim} coordinates differ at step {at}: {a.coords[dim][at]} and {b.coords[dim][at]} (nothing is aligned)")
        self._rest = rest = tuple(d for d in a.dims if d != dim)
        if tuple(d for d in b.dims if d != dim) != rest:  # the cells of both in the order of a's dims (a lazy other is computed for it)
            b = b.transpose(*a.dims)
        self._a, self._b, self._dim = a, b, dim
        self._scratch_bytes, self._bins, self._rule = int(scratch_bytes), bins, rule
        self._groups = groups  # (group dim, sorted labels, int32 id per step) of groupby(), else None

    def _like(self, a=None, b=None, bins=None, rule=None, groups=None):
        same = a is None
        return GridComparison(self._a if same else a, self._b if same else b, self._dim, self._scratch_bytes,
                              self._bins if bins is None else bins, self._rule if rule is None else rule,
                              self._groups if groups is None else groups)

    def _isel(self, **indexers):
        """the comparison on a selection along the other dims, made on both sources"""
        return self._like(self._a.isel(**indexers), self._b.isel(**indexers))

    @property
    def source(self):
        return self._a

    @property
    def other(self):
        return self._b

    @property
    def dim(self):
        return self._dim

    @property
    def labels(self):
        return None if self._bins is None else self._bins[0]

    @property
    def offsets(self):
        return np.array([0, self._a.sizes[self._dim]], dtype=np.int64) if self._bins is None else self._bins[1]

    @property
    def group_dim(self):
        return None if self._groups is None else self._groups[0]

    @property
    def group_labels(self):
        return None if self._groups is None else self._groups[1]

    @property
    def group(self):
        return None if self._groups is None else self._groups[2]

    @property
    def _rows(self):
        """(dim, labels) of the rows of a result: the compared dim with the bin labels, the group dim with the sorted group labels;
        None where the whole axis is one bin and the dim is dropped"""
        if self._groups is not None:
            return self._groups[0], self._groups[1]
        return None if self._bins is None else (self._dim, self._bins[0])

    def _result_layout(self, indexed, what):
        """(dims, coords, sizes, field order) of a result of this comparison: the first source's dims with the compared dim replaced
        in place by the rows' dim, or dropped; behind a leading ``"index"`` dim where ``indexed``"""
        src, rows = self._a, self._rows
        base = self._rest if rows is None else tuple(rows[0] if d == self._dim else d for d in src.dims)
        if indexed and INDEX_DIM in base:
            raise ValueError(f"the dim {INDEX_DIM!r} of {what}() is already a dim of this array {src.dims}")
        lead = (INDEX_DIM,) if indexed else ()
        coords = {k: v for k, v in src.coords.items() if k != self._dim}
        sizes = {}
        for d in src.dims:
            if d != self._dim:
                sizes[d] = src.sizes[d]
            elif rows is not None:
                sizes[rows[0]] = len(rows[1])
        if rows is not None:
            coords[rows[0]] = rows[1]
        order = lead + (() if rows is None else (rows[0],)) + self._rest
        return lead + base, coords, sizes, order

    _BOTH = "a comparison is evaluated over the bins of resample() or over the groups of groupby(), not both: {} after {}"

    def resample(self, indexer=None, **kwargs):
        """``resample(time=rule, **pandas_kw)``: the bins pandas' resampler makes of the dim's coordinate (``closed``, ``label``,
        ``offset``, ``origin`` go to pandas); every bin is evaluated by itself"""
        if self._groups is not None:
            raise ValueError(self._BOTH.format("resample()", "groupby()"))
        named = dict(indexer or {}, **{k: kwargs.pop(k) for k in list(kwargs) if k in self._a.dims})
        if list(named) != [self._dim]:
            raise ValueError(f"resample needs exactly {self._dim}=rule, the dim of this comparison, got {sorted(named)}")
        coords = self._a.coords if self._dim in self._a.coords else self._b.coords
        if self._dim not in coords:
            raise ValueError(f"neither array has a coordinate for dim {self._dim!r}")
        labels, offsets = time_bins(coords[self._dim], named[self._dim], **kwargs)
        if len(labels) == 0:
            raise ValueError(f"nothing to resample: dim {self._dim!r} has length 0")
        return self._like(bins=(labels, offsets), rule=named[self._dim])

    def groupby(self, group=None, name="group", **named):
        """``groupby("time.month")`` / ``"time.season"`` / ``"time.dayofyear"``, ``groupby(time=labels)`` or
        ``groupby(time=MONTH_GROUPER, name="month")``: what ``GridArray.groupby`` accepts for the compared dim, resolved by
        ``GridGroupBy`` on the coordinate of the first array (of the other where the first has none).  Every group -- all the steps
        that carry one label, pooled over the whole axis -- is evaluated as one bin of its steps in time order; the compared dim is
        replaced in place by the group dim, whose coordinate is the sorted labels.  Both sources come into HBM whole."""
        from .groupby import GridGroupBy

        if self._bins is not None:
            raise ValueError(self._BOTH.format("groupby()", "resample()"))
        if self._groups is not None:
            raise ValueError("this comparison is grouped already")
        dim = self._dim
        if isinstance(group, str) and group.count(".") == 1 and group.split(".")[0] != dim and not named:
            raise ValueError(f"group={group!r}: expected '{dim}.<field>', e.g. '{dim}.month', the dim of this comparison")
        if group is None and len(named) == 1 and dim not in named:
            raise ValueError(f"groupby needs {dim}=labels or {dim}=callable, the dim of this comparison, got {sorted(named)}")
        src = self._a if dim in self._a.coords or dim not in self._b.coords else self._b
        gb = GridGroupBy(src, group, named, name, self._scratch_bytes)
        return self._like(groups=(gb.group_dim, gb.labels, gb.group))

    # ---- the statistics ----
    def indices(self, names):
        """several statistics of this comparison from one call: a leading ``"index"`` dim whose coordinate is ``names``; both fields
        are read once per pass (two passes where ``corr`` or ``std_ratio`` is among them)"""
        return SkillGridArray(self, check_statistics(names), indexed=True)

    def _one(self, name):
        return SkillGridArray(self, (name,), indexed=False)

    def count(self):
        return self._one("count")

    def bias(self):
        return self._one("bias")

    def ratio(self):
        return self._one("ratio")

    def mae(self):
        return self._one("mae")

    def rmse(self):
        return self._one("rmse")

    def corr(self):
        return self._one("corr")

    def std_ratio(self):
        return self._one("std_ratio")

    # ---- the distribution scores (distribution.py) ----
    def distribution(self, names, width=None, origin=0.0):
        """several of ``'ks'``, ``'perkins'``, ``'na'``, ``'nb'`` from one call: a leading ``"index"`` dim whose coordinate is
        ``names``; both fields are sorted once.  ``width`` (> 0) and ``origin``: the histogram bins of ``'perkins'``"""
        from .distribution import DistributionGridArray

        return DistributionGridArray(self, names, width, origin, indexed=True)

    def ks(self):
        """the two-sample Kolmogorov-Smirnov distance of the two fields per bin and cell, each field's own non-NaN samples"""
        from .distribution import DistributionGridArray

        return DistributionGridArray(self, ("ks",))

    def perkins(self, width, origin=0.0):
        """the Perkins skill score per bin and cell: the overlap of the two histograms with bins floor((x - origin) / width)"""
        from .distribution import DistributionGridArray

        return DistributionGridArray(self, ("perkins",), width, origin)

    def __repr__(self):
        over = "the whole axis" if self._bins is None else f"{self._dim}={self._rule!r}: {len(self._bins[0])} bins"
        if self._groups is not None:
            over = f"{self._groups[0]}: {len(self._groups[1])} groups"
        return f"<GridComparison {self._a!r} with {self._b!r} along {self._dim} over {over}>"


class SkillGridArray(DeferredGridArray):
    """Statistics of a ``GridComparison`` per bin and cell.  Dims: the first source's, with the compared dim at the number of bins and
    the bin labels as its coordinate -- or replaced in place by the group dim with the sorted labels where the comparison was grouped,
    or dropped where it was neither: the whole axis is one bin --, and behind a leading ``"index"`` dim for ``indices``."""

    def __init__(self, cmp, stats, indexed=False, ctx=None):
        self._cmp, self._stats, self._indexed, self._ctx = cmp, check_statistics(stats), indexed, ctx
        self.dims, self.coords, self._sizes, self._order = cmp._result_layout(indexed, "indices")
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

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices along the sources' other dims select from both sources (the result stays lazy); a selection along the compared dim
        or the index dim is made on the computed field"""
        if any(d in indexers for d in (self._cmp._dim, self._cmp.group_dim, INDEX_DIM)):
            return self.compute().isel(**indexers)
        return SkillGridArray(self._cmp._isel(**indexers), self._stats, self._indexed, self._ctx)

    # ---- the field ----
    def device_field(self, ctx=None):
        """the statistics as a [nstat * M, C] float64 DeviceArray, row ``s * M + m`` the statistic s of bin m (M = 1 where the
        comparison was not resampled; C = cells of the other dims in the first source's order, the last fastest).  Both sources are
        walked in the same blocks of whole bins, together at most ``scratch_bytes`` (``timesource.walk_pair``); where one is a lazy
        source that gives its field through ``device_field``, both are taken whole.  A bin is always evaluated within one block: the
        result does not depend on the block size, and one bin over the whole axis needs both whole fields in HBM.  A grouped
        comparison gives [nstat * G, C], row ``s * G + g``, from one call on both whole fields (``2 * T * C * itemsize`` bytes of
        HBM)."""
        ctx = self._context(ctx)
        c = self._cmp
        off = np.asarray(c.offsets, dtype=np.int64)
        M = len(off) - 1
        if c._groups is not None:  # one block of both: the whole axis (off is its one bin)
            G = len(c.group_labels)
            with walk_pair(c._a, c._b, c._dim, ctx, c._scratch_bytes, "any", bins=off) as w:
                out = w.result((len(self._stats) * G, w.cells))
                for _, _, block_a, block_b, _ in w:
                    ctx.skill_groups(block_a, block_b, c.group, G, self._stats, out=out)
            return out
        with walk_pair(c._a, c._b, c._dim, ctx, c._scratch_bytes, "any", bins=off) as w:
            out = w.result((len(self._stats) * M, w.cells))
            for i0, i1, block_a, block_b, r0 in w:
                ctx.skill(block_a, block_b, off[i0:i1 + 1] - r0, self._stats, out=out.rows(i0, i1), plane_rows=M)
        return out

    def _field_order(self):
        return self._order

    def __repr__(self):
        return f"<SkillGridArray {self.sizes} {', '.join(self._stats)} of {self._cmp!r} computed={self.computed}>"
