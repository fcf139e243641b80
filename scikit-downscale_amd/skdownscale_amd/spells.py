"""Threshold and spell indices per period on the GPU: ``GridArray.where`` -- what is counted on a downscaled daily series: frost days,
wet days (R1mm), the longest dry or wet spell (CDD / CWD), the days in warm spells of at least six days (WSDI), the share of days above
a day-of-year percentile (TX90p).

``GridCondition`` is what ``GridArray.where(op, threshold)`` returns: the source, the comparison and the threshold -- a number, one value
per cell, or with ``by=`` a table with one field per group of steps, its rows matched by label exactly as ``gb - other`` matches them
(it is ``GroupAppliedGridArray`` that matches them, and that takes a lazy climatology, grouped quantile or rolling statistic of one from
HBM).  Nothing is computed yet.  ``resample(time=rule)`` adds pandas' bins (``resample.time_bins``); without it the whole axis is one bin
and the dim is dropped.  ``valid()``, ``count()``, ``fraction()``, ``longest_spell()``, ``spell_days(min_length)``,
``spell_count(min_length)`` and ``indices(names, min_length)`` give a lazy ``SpellGridArray``, computed when the field is asked for -- on
the host through ``values``, or as a ``DeviceArray`` through ``device_field``.

The rule, per cell over the steps of one bin in time order (include/sd_downscale.h, restated in tests/_spells_oracle.py): a step is
valid when neither the sample nor its threshold is NaN; it is a hit when it is valid and ``sample op threshold`` holds, both as doubles
(+-inf are ordinary values); an invalid step is no hit and ends a spell; spells are cut at the ends of a bin (climdex's
``spells.can.span.years = FALSE``).  ``valid``: the valid steps; ``count``: the hits; ``fraction``: hits / valid, NaN for a bin without
a valid step; ``longest_spell``: the longest run of hits; ``spell_days`` / ``spell_count``: the steps inside and the number of the
runs of at least ``min_length`` hits.  An empty bin and an all-NaN bin give 0 (``fraction``: NaN).  All results are float64 and exact.

One deviation from NumPy 2: a float32 sample is widened and compared with the threshold as a double.  NumPy compares a float32 array
with a Python float in float32: ``np.float32(0.1) > 0.1`` is False there and True here.

The source is walked in blocks of whole bins of at most ``scratch_bytes`` as ``resample`` walks it -- a host array uploaded block by
block (float32 as float32), an unchunked ``coarse.interp_like(obs)`` regridded block by block --, and a lazy ``resample`` / ``groupby``
/ ``rolling`` / ``disaggregate`` / ``remap_like`` result is taken whole from HBM.  A bin always lies within one block, so the result does
not depend on ``scratch_bytes``; one bin over the whole axis therefore needs the whole [T, C] field in HBM, as ``quantile`` does.

Out of scope: comparison operators on ``GridArray`` itself, groups of non-consecutive steps (counts by calendar month over all years),
spells that span bins, cftime calendars.
"""
from __future__ import annotations

import numbers

import numpy as np

from . import _lib
from .core import DeferredGridArray, GridArray
from .groupby import GridGroupBy, GroupAppliedGridArray
from .resample import DEFAULT_SCRATCH_BYTES, time_bins
from .timesource import walk

OPS = tuple(_lib.SPELL_OPS)
STATS = tuple(_lib.SPELL_STATS)
INDEX_DIM = "index"


def check_min_length(min_length):
    if isinstance(min_length, bool) or not isinstance(min_length, numbers.Integral) or min_length < 1:
        raise ValueError(f"min_length={min_length!r}: expected an integer of at least 1")
    return int(min_length)


def check_statistics(names):
    names = [names] if isinstance(names, str) else list(names)
    for n in names:
        if n not in STATS:
            raise ValueError(f"spell statistic {n!r}: expected one of {', '.join(repr(s) for s in STATS)}")
    if not 1 <= len(names) <= len(STATS):
        raise ValueError(f"indices() takes 1 to {len(STATS)} statistics, got {len(names)}")
    return tuple(names)


class GridCondition:
    """``GridArray.where(op, threshold, dim, by)``: the comparison is stated, nothing is computed yet.  ``resample(time=rule)`` -> the
    same condition over pandas' bins; ``count()``, ``longest_spell()``, ... -> ``SpellGridArray``."""

    def __init__(self, source, op, threshold, dim="time", by=None, name="group", scratch_bytes=DEFAULT_SCRATCH_BYTES, bins=None, rule=None):
        if op not in OPS:
            raise ValueError(f"where op {op!r}: expected one of {', '.join(repr(o) for o in OPS)}")
        if dim not in source.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {source.dims}")
        if source.sizes[dim] == 0:
            raise ValueError(f"nothing to count: dim {dim!r} has length 0")
        self._source, self._op, self._dim, self._by, self._name = source, op, dim, by, name
        self._scratch_bytes, self._bins, self._rule = int(scratch_bytes), bins, rule
        self._rest = rest = tuple(d for d in source.dims if d != dim)
        want = tuple(source.sizes[d] for d in rest)
        self._applied = None
        if not isinstance(threshold, GridArray) and np.ndim(threshold) == 0:
            if by is not None:
                raise ValueError(f"by={by!r} needs a threshold table with one field per group; a number is compared with every step")
            self._threshold = float(threshold)
        elif by is None:  # one value per cell
            if isinstance(threshold, GridArray):
                if set(threshold.dims) != set(rest) or len(threshold.dims) != len(rest):
                    raise ValueError(f"threshold has dims {threshold.dims}; expected {rest} (with by=, the group dim beside them)")
                if any(threshold.sizes[d] != source.sizes[d] for d in rest):
                    raise ValueError(f"threshold has sizes {threshold.sizes}; expected { {d: source.sizes[d] for d in rest} }")
                self._threshold = threshold
            else:
                cell = np.asarray(threshold, dtype=np.float64)
                if cell.shape != want:
                    raise ValueError(f"threshold has shape {cell.shape}; expected {want}: one value per cell")
                self._threshold = GridArray(cell, rest)
        else:
            if isinstance(by, str):
                if by.count(".") != 1 or by.split(".")[0] != dim:
                    raise ValueError(f"by={by!r}: expected '{dim}.<field>', e.g. '{dim}.month', labels or a callable for dim {dim!r}")
                gb = GridGroupBy(source, by, scratch_bytes=self._scratch_bytes)
            else:
                gb = GridGroupBy(source, None, {dim: by}, name, self._scratch_bytes)
            other = threshold if isinstance(threshold, GridArray) else np.asarray(threshold, dtype=np.float64)
            self._applied = GroupAppliedGridArray(gb, other, "sub")  # (never computed: it matches the rows and gives the table)
            self._threshold = other if isinstance(other, GridArray) else GridArray(other, (gb.group_dim,) + rest, {gb.group_dim: gb.labels})

    def _like(self, source=None, threshold=None, bins=None, rule=None):
        same = source is None
        return GridCondition(self._source if same else source, self._op, self._threshold if same else threshold, self._dim, self._by, self._name,
                             self._scratch_bytes, self._bins if bins is None else bins, self._rule if rule is None else rule)

    def _isel(self, **indexers):
        """the condition on a selection along the other dims (the threshold follows)"""
        t = self._threshold
        return self._like(self._source.isel(**indexers), t.isel(**indexers) if isinstance(t, GridArray) else t)

    @property
    def source(self):
        return self._source

    @property
    def op(self):
        return self._op

    @property
    def dim(self):
        return self._dim

    @property
    def threshold(self):
        return self._threshold

    @property
    def group(self):
        """per step, the row of the threshold table it is compared with (None for a number or a per-cell threshold)"""
        return None if self._applied is None else self._applied.group

    @property
    def labels(self):
        return None if self._bins is None else self._bins[0]

    @property
    def offsets(self):
        return np.array([0, self._source.sizes[self._dim]], dtype=np.int64) if self._bins is None else self._bins[1]

    def resample(self, indexer=None, **kwargs):
        """``resample(time=rule, **pandas_kw)``: the bins pandas' resampler makes of the dim's coordinate (``closed``, ``label``,
        ``offset``, ``origin`` go to pandas); every bin is evaluated by itself"""
        named = dict(indexer or {}, **{k: kwargs.pop(k) for k in list(kwargs) if k in self._source.dims})
        if list(named) != [self._dim]:
            raise ValueError(f"resample needs exactly {self._dim}=rule, the dim of this condition, got {sorted(named)}")
        if self._dim not in self._source.coords:
            raise ValueError(f"the array has no coordinate for dim {self._dim!r}")
        labels, offsets = time_bins(self._source.coords[self._dim], named[self._dim], **kwargs)
        if len(labels) == 0:
            raise ValueError(f"nothing to resample: dim {self._dim!r} has length 0")
        return self._like(bins=(labels, offsets), rule=named[self._dim])

    # ---- the indices ----
    def indices(self, names, min_length=1):
        """several statistics of this condition from one pass over the field: a leading ``"index"`` dim whose coordinate is ``names``"""
        return SpellGridArray(self, check_statistics(names), min_length, indexed=True)

    def _one(self, name, min_length=1):
        return SpellGridArray(self, (name,), min_length, indexed=False)

    def valid(self):
        return self._one("valid")

    def count(self):
        return self._one("count")

    def fraction(self):
        return self._one("fraction")

    def longest_spell(self):
        return self._one("longest_spell")

    def spell_days(self, min_length):
        return self._one("spell_days", min_length)

    def spell_count(self, min_length):
        return self._one("spell_count", min_length)

    def __repr__(self):
        what = f"{self._threshold!r}" if self._applied is None else f"{self._threshold!r} by {self._applied._gdim}"
        over = "the whole axis" if self._bins is None else f"{self._dim}={self._rule!r}: {len(self._bins[0])} bins"
        return f"<GridCondition {self._dim} {self._op} {what} over {over} of {self._source.sizes}>"


class SpellGridArray(DeferredGridArray):
    """Statistics of a ``GridCondition`` per bin and cell.  Dims: the source's, with the condition's dim at the number of bins and the
    bin labels as its coordinate -- or dropped where the condition was not resampled: the whole axis is one bin --, and behind a
    leading ``"index"`` dim for ``indices``."""

    def __init__(self, cond, stats, min_length=1, indexed=False, ctx=None):
        self._cond, self._stats, self._min_length, self._indexed, self._ctx = cond, check_statistics(stats), check_min_length(min_length), indexed, ctx
        src, dim = cond._source, cond._dim
        base = tuple(src.dims) if cond._bins is not None else cond._rest
        if indexed and INDEX_DIM in base:
            raise ValueError(f"the dim {INDEX_DIM!r} of indices() is already a dim of this array {src.dims}")
        self.dims = ((INDEX_DIM,) if indexed else ()) + base
        self.coords = {k: v for k, v in src.coords.items() if k != dim}
        if cond._bins is not None:
            self.coords[dim] = cond._bins[0]
        if indexed:
            self.coords[INDEX_DIM] = np.array(self._stats)
        self.name = src.name

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        c = self._cond
        s = {INDEX_DIM: len(self._stats)} if self._indexed else {}
        for d, n in c._source.sizes.items():
            if d != c._dim:
                s[d] = n
            elif c._bins is not None:
                s[d] = len(c._bins[0])
        return s

    @property
    def condition(self):
        return self._cond

    @property
    def source(self):
        return self._cond._source

    @property
    def statistics(self):
        return self._stats

    @property
    def min_length(self):
        return self._min_length

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices along the source's other dims select from the source and the threshold (the result stays lazy); a selection along
        the condition's dim or the index dim is made on the computed field"""
        if any(d in indexers for d in (self._cond._dim, INDEX_DIM)):
            return self.compute().isel(**indexers)
        return SpellGridArray(self._cond._isel(**indexers), self._stats, self._min_length, self._indexed, self._ctx)

    # ---- the field ----
    def _threshold_on(self, ctx):
        """(number or [G, C] DeviceArray the caller frees, group ids or None)"""
        c = self._cond
        if c._applied is not None:
            return c._applied._table(ctx), c._applied.group
        t = c._threshold
        if not isinstance(t, GridArray):
            return t, None
        v = np.ascontiguousarray((t if tuple(t.dims) == c._rest else t.transpose(*c._rest)).values, dtype=np.float64)
        return ctx.to_device(v.reshape(1, -1)), None

    def device_field(self, ctx=None):
        """the statistics as a [nstat * M, C] float64 DeviceArray, row ``s * M + m`` the statistic s of bin m (M = 1 where the
        condition was not resampled; C = cells of the other dims in their order, the last fastest).  The time axis is walked in blocks
        of whole bins of at most ``scratch_bytes`` as ``ResampledGridArray.device_field`` walks it; a lazy source that gives its field
        through ``device_field`` is taken whole.  A bin is always evaluated within one block: the result does not depend on the block
        size, and one bin over the whole axis needs the whole field in HBM."""
        ctx = self._context(ctx)
        c = self._cond
        off = np.asarray(c.offsets, dtype=np.int64)
        M = len(off) - 1
        thr, group = self._threshold_on(ctx)
        try:
            with walk(c._source, c._dim, ctx, c._scratch_bytes, "any", bins=off, verb="count") as w:
                out = w.result((len(self._stats) * M, w.cells))
                for a, b, block, r0 in w:
                    ctx.spells(block, c._op, thr, off[a:b + 1] - r0, self._stats, self._min_length,
                               None if group is None else group[r0:int(off[b])], out=out.rows(a, b), plane_rows=M)
            return out
        finally:
            if not isinstance(thr, float):
                thr.free()

    def _field_order(self):
        c = self._cond
        return ((INDEX_DIM,) if self._indexed else ()) + ((c._dim,) if c._bins is not None else ()) + c._rest

    def __repr__(self):
        what = ", ".join(self._stats) + (f" (min_length={self._min_length})" if self._min_length != 1 else "")
        return f"<SpellGridArray {self.sizes} {what} of {self._cond!r} computed={self.computed}>"
