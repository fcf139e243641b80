"""Resampling of the time axis on the GPU: the step of the reference's BCSD recipes that comes before ``fit``
(``resample('MS').mean()`` for temperature, ``.sum()`` for precipitation, ``interp_like(obs).resample(time='1d').mean()``).

``time_bins`` asks pandas' resampler for the bins -- it is the only place that does --, ``GridResample`` is what
``GridArray.resample`` returns, and ``ResampledGridArray`` is what its ``mean()`` / ``sum()`` return: the source and the bin table,
reduced when the field is asked for -- on the host through ``values``, or as an ``[M, C]`` ``DeviceArray`` through ``device_field``.
On ``coarse.interp_like(obs)`` the fine daily field is produced and reduced in HBM, block by block, and never crosses PCIe.

The rule is pandas' ``DataFrame.resample(rule, **kw).mean()`` / ``.sum()`` per cell: NaN samples are skipped; a bin without a non-NaN
sample -- a gap in the calendar or an all-NaN bin -- gives NaN for ``mean`` and 0.0 for ``sum`` (pandas' ``min_count=0``).  xarray's own
``resample().sum()`` may differ on empty bins; xarray is not installed where this project is developed, so that was not compared.
The result is float64 whatever the source (pandas keeps float32 for float32 input: a known deviation; float32 samples are widened
one by one on the device, so the values are those of the widened source).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .core import DeferredGridArray, chunk_lengths
from .timesource import walk

OPS = ("mean", "sum")
DEFAULT_SCRATCH_BYTES = 1 << 30
# what pandas' resampler offers beyond the two reductions the engine has: asked for by name, refused by name
_OTHER_REDUCTIONS = ("max", "min", "median", "std", "var", "sem", "prod", "first", "last", "count", "size", "nunique", "ohlc", "quantile",
                     "agg", "aggregate", "apply", "transform", "interpolate", "ffill", "bfill", "nearest", "asfreq", "pad", "backfill")


def time_bins(time, rule, **kw):
    """The bins pandas' resampler makes of a time coordinate: ``(labels, offsets)`` with ``labels`` the index of the resampled series
    (``M`` entries) and ``offsets`` int64 ``[M + 1]``, bin ``m`` = samples ``offsets[m] .. offsets[m + 1] - 1``.  ``kw`` goes to
    ``Series.resample`` (``closed``, ``label``, ``offset``, ``origin``); whatever pandas refuses raises pandas' error.  The coordinate
    must be monotonic non-decreasing (it is not sorted here): the bins are runs of consecutive samples only then."""
    index = time if isinstance(time, pd.Index) else pd.Index(np.asarray(time))
    if not index.is_monotonic_increasing:
        v = np.asarray(index)
        with np.errstate(invalid="ignore"):
            back = np.flatnonzero(v[1:] < v[:-1])
        if len(back):
            i = int(back[0]) + 1
            raise ValueError(f"the time coordinate is not monotonic non-decreasing: position {i} ({index[i]}) lies before position {i - 1} "
                             f"({index[i - 1]}); sort the array along time before resampling")
    counts = pd.Series(0, index=index).resample(rule, **kw).size()
    offsets = np.concatenate([[0], np.cumsum(counts.to_numpy(dtype=np.int64))]).astype(np.int64)
    if offsets[-1] != len(index):
        raise ValueError(f"the resampler kept {int(offsets[-1])} of the {len(index)} samples (NaT in the time coordinate?)")
    return counts.index, offsets


class GridResample:
    """``GridArray.resample(time=rule, **kw)``: the bins are made, nothing is reduced yet.  ``mean()`` / ``sum()`` ->
    ``ResampledGridArray``."""

    def __init__(self, source, dim, rule, kw=None, scratch_bytes=DEFAULT_SCRATCH_BYTES):
        if dim not in source.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {source.dims}")
        if dim not in source.coords:
            raise ValueError(f"the array has no coordinate for dim {dim!r}")
        self._source, self._dim, self._rule, self._kw, self._scratch_bytes = source, dim, rule, dict(kw or {}), scratch_bytes
        self.labels, self.offsets = time_bins(source.coords[dim], rule, **self._kw)
        if len(self.labels) == 0:
            raise ValueError(f"nothing to resample: dim {dim!r} has length 0")

    def _reduce(self, op):
        return ResampledGridArray(self._source, self._dim, self._rule, op, self._kw, scratch_bytes=self._scratch_bytes,
                                  bins=(self.labels, self.offsets))

    def mean(self):
        return self._reduce("mean")

    def sum(self):
        return self._reduce("sum")

    def __getattr__(self, name):
        if name in _OTHER_REDUCTIONS:
            def refuse(*args, **kwargs):
                raise NotImplementedError(f"resample(...).{name}(): only mean() and sum() are implemented")

            return refuse
        raise AttributeError(name)

    def __repr__(self):
        return f"<GridResample {self._dim}={self._rule!r}: {len(self.labels)} bins of {self._source.sizes[self._dim]} samples>"


class ResampledGridArray(DeferredGridArray):
    """A ``GridArray`` whose ``dim`` is reduced over pandas' bins of ``rule``: same dims, ``dim`` at the number of bins with the bin
    labels as its coordinate."""

    _kind = "resample"

    def __init__(self, source, dim, rule, op="mean", kw=None, ctx=None, scratch_bytes=DEFAULT_SCRATCH_BYTES, chunksizes=None, bins=None):
        if op not in OPS:
            raise NotImplementedError(f"resample reduction {op!r}: only mean and sum are implemented")
        self._source, self._dim, self._rule, self._op, self._kw = source, dim, rule, op, dict(kw or {})
        self._ctx = ctx
        self._scratch_bytes = int(scratch_bytes)
        self._labels, self._offsets = bins if bins is not None else time_bins(source.coords[dim], rule, **self._kw)
        self.dims = tuple(source.dims)
        self.coords = dict(source.coords)
        self.coords[dim] = self._labels
        self.name = source.name
        self.chunksizes = chunksizes

    def _like(self, source=None, chunksizes=None):
        same = source is None
        return ResampledGridArray(self._source if same else source, self._dim, self._rule, self._op, self._kw, self._ctx, self._scratch_bytes,
                                  chunksizes, bins=(self._labels, self._offsets))

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        s = dict(self._source.sizes)
        s[self._dim] = len(self._labels)
        return s

    @property
    def source(self):
        return self._source

    @property
    def offsets(self):
        return self._offsets

    def chunk(self, chunks):
        return self._like(chunksizes=chunk_lengths(self.sizes, chunks))

    def unchunked(self):
        return self if self.chunksizes is None else self._like()

    def isel(self, **indexers):
        """slices along the other dims select from the source (the result stays lazy); a selection along the resampled dim is made
        on the computed field"""
        if self._dim in indexers:
            return self.compute().isel(**indexers)
        return self._like(source=self._source.isel(**indexers))

    # ---- the reduced field ----
    def _rest_dims(self):
        return tuple(d for d in self.dims if d != self._dim)

    def _row_dim(self):
        return self._dim

    def _field_order(self):
        return (self._dim,) + self._rest_dims()

    def device_field(self, ctx=None):
        """the reduced field as an [M, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest).  The
        time axis is walked in blocks of whole bins of at most ``scratch_bytes`` (``timesource.walk``) and every block reduced into
        its rows of the result.  A bin is always reduced within one block, in time order: the result does not depend on the block
        size."""
        ctx = self._context(ctx)
        off = self._offsets
        with walk(self._source, self._dim, ctx, self._scratch_bytes, "resample", bins=off, verb="resample") as w:
            out = w.result((len(off) - 1, w.cells))
            for a, b, block, r0 in w:
                ctx.resample(block, off[a:b + 1] - r0, self._op, out=out.rows(a, b))
        return out

    def __repr__(self):
        return (f"<ResampledGridArray {self.sizes} {self._op} over {self._dim}={self._rule!r} of {self._source.sizes} "
                f"computed={self.computed}>")
