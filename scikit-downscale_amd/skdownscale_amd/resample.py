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

from . import _lib
from .core import DeferredGridArray, chunk_lengths

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


def _bin_blocks(offsets, max_rows):
    """the bins in consecutive runs [m0, m1) of at most ``max_rows`` samples -- at least one bin, however long, and at least one
    sample (a run of empty bins joins its neighbour)"""
    M = len(offsets) - 1
    blocks, m0 = [], 0
    for m in range(1, M + 1):
        have = offsets[m] - offsets[m0]
        if m == M or (have > 0 and offsets[m + 1] - offsets[m0] > max_rows):
            blocks.append((m0, m))
            m0 = m
    if len(blocks) > 1 and offsets[blocks[-1][1]] == offsets[blocks[-1][0]]:
        (a, _), (_, b) = blocks[-2], blocks[-1]
        blocks[-2:] = [(a, b)]
    return blocks


def resident_source(src, dim):
    """``src`` when it is an unchunked ``coarse.interp_like(obs)`` with dims (dim, y, x): its fine field can be produced in HBM, block
    of rows by block of rows (``src._regridder_on(ctx).regrid(src._coarse_stack()[r0:r1], out=block)``); else None.  The rule of every
    lazy array that walks the time axis of a source (``ResampledGridArray``, the groupby arrays).  Likewise ``src`` when it is a not
    yet computed ``fine.remap_like(coarse)`` with those dims over a host array: a block of fine rows is uploaded and remapped into
    the block."""
    from .regrid import InterpolatedGridArray
    from .remap import RemappedGridArray

    if isinstance(src, RemappedGridArray) and (src.computed or not src._host_source()):
        return None
    if (not isinstance(src, (InterpolatedGridArray, RemappedGridArray)) or len(src.dims) != 3 or src.dims[0] != dim
            or src._lead_dims() != src.dims[:1]):
        return None
    if src.chunksizes is not None and any(len(src.chunksizes[d]) > 1 for d in src.dims[1:]):
        return None
    return src


def host_rows(src, dim):
    """``src`` as a host [T, C] array, ``dim`` first and the other dims flattened in their order; float32 stays float32"""
    rest = tuple(d for d in src.dims if d != dim)
    v = _lib.as_field((src.transpose(dim, *rest) if src.dims[0] != dim else src).values)
    return v.reshape(v.shape[0], -1)


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

    def _resident_source(self):
        return resident_source(self._source, self._dim)

    def _host_rows(self):
        return host_rows(self._source, self._dim)

    def device_field(self, ctx=None):
        """the reduced field as an [M, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest).  The
        time axis is walked in blocks of whole bins of at most ``scratch_bytes``: a block of ``coarse.interp_like(obs)`` is regridded
        into device scratch, a block of a host array is uploaded into it (float32 as float32), and reduced into its rows of the
        result.  A bin is always reduced within one block, in time order: the result does not depend on the block size."""
        ctx = self._context(ctx)
        off = self._offsets
        M = len(off) - 1
        resident = self._resident_source()
        if resident is not None:
            rg = resident._regridder_on(ctx)
            rows, dtype = resident._coarse_stack(), np.dtype(np.float64)
            C = int(np.prod(rg.shape_out, dtype=np.int64))
        else:
            rows = self._host_rows()
            dtype, C = rows.dtype, rows.shape[1]
        if C < 1:
            raise ValueError(f"nothing to resample: the array has sizes {self._source.sizes}")
        max_rows = max(1, self._scratch_bytes // (C * dtype.itemsize))
        blocks = _bin_blocks(off, max_rows)
        scratch = ctx.empty((max(int(off[b] - off[a]) for a, b in blocks), C), dtype)
        out = ctx.empty((M, C))
        for a, b in blocks:
            r0, r1 = int(off[a]), int(off[b])
            block = scratch.rows(0, r1 - r0)
            if resident is not None:
                rg.regrid(rows[r0:r1], out=block)
            else:
                block.copy_from_host(rows[r0:r1])
            ctx.resample(block, off[a:b + 1] - r0, self._op, out=out.rows(a, b))
        scratch.free()
        return out

    def _compute_values(self):
        field = self.device_field()
        vals = self._in_dims(field.to_host(), (self._dim,) + self._rest_dims())
        field.free()
        return vals

    def __repr__(self):
        return (f"<ResampledGridArray {self.sizes} {self._op} over {self._dim}={self._rule!r} of {self._source.sizes} "
                f"computed={self.computed}>")
