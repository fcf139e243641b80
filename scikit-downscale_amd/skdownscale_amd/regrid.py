"""Regridding of coarse fields on the GPU: the step of the reference's gridded workflow that comes before
``PointWiseDownscaler.fit`` (``da.interp_like(obs.isel(time=0, drop=True), method='linear')``).

``Regridder`` owns the engine's tables for one (source grid, target grid, method); ``InterpolatedGridArray`` is what
``GridArray.interp_like`` / ``GridArray.interp`` return: it keeps the coarse data and produces the fine field when it is asked for --
on the host through ``values``, or as a ``[T, C]`` ``DeviceArray`` through ``device_field`` without the fine field ever crossing PCIe.

The rule is xarray's for 1-D coordinates: one ``scipy.interpolate.interp1d(bounds_error=False, fill_value=nan,
assume_sorted=False)`` per dimension, the first spatial dim of the field before the second (csrc/sd_regrid_plan.h restates it).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .core import DEFAULT_FEATURE_DIM, DeferredGridArray, _block_slices, chunk_lengths
from .timesource import RowProducer

METHODS = ("linear", "nearest")
PASS_THROUGH_DIMS = ("time", DEFAULT_FEATURE_DIM)  # never interpolated over


def _coordinate(which, name, values):
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError(f"{which} coordinate {name!r} must be one-dimensional, got shape {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if np.isnan(a).any():
        raise ValueError(f"{which} coordinate {name!r} contains NaN")
    return a


class Regridder:
    """Bilinear (``'linear'``) or nearest-neighbour interpolation between two rectilinear grids.

    ``src_coords``: mapping of exactly two dim names to 1-D coordinates, in the order of the field's spatial dims (the first one is
    interpolated first); strictly ascending or descending.  ``dst_coords``: the same two names, target coordinates in any order.
    ``regrid(field)`` takes a ``[T, ny, nx]`` host array (float32 or float64) or ``DeviceArray`` to a ``[T, Ny * Nx]`` float64
    ``DeviceArray``, cells fastest.  The device tables are built on first use."""

    def __init__(self, src_coords, dst_coords, method="linear", ctx=None):
        if method not in METHODS:
            raise NotImplementedError(f"method={method!r}: only 'linear' and 'nearest' are implemented")
        self.method = method
        self.dims = tuple(src_coords)
        if len(self.dims) != 2:
            raise ValueError(f"Regridder: expected exactly two source dims, got {list(self.dims)}")
        if set(dst_coords) != set(self.dims):
            raise ValueError(f"Regridder: target coords {sorted(dst_coords)} do not name the source dims {sorted(self.dims)}")
        self.src_coords = {d: _coordinate("source", d, src_coords[d]) for d in self.dims}
        self.dst_coords = {d: _coordinate("target", d, dst_coords[d]) for d in self.dims}
        for d, x in self.src_coords.items():
            if len(x) < 2:
                raise ValueError(f"source dimension {d!r} has length {len(x)}: at least 2 nodes are needed to interpolate")
            steps = np.diff(x)
            if not ((steps > 0).all() or (steps < 0).all()):
                raise ValueError(f"source coordinate {d!r} is not strictly monotonic (it is non-monotonic or has duplicates)")
        self._ctx = ctx
        self._state = None

    @property
    def shape_in(self):
        return tuple(len(self.src_coords[d]) for d in self.dims)

    @property
    def shape_out(self):
        return tuple(len(self.dst_coords[d]) for d in self.dims)

    @property
    def ctx(self):
        if self._ctx is None:
            from .engine import default_context

            self._ctx = default_context()
        return self._ctx

    @property
    def state(self):
        if self._state is None:
            y, x = self.dims
            self._state = self.ctx.regrid_create(self.src_coords[y], self.src_coords[x], self.dst_coords[y], self.dst_coords[x], self.method)
        return self._state

    def regrid(self, field, out=None):
        return self.state.apply(field, out=out)

    __call__ = regrid

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None


def interp_dims(array, target_names):
    """the two dims of ``array`` to interpolate over: those it shares by name with the target, in the order of ``array``"""
    dims = tuple(d for d in array.dims if d in target_names and d not in PASS_THROUGH_DIMS)
    if len(dims) != 2:
        raise ValueError(f"interpolation needs exactly two shared spatial dims, found {list(dims)} between {array.dims} and "
                         f"{tuple(target_names)}")
    missing = [d for d in dims if d not in array.coords]
    if missing:
        raise ValueError(f"the array has no coordinate for dim {missing[0]!r}")
    return dims


class InterpolatedGridArray(DeferredGridArray):
    """A coarse ``GridArray`` seen on a finer grid: same dims, the two interpolated dims at the target's sizes and coordinates."""

    _kind = "interp"

    def __init__(self, source, target_coords, method="linear", ctx=None, chunksizes=None):
        self._source = source
        self._spatial = tuple(d for d in source.dims if d in target_coords)
        self._method = method
        self._ctx = ctx
        # validates the coordinates now; one plan for the whole grid (a chunked array builds one per block instead)
        self._regridder = Regridder({d: source.coords[d] for d in self._spatial}, {d: target_coords[d] for d in self._spatial}, method, ctx)
        self.dims = tuple(source.dims)
        self.coords = dict(source.coords)
        self.coords.update({d: np.asarray(target_coords[d]) for d in self._spatial})
        self.name = source.name
        self.chunksizes = chunksizes

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        s = dict(self._source.sizes)
        s.update({d: len(self.coords[d]) for d in self._spatial})
        return s

    @property
    def source(self):
        return self._source

    def _target(self):
        return {d: self.coords[d] for d in self._spatial}

    def chunk(self, chunks):
        return InterpolatedGridArray(self._source, self._target(), self._method, self._ctx, chunk_lengths(self.sizes, chunks))

    def unchunked(self):
        return self if self.chunksizes is None else InterpolatedGridArray(self._source, self._target(), self._method, self._ctx)

    def isel(self, **indexers):
        """slices along the interpolated dims select target coordinates, along any other dim they select from the coarse data"""
        target = {d: self.coords[d][indexers[d]] if d in indexers else self.coords[d] for d in self._spatial}
        source = self._source.isel(**{d: s for d, s in indexers.items() if d not in self._spatial})
        return InterpolatedGridArray(source, target, self._method, self._ctx)

    # ---- the fine field ----
    def _lead_dims(self):
        return tuple(d for d in self.dims if d not in self._spatial)

    def _coarse_stack(self):
        """the coarse data as [T', ny, nx]: the other dims flattened in front, the interpolated ones in the order of the field"""
        v = _lib.as_field(self._source.transpose(*self._lead_dims(), *self._spatial).values)
        return v.reshape((-1,) + v.shape[-2:])

    def _blocks(self):
        """(selection, unchunked block) of a chunked array, each with a plan of its own from the block's target coordinates"""
        return [(sel, self.isel(**sel)) for sel in _block_slices(self._spatial, self.chunksizes)]

    def device_field(self, ctx=None):
        """the fine field as a [T, C] float64 DeviceArray (C = cells of the two interpolated dims, the second fastest) without touching
        the host; the array must be [time, y, x] (or [y, x]: T = 1)"""
        if self._lead_dims() not in ((), self.dims[:1]):
            raise ValueError(f"device_field needs dims (time, y, x); this array has {self.dims}")
        if self.chunksizes is not None and any(len(self.chunksizes[d]) > 1 for d in self._spatial):
            raise ValueError("device_field of a chunked array: take it per block (isel)")
        return self._regridder_on(ctx).regrid(self._coarse_stack())

    def _regridder_on(self, ctx):
        """the regridder, with its tables on ``ctx`` if one is named (they live on the context that runs the model)"""
        rg = self._regridder
        if ctx is not None and rg._ctx is not ctx:
            rg = self._regridder = Regridder(rg.src_coords, rg.dst_coords, self._method, ctx)
        return rg

    def _block_producer(self, ctx, dim):
        """the fine field as [steps of ``dim``, C], regridded in HBM block of rows by block of rows: for an array with dims
        (dim, y, x) that is not chunked in space"""
        if (len(self.dims) != 3 or self.dims[0] != dim or self._lead_dims() != self.dims[:1]
                or (self.chunksizes is not None and any(len(self.chunksizes[d]) > 1 for d in self.dims[1:]))):
            return None
        rg, stack = self._regridder_on(ctx), self._coarse_stack()
        return RowProducer(len(stack), int(np.prod(rg.shape_out, dtype=np.int64)), np.dtype(np.float64),
                           lambda r0, r1, out: rg.regrid(stack[r0:r1], out=out), False)

    def _compute_values(self):
        order = self._lead_dims() + self._spatial
        stack = self._coarse_stack()
        if self.chunksizes is None:
            return self._in_dims(self._regridder.regrid(stack).to_host(), order)
        fine = np.empty(tuple(self.sizes[d] for d in order))
        for sel, block in self._blocks():
            rg = block._regridder
            fine[(Ellipsis,) + tuple(sel[d] for d in self._spatial)] = rg.regrid(stack).to_host().reshape(fine.shape[:-2] + rg.shape_out)
            rg.close()
        return self._in_dims(fine, order)

    def __repr__(self):
        return f"<InterpolatedGridArray {self.sizes} from {self._source.sizes} method={self._method!r} computed={self.computed}>"
