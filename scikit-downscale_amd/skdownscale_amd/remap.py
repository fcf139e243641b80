"""Conservative remapping of fine fields onto a coarse grid on the GPU: the first step of the BCSD of Wood et al. 2004, the
observations aggregated to the GCM's grid (``obs.remap_like(gcm)``), which ``interp_like`` cannot do -- it samples two to four fine
nodes per coarse cell, ignores the rest and does not conserve the field's integral.

``cell_bounds`` infers the bounds of the cells around 1-D centres, ``ConservativeRemapper`` owns the engine's tables for one (source
grid, target grid) and ``RemappedGridArray`` is what ``GridArray.remap_like`` returns: it keeps the fine source and produces the coarse
field when it is asked for -- on the host through ``values``, or as a ``[T, C]`` ``DeviceArray`` through ``device_field``.  A fine host
array goes up block by block (float32 as float32); a lazy time-axis result (``resample`` ...) is taken from HBM.

The rule is first-order area overlap on rectilinear grids, separable like the interpolation: per dimension the overlap lengths of the
cells, with latitudes measured in ``sin(lat)`` for ``weights='area'``; a target cell is the overlap-weighted mean of the non-NaN
source cells it covers, NaN where their weight is less than ``min_valid`` of the covered weight or where it lies outside the source
(include/sd_downscale.h states the order of the sums; csrc/sd_remap_plan.h builds the tables).  Longitudes are plain numbers: a
0..360 source does not wrap onto a -180..180 target.  Curvilinear grids and higher-order methods are out of scope.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeferredGridArray
from .timesource import RowProducer, takes_whole, upload_rows, walk

WEIGHTS = ("area", "plain")
LATITUDE_NAMES = ("lat", "latitude")
DEFAULT_SCRATCH_BYTES = 1 << 30


def cell_bounds(coord, name="coordinate"):
    """The n + 1 bounds of the cells around n >= 2 centres: the midpoints between neighbours, the two ends extrapolated by half the
    end spacing; in the order of the centres, which must be strictly monotonic"""
    c = np.asarray(coord)
    if c.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {c.shape}")
    c = np.ascontiguousarray(c, dtype=np.float64)
    if np.isnan(c).any():
        raise ValueError(f"{name} contains NaN")
    if len(c) < 2:
        raise ValueError(f"{name} has {len(c)} centre(s): at least 2 are needed to infer cell bounds; give explicit bounds")
    steps = np.diff(c)
    if not ((steps > 0).all() or (steps < 0).all()):
        raise ValueError(f"{name} is not strictly monotonic (it is non-monotonic or has duplicates)")
    mid = 0.5 * (c[:-1] + c[1:])
    return np.concatenate([[c[0] - 0.5 * (c[1] - c[0])], mid, [c[-1] + 0.5 * (c[-1] - c[-2])]])


def _explicit_bounds(which, dim, b, n):
    b = np.asarray(b)
    if b.ndim != 1 or len(b) != n + 1:
        raise ValueError(f"{which} bounds of {dim!r}: expected {n + 1} bounds for {n} cells, got shape {b.shape}")
    b = np.ascontiguousarray(b, dtype=np.float64)
    if np.isnan(b).any():
        raise ValueError(f"{which} bounds of {dim!r} contain NaN")
    steps = np.diff(b)
    if not ((steps > 0).all() or (steps < 0).all()):
        raise ValueError(f"{which} bounds of {dim!r} are not strictly monotonic (they are non-monotonic or have duplicates)")
    return b


class ConservativeRemapper:
    """First-order conservative (area-overlap) remapping between two rectilinear grids.

    ``src_coords`` / ``dst_coords``: mappings of the same two dim names to 1-D cell centres, in the order of the field's spatial dims.
    ``weights='area'`` measures the latitude dim in ``sin(lat)`` (degrees, clipped to [-90, 90]) so that the weights are areas on the
    sphere; ``latitude='auto'`` takes the dim named ``lat`` or ``latitude``, a dim name names it, ``None`` says there is none.
    ``weights='plain'`` uses coordinate units on both dims (projected grids).  Cell bounds are inferred from the centres
    (``cell_bounds``) unless given: ``src_bounds`` / ``dst_bounds`` are mappings ``{dim: n + 1 bounds}``; ``bounds={dim: array}`` goes to
    whichever of the two grids its length fits.  ``remap(field, min_valid)`` takes a ``[T, ny, nx]`` host array (float32 or float64) or a
    ``[T, ny * nx]`` ``DeviceArray`` to a ``[T, Ny * Nx]`` float64 ``DeviceArray``.  The device tables are built on first use."""

    def __init__(self, src_coords, dst_coords, weights="area", latitude="auto", bounds=None, ctx=None, src_bounds=None, dst_bounds=None):
        if weights not in WEIGHTS:
            raise NotImplementedError(f"weights={weights!r}: only 'area' and 'plain' are implemented")
        self.weights = weights
        self.dims = tuple(src_coords)
        if len(self.dims) != 2:
            raise ValueError(f"ConservativeRemapper: expected exactly two source dims, got {list(self.dims)}")
        if set(dst_coords) != set(self.dims):
            raise ValueError(f"ConservativeRemapper: target coords {sorted(dst_coords)} do not name the source dims {sorted(self.dims)}")
        if latitude == "auto":
            named = [d for d in self.dims if d in LATITUDE_NAMES]
            latitude = named[0] if named else None
        elif latitude is not None and latitude not in self.dims:
            raise ValueError(f"latitude={latitude!r} is not one of the spatial dims {self.dims}")
        self.latitude = latitude if weights == "area" else None
        given = {"source": dict(src_bounds or {}), "target": dict(dst_bounds or {})}
        sizes = {"source": {d: len(np.atleast_1d(src_coords[d])) for d in self.dims},
                 "target": {d: len(np.atleast_1d(dst_coords[d])) for d in self.dims}}
        for d, b in (bounds or {}).items():
            fits = [w for w in ("source", "target") if d in sizes[w] and np.ndim(b) == 1 and len(b) == sizes[w][d] + 1]
            if not fits:
                raise ValueError(f"bounds of {d!r} with shape {np.shape(b)} fit neither the source nor the target grid "
                                 f"({ {w: s.get(d) for w, s in sizes.items()} } cells)")
            for w in fits:
                given[w].setdefault(d, b)
        for w in given:
            unknown = [d for d in given[w] if d not in self.dims]
            if unknown:
                raise ValueError(f"{w} bounds name {unknown[0]!r}, which is not one of the spatial dims {self.dims}")
        self.shape_in = tuple(sizes["source"][d] for d in self.dims)
        self.shape_out = tuple(sizes["target"][d] for d in self.dims)
        self.bounds = {}  # which -> dim -> the bounds in coordinate units
        for w, coords in (("source", src_coords), ("target", dst_coords)):
            self.bounds[w] = {d: (_explicit_bounds(w, d, given[w][d], sizes[w][d]) if d in given[w]
                                  else cell_bounds(coords[d], f"{w} coordinate {d!r}")) for d in self.dims}
        self._ctx = ctx
        self._state = None

    def measure(self, which, dim):
        """the bounds of ``dim`` in the units whose differences are the weights: sin(lat) for the latitude under 'area'"""
        b = self.bounds[which][dim]
        return np.sin(np.deg2rad(np.clip(b, -90.0, 90.0))) if dim == self.latitude else b

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
            self._state = self.ctx.remap_create(self.measure("source", y), self.measure("source", x), self.measure("target", y),
                                                self.measure("target", x))
        return self._state

    def remap(self, field, min_valid=0.5, out=None, scratch_bytes=None):
        """``scratch_bytes``: a host field larger than this goes up in blocks of whole time steps of at most that many bytes (at least
        one step); every step is remapped on its own, so the result does not depend on the blocks"""
        if scratch_bytes is None or not isinstance(field, np.ndarray):
            return self.state.apply(field, min_valid, out=out)
        cells = int(np.prod(self.shape_in, dtype=np.int64))
        field = _lib.as_field(field)
        if field.ndim not in (2, 3) or field.shape[0] < 1 or field.size != field.shape[0] * cells:
            raise ValueError(f"field: expected a [T, {self.shape_in[0]}, {self.shape_in[1]}] field, got shape {field.shape}")
        field = field.reshape(field.shape[0], cells)
        with walk(upload_rows(field), None, self.ctx, scratch_bytes) as w:
            out = w.result((field.shape[0], int(np.prod(self.shape_out, dtype=np.int64))), out)
            for r0, r1, block, _ in w:
                self.state.apply(block, min_valid, out=out.rows(r0, r1))
        return out

    __call__ = remap

    def on(self, ctx):
        """this remapper, with its tables on ``ctx`` if one is named (they live on the context that runs the call)"""
        if ctx is None or self._ctx is ctx:
            return self
        other = object.__new__(ConservativeRemapper)
        other.__dict__.update(self.__dict__)
        other._ctx, other._state = ctx, None
        return other

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None


class RemappedGridArray(DeferredGridArray):
    """A fine ``GridArray`` seen on a coarser grid: same dims, the two remapped dims at the target's sizes and coordinates."""

    _kind = "remap"

    def __init__(self, source, target_coords, weights="area", latitude="auto", min_valid=0.5, src_bounds=None, dst_bounds=None, ctx=None,
                 scratch_bytes=None):
        self._source = source
        self._spatial = tuple(d for d in source.dims if d in target_coords)
        self._min_valid = float(min_valid)
        if not 0.0 <= self._min_valid <= 1.0:
            raise ValueError(f"min_valid={min_valid!r}: expected a share of the covered area in [0, 1]")
        self._scratch_bytes = DEFAULT_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
        if self._scratch_bytes < 1:
            raise ValueError(f"scratch_bytes={scratch_bytes!r}: expected a positive number of bytes")
        self._ctx = ctx
        self._remapper = ConservativeRemapper({d: source.coords[d] for d in self._spatial}, {d: target_coords[d] for d in self._spatial},
                                              weights, latitude, ctx=ctx, src_bounds=src_bounds, dst_bounds=dst_bounds)
        self.dims = tuple(source.dims)
        self.coords = dict(source.coords)
        self.coords.update({d: np.asarray(target_coords[d]) for d in self._spatial})
        self.name = source.name

    def _like(self, source):
        new = object.__new__(RemappedGridArray)
        new.__dict__.update(self.__dict__)
        new._source, new._full = source, None
        new.coords = dict(source.coords)
        new.coords.update({d: self.coords[d] for d in self._spatial})
        return new

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        s = dict(self._source.sizes)
        s.update({d: len(self.coords[d]) for d in self._spatial})
        return s

    @property
    def source(self):
        return self._source

    @property
    def remapper(self):
        return self._remapper

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices along the other dims select from the source (the result stays lazy); a selection along a remapped dim is made on
        the computed field"""
        if any(d in self._spatial for d in indexers):
            return self.compute().isel(**indexers)
        return self._like(self._source.isel(**indexers))

    # ---- the coarse field ----
    def _lead_dims(self):
        return tuple(d for d in self.dims if d not in self._spatial)

    def _host_source(self):
        """the source is (or has become) a host array: anything but a lazy array that has not been computed"""
        return not isinstance(self._source, DeferredGridArray) or self._source.computed

    def _source_stack(self):
        """the fine data as [T', ny, nx]: the other dims flattened in front, the remapped ones in the order of the field; float32 stays
        float32"""
        src = self._source
        order = self._lead_dims() + self._spatial
        v = _lib.as_field((src if tuple(src.dims) == order else src.transpose(*order)).values)
        return v.reshape((-1,) + v.shape[-2:])

    def _remapper_on(self, ctx):
        self._remapper = self._remapper.on(ctx)
        return self._remapper

    def _row_dim(self):
        """the leading dim where the coarse field is made in HBM from a lazy source's field"""
        return self.dims[0] if len(self.dims) == 3 and not self._host_source() and self._lead_dims() == self.dims[:1] else None

    def _block_producer(self, ctx, dim):
        """the coarse field as [steps of ``dim``, C] from a host source with dims (dim, y, x): a block of fine rows is uploaded and
        remapped into the block"""
        if self.computed or not self._host_source() or len(self.dims) != 3 or self.dims[0] != dim or self._lead_dims() != self.dims[:1]:
            return None
        rm, stack = self._remapper_on(ctx), self._source_stack()
        return RowProducer(len(stack), int(np.prod(rm.shape_out, dtype=np.int64)), np.dtype(np.float64),
                           lambda r0, r1, out: rm.remap(stack[r0:r1], self._min_valid, out=out, scratch_bytes=self._scratch_bytes), False)

    def device_field(self, ctx=None):
        """the coarse field as a [T, C] float64 DeviceArray (C = cells of the two remapped dims, the second fastest); the array must be
        [time, y, x] (or [y, x]: T = 1).  A host source goes up in blocks of at most ``scratch_bytes``; a lazy time-axis result with
        the same dims is computed in HBM and remapped there."""
        if self._lead_dims() not in ((), self.dims[:1]):
            raise ValueError(f"device_field needs dims (time, y, x); this array has {self.dims}")
        ctx = self._context(ctx)
        rm = self._remapper_on(ctx)
        src = self._source
        if len(src.dims) == 3 and tuple(src.dims[1:]) == self._spatial and takes_whole(src, "remap", src.dims[0]):
            with walk(src, src.dims[0], ctx, self._scratch_bytes, "remap") as w:
                for _, _, fine, _ in w:
                    return rm.remap(fine, self._min_valid)
        return rm.remap(self._source_stack(), self._min_valid, scratch_bytes=self._scratch_bytes)

    def _compute_values(self):
        order = self._lead_dims() + self._spatial
        if self._lead_dims() in ((), self.dims[:1]):
            field = self.device_field()
        else:
            field = self._remapper_on(self._context()).remap(self._source_stack(), self._min_valid, scratch_bytes=self._scratch_bytes)
        try:
            return self._in_dims(field.to_host(), order)
        finally:
            field.free()

    def __repr__(self):
        return (f"<RemappedGridArray {self.sizes} from {self._source.sizes} weights={self._remapper.weights!r} "
                f"min_valid={self._min_valid} computed={self.computed}>")
