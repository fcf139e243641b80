"""Localized analogs on the GPU (LOCA, Pierce et al. 2014): one real library day per location instead of one blend per day.

A blend of 30 days (``ConstructedAnalogs``) smooths extremes and makes drizzle.  Here the k regional analogs of a target day are found as
there (``ca_select``: the same candidates, distance and order), then every coarse cell keeps the one analog whose pattern matches the
target best within ``radius`` coarse cells around it (``ca_local``), and the fine field copies, fine cell by fine cell, the fine library
of the day chosen for the coarse cell it lies in -- as it is, shifted by the coarse difference (temperature) or scaled by the coarse
ratio (precipitation).  ``LocalizedAnalogs`` holds the two libraries (``fit``) and makes the choices of a coarse target (``predict``);
these touch coarse data only and run at once.  What ``predict`` returns, a ``LocalizedGridArray``, is lazy exactly as a
``ConstructedGridArray`` is: whole through ``device_field`` (``compare``, ``quantile``, ``where``), or block of target days by block with
the fine library resident (``resample``, ``groupby``, ``rolling``).

The rule is stated in include/sd_downscale.h and restated by tests/_localized_oracle.py.  Out of scope: LOCA's smoothing across the
boundaries between different analog days, its multivariate and bias-correction steps, curvilinear grids (the coordinates are 1-D),
cftime calendars, more than 32 analogs, coarse grids of more than 4 096 cells and the sharded path.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .constructed import PERIOD, ConstructedAnalogs
from .core import DeferredGridArray
from .remap import cell_bounds
from .timesource import RowProducer, host_rows

ADJUSTS = tuple(_lib.CA_ADJUST)


def coarse_index(coarse_coord, fine_coord, name="coordinate"):
    """for every fine centre the index of the coarse cell whose bounds (``remap.cell_bounds`` of the coarse centres) contain it: the
    lower bound of a cell is inclusive, so is the upper bound of the outermost cell; -1 outside the hull.  Either coordinate may descend."""
    bounds = cell_bounds(coarse_coord, f"the coarse coordinate {name!r}")
    x = np.asarray(fine_coord)
    if x.ndim != 1 or not (np.issubdtype(x.dtype, np.number) and not np.issubdtype(x.dtype, np.complexfloating)):
        raise ValueError(f"the fine coordinate {name!r} must be one-dimensional and numeric, got shape {x.shape} of {x.dtype}")
    x = x.astype(np.float64)
    n = len(bounds) - 1
    descending = bounds[0] > bounds[-1]
    asc = bounds[::-1] if descending else bounds
    m = np.searchsorted(asc, x, side="right") - 1
    m[x == asc[-1]] = n - 1
    m[(m < 0) | (m >= n) | np.isnan(x)] = -1
    if descending:
        m = np.where(m >= 0, n - 1 - m, -1)
    return m.astype(np.int32)


class LocalizedAnalogs(ConstructedAnalogs):
    """``LocalizedAnalogs(n_analogs=30, window=45, radius=1, adjust='shift', max_scale=None, exclude_same_year=False, weights='area',
    latitude='auto')``.

    ``n_analogs``, ``window``, ``exclude_same_year``, ``weights``, ``latitude``: the regional stage, as for ``ConstructedAnalogs``.
    ``radius``: coarse cells around a coarse cell over which the k analogs are compared for it, an int or ``(ry, rx)`` in the order of
    the coarse library's spatial dims; 0 compares the cell alone, a radius that covers the grid chooses the regionally closest day
    everywhere.  ``adjust``: ``'none'`` the fine library of the chosen day as it is; ``'shift'`` plus the coarse target minus the
    coarse library of that day and cell; ``'scale'`` times their ratio (1 where the library is not > 0), at most ``max_scale``
    (``None``: no limit).

    ``fit(coarse_library, fine_library)`` -- two spatial dims of the same names with 1-D coordinates: every fine cell belongs to the
    coarse cell whose bounds contain its centre -- and ``predict(coarse_target)`` -> ``LocalizedGridArray``; ``analog_index_``,
    ``analog_distance_`` [Tq, k], ``status_`` [Tq], ``local_index_`` and ``local_distance_`` [Tq, ny, nx] are those of the last
    ``predict``."""

    def __init__(self, n_analogs=30, window=45, radius=1, adjust="shift", max_scale=None, exclude_same_year=False, weights="area",
                 latitude="auto", dim="time", ctx=None):
        super().__init__(n_analogs=n_analogs, window=window, kind="mean", ridge=0.0, exclude_same_year=exclude_same_year, weights=weights,
                         latitude=latitude, dim=dim, ctx=ctx)
        del self.kind, self.ridge  # (there is no weights stage)
        try:
            pair = (radius, radius) if np.ndim(radius) == 0 else tuple(radius)
            ok = len(pair) == 2 and all(int(r) == r and r >= 0 for r in pair)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"radius={radius!r}: expected a number of coarse cells >= 0 or a pair (ry, rx) of them")
        self.radius = (int(pair[0]), int(pair[1]))
        if adjust not in ADJUSTS:
            raise ValueError(f"adjust={adjust!r}: expected one of {', '.join(repr(s) for s in ADJUSTS)}")
        self.adjust = adjust
        if max_scale is not None and not float(max_scale) > 0.0:
            raise ValueError(f"max_scale={max_scale!r}: expected None or a limit > 0")
        self.max_scale = None if max_scale is None else float(max_scale)

    def fit(self, coarse, fine):
        self._coarse = None
        super().fit(coarse, fine)
        made, self._coarse = self._coarse, None  # (fitted only once the grids are matched)
        spatial = made["dims"]
        if len(spatial) != 2:
            raise ValueError(f"the coarse library needs exactly two spatial dims beside {self.dim!r}, got {spatial}")
        fine_spatial = tuple(d for d in fine.dims if d != self.dim)
        if set(fine_spatial) != set(spatial) or len(fine_spatial) != 2:
            raise ValueError(f"the fine library has spatial dims {fine_spatial}; expected {spatial} in any order")
        axis = {}
        for d in spatial:
            for name, a in (("coarse", coarse), ("fine", fine)):
                if d not in a.coords:
                    raise ValueError(f"the {name} library has no coordinate for dim {d!r}")
            axis[d] = coarse_index(coarse.coords[d], fine.coords[d], d).astype(np.int64)
        nx = made["sizes"][spatial[1]]
        i = axis[spatial[0]].reshape([-1 if d == spatial[0] else 1 for d in fine_spatial])
        j = axis[spatial[1]].reshape([-1 if d == spatial[1] else 1 for d in fine_spatial])
        self._cell_of = np.ascontiguousarray(np.where((i >= 0) & (j >= 0), i * nx + j, -1), dtype=np.int32)  # in the fine dims' order
        self._coarse = made
        return self

    def predict(self, target, ctx=None):
        tq, Q, key_l, key_q, excl_l, excl_q = self._coarse_target(target)
        spatial, k = self._coarse["dims"], self.n_analogs
        ny, nx = (self._coarse["sizes"][d] for d in spatial)
        if ctx is None:
            from .engine import default_context

            ctx = self._ctx or default_context()
        made = []
        try:
            made.append(ctx.to_device(self._L))
            made.append(ctx.to_device(Q))
            Ld, Qd = made
            made.extend(ctx.ca_select(Ld, Qd, self._wc, k, key_l, key_q, PERIOD, -1 if self.window is None else self.window, excl_l, excl_q))
            made.extend(ctx.ca_local(Ld, Qd, self._wc, (ny, nx), self.radius, made[2]))
            idx, dist, status, lidx, ldist = (a.to_host() for a in made[2:])
        finally:
            for a in made:
                a.free()
        self.analog_index_, self.analog_distance_, self.status_ = idx, dist, status
        self.local_index_, self.local_distance_ = lidx.reshape(-1, ny, nx), ldist.reshape(-1, ny, nx)
        self._few_candidates(status, tq)
        return LocalizedGridArray(self._fine, self.dim, tq, lidx, self._cell_of, self._L, Q, self.adjust, self.max_scale, ctx=ctx,
                                  name=target.name)


class LocalizedGridArray(DeferredGridArray):
    """The fine field of a localized-analog prediction, [target days, *fine cells]: ``out[q, f] = fine[local_idx[q, cell_of[f]], f]``,
    adjusted to the coarse target.  It keeps the fine library, the [Tq, Cc] table of chosen days, ``cell_of`` in the shape of the fine
    grid and the two coarse fields; a target day without analogs (a non-finite target pattern) is a NaN row, a fine cell outside the
    coarse grid a NaN cell."""

    _kind = "localized"

    def __init__(self, fine, dim, time, local_idx, cell_of, L, Q, adjust="none", max_scale=None, ctx=None, name=None):
        self._fine, self._dim = fine, dim
        self._lidx = np.ascontiguousarray(local_idx, dtype=np.int32)
        self._cell_of = np.asarray(cell_of, dtype=np.int32)
        self._L, self._Q, self._adjust, self._max_scale = L, Q, adjust, max_scale
        self._ctx = ctx
        self._spatial = tuple(d for d in fine.dims if d != dim)
        self.dims = (dim,) + self._spatial
        self.coords = {k: v for k, v in fine.coords.items() if k != dim}
        self.coords[dim] = time
        self.name = name if name is not None else fine.name

    @property
    def sizes(self):
        s = {self._dim: len(self._lidx)}
        s.update({d: self._fine.sizes[d] for d in self._spatial})
        return s

    @property
    def local_index(self):
        return self._lidx

    @property
    def cell_of(self):
        return self._cell_of

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices stay lazy: along the spatial dims they select cells of the fine library and of ``cell_of``, along the time dim rows of
        the table of chosen days and of the coarse target"""
        unknown = [d for d in indexers if d not in self.dims]
        if unknown:
            raise ValueError(f"dim {unknown[0]!r} is not a dim of this array {self.dims}")
        if not all(isinstance(s, slice) for s in indexers.values()):
            return self.compute().isel(**indexers)
        rows = indexers.get(self._dim, slice(None))
        fine = self._fine.isel(**{d: s for d, s in indexers.items() if d != self._dim})
        cell_of = self._cell_of[tuple(indexers.get(d, slice(None)) for d in self._spatial)]
        return LocalizedGridArray(fine, self._dim, self.coords[self._dim][rows], self._lidx[rows], cell_of, self._L, self._Q[rows], self._adjust,
                                  self._max_scale, self._ctx, self.name)

    # ---- the fine field ----
    def _row_dim(self):
        return self._dim

    def _field_order(self):
        return self.dims

    def _library(self, ctx):
        """what an apply call reads, resident: the fine library as a [Tl, Cf] DeviceArray (float32 as float32), ``cell_of``, the table of
        chosen days and, unless adjust is 'none', the coarse library and target -> (arrays, keywords of ``ca_local_apply``)"""
        rows = host_rows(self._fine, self._dim)
        if min(rows.shape) < 1 or len(self._lidx) < 1:
            raise ValueError(f"nothing to construct: the array has sizes {self.sizes}")
        made = []
        try:
            made.append(ctx.to_device(rows, rows.dtype))
            made.append(ctx.to_device(np.ascontiguousarray(self._cell_of.reshape(-1)), np.int32))
            made.append(ctx.to_device(self._lidx, np.int32))
            if self._adjust != "none":
                made.append(ctx.to_device(self._L))
                made.append(ctx.to_device(np.ascontiguousarray(self._Q)))
        except BaseException:
            for a in made:
                a.free()
            raise
        return made

    def _apply(self, ctx, made, **rows):
        return ctx.ca_local_apply(*made, adjust=self._adjust, max_scale=0.0 if self._max_scale is None else self._max_scale, **rows)

    def device_field(self, ctx=None):
        """the whole fine field as a [Tq, Cf] float64 DeviceArray (the cells of the fine dims in their order, the last fastest)"""
        ctx = self._context(ctx)
        made = self._library(ctx)
        try:
            return self._apply(ctx, made)
        finally:
            for a in made:
                a.free()

    def _block_producer(self, ctx, dim):
        """rows [r0, r1) of the fine field with the fine library, ``cell_of`` and the coarse fields resident: they go up once, when the
        first block is asked for"""
        if self.computed or dim != self._dim:
            return None
        cells = int(np.prod([self._fine.sizes[d] for d in self._spatial], dtype=np.int64))
        resident = []

        def produce(r0, r1, out):
            if not resident:
                resident.extend(self._library(ctx))
            return self._apply(ctx, resident, q0=r0, q1=r1, out=out)

        return RowProducer(len(self._lidx), cells, np.dtype(np.float64), produce, False)

    def __repr__(self):
        return (f"<LocalizedGridArray {self.sizes} from one of {self._fine.sizes[self._dim]} library days per coarse cell, "
                f"adjust={self._adjust!r} computed={self.computed}>")
