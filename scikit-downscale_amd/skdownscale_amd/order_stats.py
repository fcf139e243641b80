"""Per-cell order statistics over the time axis on the GPU: ``GridArray.quantile`` / ``GridArray.median`` -- percentile thresholds
for extremes (TX90p, R95p), a per-cell ``thresh`` for the GARD estimators, the median climatology of a skewed variable.

The definition is NumPy's: ``np.nanquantile(x, q, method=...)`` / ``np.nanmedian(x)`` per cell and group (``skipna=False``:
``np.quantile`` / ``np.median``, NaN where the group holds a NaN) for the methods 'linear', 'lower', 'higher', 'nearest' and
'midpoint'; the result equals NumPy's bit for bit for finite samples and is float64 whatever the source.  +-inf samples sort as
ordinary values; what the interpolation then makes of them follows IEEE arithmetic as in NumPy (inf - inf is NaN).

``TimeQuantileGridArray`` is what both return: the source, the quantiles and the group ids, computed when the field is asked for -- on
the host through ``values``, or as a ``DeviceArray`` through ``device_field``.  A quantile needs a cell's whole time axis at once, so
the source is brought into HBM whole as [T, C] -- ``T * C * itemsize`` bytes: a lazy ``resample`` / ``groupby`` / ``rolling`` /
``disaggregate`` / ``remap_like`` result through its own ``device_field`` (float64), an unchunked ``coarse.interp_like(obs)`` regridded
block by block into the rows of one float64 field, a host array uploaded (float32 as float32).  Groups of more than 1 344 steps take
that much device scratch again; groups of more than 19 456 steps are refused.  An allocation that fails is a ``MemoryError``, not a
fallback: ``isel`` along the other dims stays lazy, so a caller can cut the cells.
"""
from __future__ import annotations

import numpy as np

from .core import DeferredGridArray
from .groupby import GridGroupBy
from .resample import DEFAULT_SCRATCH_BYTES
from .timesource import walk

METHODS = ("linear", "lower", "higher", "nearest", "midpoint")
QUANTILE_DIM = "quantile"


def check_quantiles(q):
    """``(q as float64 [Q], scalar?)``; ValueError in NumPy's words for anything outside [0, 1], NaN included"""
    arr = np.asarray(q, dtype=np.float64)
    if arr.ndim > 1 or arr.size < 1:
        raise ValueError(f"q must be one quantile or a non-empty 1-D sequence of them, got shape {arr.shape}")
    if not np.all((arr >= 0.0) & (arr <= 1.0)):
        raise ValueError("Quantiles must be in the range [0, 1]")
    return np.atleast_1d(arr).copy(), arr.ndim == 0


class TimeQuantileGridArray(DeferredGridArray):
    """Quantiles (or the median) of a ``GridArray`` over ``dim``, per cell and, with ``by``, per group of steps.  Dims: the source's
    with ``dim`` dropped (``by=None``) or replaced in place by the group dim, whose coordinate is the sorted labels; an array ``q``
    adds a leading ``"quantile"`` dim whose coordinate is ``q``."""

    _kind = "quantile"

    def __init__(self, source, dim, q=0.5, by=None, method="linear", skipna=True, name="group", ctx=None, scratch_bytes=DEFAULT_SCRATCH_BYTES):
        if method != "median" and method not in METHODS:
            raise ValueError(f"quantile method {method!r}: expected one of {', '.join(repr(m) for m in METHODS)}")
        if dim not in source.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {source.dims}")
        if source.sizes[dim] == 0:
            raise ValueError(f"nothing to sort: dim {dim!r} has length 0")
        self._q, self._scalar = (np.array([0.5]), True) if method == "median" else check_quantiles(q)
        self._source, self._dim, self._method, self._skipna = source, dim, method, bool(skipna)
        self._ctx, self._scratch_bytes, self._by, self._name = ctx, int(scratch_bytes), by, name
        if by is None:
            self._gdim, self._labels, self._group = None, None, None
            base = tuple(d for d in source.dims if d != dim)
        else:
            if isinstance(by, str):
                if by.count(".") != 1 or by.split(".")[0] != dim:
                    raise ValueError(f"by={by!r}: expected '{dim}.<field>', e.g. '{dim}.month', labels or a callable for dim {dim!r}")
                gb = GridGroupBy(source, by)
            else:
                gb = GridGroupBy(source, None, {dim: by}, name)
            self._gdim, self._labels, self._group = gb.group_dim, gb.labels, gb.group
            base = tuple(self._gdim if d == dim else d for d in source.dims)
        if not self._scalar and QUANTILE_DIM in base:
            raise ValueError(f"the dim {QUANTILE_DIM!r} of an array q is already a dim of this array {source.dims}")
        self.dims = base if self._scalar else (QUANTILE_DIM,) + base
        self.coords = {k: v for k, v in source.coords.items() if k != dim}
        if self._gdim is not None:
            self.coords[self._gdim] = self._labels
        if not self._scalar:
            self.coords[QUANTILE_DIM] = self._q.copy()
        self.name = source.name

    def _like(self, source):
        new = object.__new__(TimeQuantileGridArray)
        new.__dict__.update(self.__dict__)
        new._source, new._full = source, None
        new.coords = {k: v for k, v in source.coords.items() if k != self._dim}
        new.coords.update({k: self.coords[k] for k in (self._gdim, QUANTILE_DIM) if k in self.coords})
        return new

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        s = {}
        if not self._scalar:
            s[QUANTILE_DIM] = len(self._q)
        for d, n in self._source.sizes.items():
            if d != self._dim:
                s[d] = n
            elif self._gdim is not None:
                s[self._gdim] = len(self._labels)
        return s

    @property
    def source(self):
        return self._source

    @property
    def q(self):
        return float(self._q[0]) if self._scalar else self._q.copy()

    @property
    def method(self):
        return self._method

    @property
    def group(self):
        return self._group

    @property
    def group_dim(self):
        return self._gdim

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices along the source's other dims select from the source (the result stays lazy); a selection along the group dim or the
        quantile dim is made on the computed field"""
        if any(d in indexers for d in (self._gdim, QUANTILE_DIM) if d is not None):
            return self.compute().isel(**indexers)
        return self._like(self._source.isel(**indexers))

    # ---- the field ----
    def _rest_dims(self):
        return tuple(d for d in self._source.dims if d != self._dim)

    def _row_dim(self):
        """the dim whose steps are the rows of ``device_field`` where that is a [G, C] table other lazy arrays can take from HBM: the
        group dim of a scalar-q (or median) grouped result; else None"""
        return self._gdim if self._scalar else None

    def _field_order(self):
        return (() if self._scalar else (QUANTILE_DIM,)) + (() if self._gdim is None else (self._gdim,)) + self._rest_dims()

    def device_field(self, ctx=None):
        """the result as a [Q * G, C] float64 DeviceArray, row ``q * G + g`` (G = 1 without ``by``; C = cells of the other dims in
        their order, the last fastest): [G, C] for one quantile or the median"""
        ctx = self._context(ctx)
        G = None if self._group is None else len(self._labels)
        with walk(self._source, self._dim, ctx, self._scratch_bytes, "any", whole=True, verb="sort") as w:
            for _, _, field, _ in w:
                return ctx.quantile(field, self._q, self._group, G, self._method, self._skipna)

    def __repr__(self):
        what = "median" if self._method == "median" else f"quantile q={self.q!r} method={self._method!r}"
        return f"<TimeQuantileGridArray {self.sizes} {what} over {self._dim} of {self._source.sizes} computed={self.computed}>"
