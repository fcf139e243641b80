"""Grouping of the time axis on the GPU: the climatology of every BCSD recipe and the anomalies taken against it (the reference's
``df.groupby(MONTH_GROUPER).mean()`` and ``_remove_climatology`` per cell, ``da.groupby('time.month').mean()`` and ``gb - clim`` of
the workflow around it).

``group_labels`` makes one label per step -- it is the only place that asks pandas --, ``GridGroupBy`` is what ``GridArray.groupby``
returns, ``GroupReducedGridArray`` is what its ``mean()`` / ``sum()`` return and ``GroupAppliedGridArray`` what ``gb - other``,
``gb + other``, ``gb * other`` and ``gb / other`` return: the source and the group ids, computed when the field is asked for -- on the
host through ``values``, or as a ``DeviceArray`` through ``device_field``.  The source is walked in blocks of time steps: a block of
``coarse.interp_like(obs)`` is regridded into device scratch, a block of a host array is uploaded into it (float32 as float32), and a
``ResampledGridArray`` is reduced in HBM by its own ``device_field`` (a lazy ``RolledGridArray`` likewise); none of them crosses PCIe as a
fine float64 field.

Groups recur -- every year has a January --, so the reduction carries its sums from block to block; the samples of a (group, cell)
are added in time order whatever the blocks, so the result does not depend on where they are cut.

The rule is pandas' ``DataFrame.groupby(key).mean()`` / ``.sum()`` per cell: NaN samples are skipped; a group without a non-NaN
sample gives NaN for ``mean`` and 0.0 for ``sum`` (pandas' ``min_count=0``).  The result is float64 whatever the source.  ``std`` /
``var`` are out of scope: they need a second pass over a lazily produced source.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .core import DeferredGridArray, GridArray, chunk_lengths
from .resample import DEFAULT_SCRATCH_BYTES
from .timesource import _halo_blocks, _time_blocks, takes_whole, walk  # noqa: F401 -- the cutters stay importable from where they lived

OPS = ("mean", "sum")
APPLY_OPS = {"sub": "-", "add": "+", "mul": "*", "div": "/"}
SEASONS = np.array(["DJF", "MAM", "JJA", "SON"])
# what pandas' / xarray's groupby offers beyond the two reductions the engine has: asked for by name, refused by name
_OTHER_REDUCTIONS = ("max", "min", "median", "std", "var", "sem", "prod", "first", "last", "count", "size", "nunique", "ohlc", "quantile",
                     "agg", "aggregate", "apply", "transform", "map", "reduce", "all", "any", "cumsum", "cumprod", "idxmax", "idxmin",
                     "describe", "rank", "shift", "fillna", "where", "assign_coords")


def group_labels(coord, field):
    """one label per step of a time coordinate: ``field`` is ``season``, any per-step attribute of its ``DatetimeIndex`` (``month``,
    ``dayofyear``, ``year`` ...), or a callable applied to every timestamp"""
    index = coord if isinstance(coord, pd.Index) else pd.Index(np.asarray(coord))
    if callable(field):
        return np.asarray([field(x) for x in index])
    if not isinstance(index, pd.DatetimeIndex):
        raise ValueError(f"group field {field!r} needs a datetime coordinate, this one is {index.dtype}")
    if field == "season":
        return SEASONS[(np.asarray(index.month) % 12) // 3]
    labels = getattr(index, field, None) if isinstance(field, str) and not field.startswith("_") else None
    if labels is None or callable(labels) or np.ndim(labels) != 1 or len(labels) != len(index):
        raise ValueError(f"unknown group field {field!r}: expected 'season' or a per-step attribute of pandas' DatetimeIndex such as 'month', "
                         f"'dayofyear', 'year', 'day', 'hour', 'quarter', 'dayofweek'")
    return np.asarray(labels)


class GridGroupBy:
    """``GridArray.groupby(...)``: the labels are made, nothing is computed yet.  ``mean()`` / ``sum()`` -> ``GroupReducedGridArray``;
    ``gb - other``, ``gb + other``, ``gb * other``, ``gb / other`` -> ``GroupAppliedGridArray``."""

    def __init__(self, source, group=None, named=None, name="group", scratch_bytes=DEFAULT_SCRATCH_BYTES):
        named = dict(named or {})
        if (group is None) == (len(named) != 1) or len(named) > 1:
            raise ValueError(f"groupby needs either '<dim>.<field>' or exactly one dim=labels / dim=callable, got group={group!r} and "
                             f"{sorted(named)} (dims of this array: {source.dims})")
        if group is not None:
            if not isinstance(group, str) or group.count(".") != 1:
                raise ValueError(f"group={group!r}: expected '<dim>.<field>', e.g. 'time.month'")
            dim, key = group.split(".")
            gdim = key
        else:
            (dim, key), = named.items()
            gdim = name
        if dim not in source.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {source.dims}")
        T = source.sizes[dim]
        if isinstance(key, str) or callable(key):
            if dim not in source.coords:
                raise ValueError(f"the array has no coordinate for dim {dim!r}")
            per_step = group_labels(source.coords[dim], key)
        else:
            per_step = np.asarray(key)
        if per_step.ndim != 1 or len(per_step) != T:
            raise ValueError(f"labels of shape {per_step.shape}: expected one label for each of the {T} steps of dim {dim!r}")
        if T == 0:
            raise ValueError(f"nothing to group: dim {dim!r} has length 0")
        if pd.isna(per_step).any():
            raise ValueError(f"label {int(np.flatnonzero(pd.isna(per_step))[0])} of dim {dim!r} is NaN / NaT: every step needs a group")
        if gdim in source.dims and gdim != dim:
            raise ValueError(f"the group dim {gdim!r} is already a dim of this array {source.dims}")
        self._source, self._dim, self._gdim, self._scratch_bytes = source, dim, gdim, int(scratch_bytes)
        self.labels, ids = np.unique(per_step, return_inverse=True)
        self.group = ids.astype(np.int32)

    @property
    def dim(self):
        return self._dim

    @property
    def group_dim(self):
        return self._gdim

    def _reduce(self, op):
        return GroupReducedGridArray(self._source, self._dim, self._gdim, self.labels, self.group, op, scratch_bytes=self._scratch_bytes)

    def mean(self):
        return self._reduce("mean")

    def sum(self):
        return self._reduce("sum")

    def _apply(self, other, op):
        if not isinstance(other, (GridArray, np.ndarray)):
            return NotImplemented
        return GroupAppliedGridArray(self, other, op)

    def __sub__(self, other):
        return self._apply(other, "sub")

    def __add__(self, other):
        return self._apply(other, "add")

    def __mul__(self, other):
        return self._apply(other, "mul")

    def __truediv__(self, other):
        return self._apply(other, "div")

    def __getattr__(self, name):
        if name in _OTHER_REDUCTIONS:
            def refuse(*args, **kwargs):
                raise NotImplementedError(f"groupby(...).{name}(): only mean() and sum() are implemented")

            return refuse
        raise AttributeError(name)

    def __repr__(self):
        return f"<GridGroupBy {self._dim} -> {self._gdim}: {len(self.labels)} groups of {self._source.sizes[self._dim]} steps>"


class GroupReducedGridArray(DeferredGridArray):
    """A ``GridArray`` whose ``dim`` is reduced over groups of its steps: the dims of the source with ``dim`` replaced in place by the
    group dim, whose coordinate is the sorted labels."""

    _kind = "group_reduced"

    def __init__(self, source, dim, gdim, labels, group, op="mean", ctx=None, scratch_bytes=DEFAULT_SCRATCH_BYTES, chunksizes=None):
        if op not in OPS:
            raise NotImplementedError(f"groupby reduction {op!r}: only mean and sum are implemented")
        self._source, self._dim, self._gdim, self._labels, self._group, self._op = source, dim, gdim, labels, group, op
        self._ctx, self._scratch_bytes = ctx, int(scratch_bytes)
        self.dims = tuple(gdim if d == dim else d for d in source.dims)
        self.coords = {k: v for k, v in source.coords.items() if k != dim}
        self.coords[gdim] = labels
        self.name = source.name
        self.chunksizes = chunksizes

    def _like(self, source=None, chunksizes=None):
        return GroupReducedGridArray(self._source if source is None else source, self._dim, self._gdim, self._labels, self._group, self._op,
                                     self._ctx, self._scratch_bytes, chunksizes)

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        return {(self._gdim if d == self._dim else d): (len(self._labels) if d == self._dim else n) for d, n in self._source.sizes.items()}

    @property
    def source(self):
        return self._source

    @property
    def group(self):
        return self._group

    @property
    def group_dim(self):
        return self._gdim

    def chunk(self, chunks):
        return self._like(chunksizes=chunk_lengths(self.sizes, chunks))

    def unchunked(self):
        return self if self.chunksizes is None else self._like()

    def isel(self, **indexers):
        """slices along the other dims select from the source (the result stays lazy); a selection along the group dim is made on the
        computed field"""
        if self._gdim in indexers:
            return self.compute().isel(**indexers)
        return self._like(source=self._source.isel(**indexers))

    # ---- the reduced field ----
    def _rest_dims(self):
        return tuple(d for d in self.dims if d != self._gdim)

    def _row_dim(self):
        return self._gdim

    def _field_order(self):
        return (self._gdim,) + self._rest_dims()

    def device_field(self, ctx=None):
        """the reduced field as a [G, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest).  The time
        axis is walked in blocks of at most ``scratch_bytes``; the sums of a group are carried from block to block and every cell's
        samples are added in time order: the result does not depend on the block size."""
        ctx = self._context(ctx)
        G, T = len(self._labels), self._source.sizes[self._dim]
        out = acc = None
        try:
            with walk(self._source, self._dim, ctx, self._scratch_bytes, "groupby") as w:
                for r0, r1, block, _ in w:
                    out, acc = ctx.groupby_reduce(block, self._group[r0:r1], G, self._op, acc=acc, finish=r1 == T)
        finally:
            for a in acc or ():
                a.free()
        return out

    def __repr__(self):
        return (f"<GroupReducedGridArray {self.sizes} {self._op} over {self._dim} -> {self._gdim} of {self._source.sizes} "
                f"computed={self.computed}>")


class GroupAppliedGridArray(DeferredGridArray):
    """``gb (op) other``: every step of the source combined with the row of ``other`` that carries its label; dims, coords and sizes
    are the source's."""

    _kind = "group_applied"

    def __init__(self, gb, other, op, ctx=None):
        if op not in APPLY_OPS:
            raise NotImplementedError(f"groupby arithmetic {op!r}: only {sorted(APPLY_OPS)} are implemented")
        src, dim, gdim = gb._source, gb._dim, gb._gdim
        rest = tuple(d for d in src.dims if d != dim)
        want = tuple(src.sizes[d] for d in rest)
        self._source, self._dim, self._gdim, self._rest, self._op = src, dim, gdim, rest, op
        self._ctx, self._scratch_bytes = ctx, gb._scratch_bytes
        if isinstance(other, GridArray):
            if set(other.dims) != {gdim, *rest} or len(other.dims) != len(rest) + 1:
                raise ValueError(f"other has dims {other.dims}; expected the group dim {gdim!r} and {rest}")
            if any(other.sizes[d] != src.sizes[d] for d in rest):
                raise ValueError(f"other has sizes {other.sizes}; expected { {d: src.sizes[d] for d in rest} } beside {gdim!r}")
            if gdim not in other.coords or len(other.coords[gdim]) != other.sizes[gdim]:
                raise ValueError(f"other has no coordinate for the group dim {gdim!r}: its rows cannot be matched by label")
            theirs = np.asarray(other.coords[gdim])
            row = {label: i for i, label in enumerate(theirs.tolist())}
            missing = [label for label in gb.labels.tolist() if label not in row]
            if missing:
                raise ValueError(f"other has no {gdim}={missing[0]!r}: its {gdim!r} coordinate must hold every label present in the source "
                                 f"(missing {missing})")
            self._group = np.asarray([row[label] for label in gb.labels.tolist()], dtype=np.int32)[gb.group]  # rows of other, by label
            self._other = other
        else:
            table = np.asarray(other, dtype=np.float64)
            if table.shape != (len(gb.labels),) + want:
                raise ValueError(f"other has shape {table.shape}; expected {(len(gb.labels),) + want}: one field per sorted label")
            self._group = gb.group
            self._other = GridArray(table, (gdim,) + rest)
        self.dims = tuple(src.dims)
        self.coords = dict(src.coords)
        self.name = src.name

    @property
    def sizes(self):
        return dict(self._source.sizes)

    @property
    def source(self):
        return self._source

    @property
    def group(self):
        return self._group

    def _row_dim(self):
        return self._dim

    def _field_order(self):
        return (self._dim,) + self._rest

    def _table(self, ctx):
        """other as a [G', C] float64 DeviceArray in this array's cell order: a lazy reduction or a lazy grouped quantile in that order,
        or a lazy rolling statistic of one, is computed in HBM, any other array goes up once"""
        order = (self._gdim,) + self._rest
        o = self._other
        if takes_whole(o, "table", self._gdim) and tuple(o.dims) == order:
            return o.device_field(ctx)
        v = np.ascontiguousarray((o if tuple(o.dims) == order else o.transpose(*order)).values, dtype=np.float64)
        return ctx.to_device(v.reshape(v.shape[0], -1))

    def device_field(self, ctx=None):
        """the field as a [T, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest): the source is
        walked in blocks of time steps as for the reduction; the table is uploaded (or computed) once"""
        ctx = self._context(ctx)
        table = self._table(ctx)
        try:
            with walk(self._source, self._dim, ctx, self._scratch_bytes, "groupby") as w:
                out = w.result((self._source.sizes[self._dim], w.cells))
                for r0, r1, block, _ in w:
                    ctx.groupby_apply(block, self._group[r0:r1], table, self._op, out=out.rows(r0, r1))
        finally:
            table.free()
        return out

    def __repr__(self):
        return f"<GroupAppliedGridArray {self.sizes} {self._dim} {APPLY_OPS[self._op]} {self._gdim} computed={self.computed}>"
