"""Grid driver: ``PointWiseDownscaler`` with the reference's surface (core.py:200-448).

The reference loops over cells in Python (core.py:86-96 and 137-141), deep-copying the estimator
and building a pandas DataFrame per cell.  Here BCSD / analog estimators are fitted and applied to
*all cells in one batched launch* of the HIP engine; any other estimator (sklearn Pipelines ...)
takes the reference's per-cell loop unchanged in behaviour.

Inputs may be ``xarray.DataArray`` / ``xarray.Dataset`` (lazy import; xarray is optional) or the
tiny labelled-array stand-in ``GridArray`` (numpy values + dims + coords) used where xarray is
not installed.  Output type follows the input type.
"""
from __future__ import annotations

import copy

import numpy as np
import pandas as pd

from . import _lib
from .arrm import ArrmGridModel, PiecewiseLinearRegression
from .bcsd import BcsdBase, check_supported
from .engine import default_context
from .gard import AnalogGridModel, AnalogRegression, PureAnalog, PureRegression, RegressionGridModel
from .quantile import (CunnaneGridModel, CunnaneTransformer, QmGridModel, QuantileMapper, QuantileMapperGridModel,
                       QuantileMappingReressor, check_extrapolate)
from .grouping import GroupedGridModel, GroupedRegressor
from .zscore import ZScoreGridModel, ZScoreRegressor

DEFAULT_FEATURE_DIM = "variable"


def chunk_lengths(sizes, chunks):
    """dim -> block lengths of an array of these ``sizes`` under ``chunks``: dim -> block length (-1, None or a length past the end:
    one block), like ``xarray.DataArray.chunk``"""
    cs = {}
    for d, n in sizes.items():
        b = chunks.get(d, -1) if chunks else -1
        b = n if b in (-1, None) or b >= n else int(b)
        cs[d] = tuple([b] * (n // b) + ([n % b] if n % b else [])) if n else (0,)
    return cs


class GridArray:
    """Minimal labelled array: ``values`` (ndarray), ``dims`` (tuple of names), ``coords`` (dict)."""

    def __init__(self, values, dims, coords=None, name=None):
        self.values = np.asarray(values)
        self.dims = tuple(dims)
        if self.values.ndim != len(self.dims):
            raise ValueError(f"values has {self.values.ndim} dims but dims={self.dims}")
        self.coords = dict(coords or {})
        self.name = name

    @property
    def shape(self):
        return self.values.shape

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def sizes(self):
        return dict(zip(self.dims, self.values.shape))

    # chunk structure like a dask-backed xarray object: PointWiseDownscaler walks the spatial blocks (core.py:256-262,
    # 300-336: xr.map_blocks); the values themselves stay plain NumPy
    chunksizes = None

    @property
    def chunks(self):
        return None if self.chunksizes is None else tuple(self.chunksizes[d] for d in self.dims)

    def chunk(self, chunks):
        """``chunks``: dim -> block length (or -1 for one block), like ``xarray.DataArray.chunk``"""
        g = GridArray(self.values, self.dims, self.coords, self.name)
        g.chunksizes = chunk_lengths(self.sizes, chunks)
        return g

    def isel(self, **indexers):
        """positional selection by slices along named dims (coords follow)"""
        key = tuple(indexers.get(d, slice(None)) for d in self.dims)
        coords = {}
        for k, v in self.coords.items():
            if k in indexers and np.ndim(v) == 1 and len(v) == self.sizes.get(k, -1):
                coords[k] = v[indexers[k]]
            else:
                coords[k] = v
        return GridArray(self.values[key], self.dims, coords, self.name)

    def transpose(self, *dims):
        if Ellipsis in dims:
            i = dims.index(Ellipsis)
            rest = [d for d in self.dims if d not in dims]
            dims = tuple(dims[:i]) + tuple(rest) + tuple(dims[i + 1:])
        perm = [self.dims.index(d) for d in dims]
        return GridArray(self.values.transpose(perm), dims, self.coords, self.name)

    def interp_like(self, other, method="linear"):
        """Interpolate onto the grid of ``other`` over exactly the two spatial dims both arrays name (``xarray``'s
        ``interp_like`` for 1-D coordinates); ``time`` and ``variable`` pass through, and an ``other`` with a time dim contributes
        only its spatial coordinates.  -> ``InterpolatedGridArray``: the coarse data, interpolated on the GPU when needed."""
        from .regrid import interp_dims

        dims = interp_dims(self, other.dims)
        missing = [d for d in dims if d not in other.coords]
        if missing:
            raise ValueError(f"`other` has no coordinate for dim {missing[0]!r}")
        return self.interp({d: other.coords[d] for d in dims}, method=method)

    def interp(self, coords=None, method="linear", **coords_kw):
        """Interpolate onto new 1-D coordinates of exactly two spatial dims (``da.interp(lat=..., lon=...)``)"""
        from .regrid import InterpolatedGridArray, interp_dims

        target = dict(coords or {}, **coords_kw)
        unknown = [d for d in target if d not in self.dims]
        if unknown:
            raise ValueError(f"dim {unknown[0]!r} is not a dim of this array {self.dims}")
        interp_dims(self, target)
        return InterpolatedGridArray(self, target, method)

    def remap_like(self, other, weights="area", latitude="auto", min_valid=0.5, src_bounds=None, dst_bounds=None, scratch_bytes=None):
        """First-order conservative (area-overlap) remapping onto the coarser grid of ``other`` over exactly the two spatial dims both
        arrays name: the aggregation of fine observations to a GCM's grid (step 1 of BCSD, Wood et al. 2004), where ``interp_like``
        would sample a few nodes and alias.  Every target cell is the overlap-weighted mean of the non-NaN source cells it covers,
        NaN where they carry less than ``min_valid`` of the covered weight (0: any valid sample suffices) or where the cell lies
        outside the source; a partly covered cell is the mean over its covered part.  ``weights='area'`` measures the latitude dim
        (``latitude='auto'``: the one named ``lat`` / ``latitude``; or a dim name, or None) in sin(lat), ``'plain'`` uses coordinate
        units on both dims.  Cell bounds are the midpoints between centres, the ends extrapolated by half a spacing, unless
        ``src_bounds`` / ``dst_bounds`` ``{dim: n + 1 bounds}`` give them.  Longitudes do not wrap.  ``time`` and ``variable`` pass
        through.  ``scratch_bytes``: device scratch of one block of fine time steps (default 1 GiB); float32 goes up as float32.
        -> a lazy ``RemappedGridArray`` (float64)."""
        from .regrid import interp_dims
        from .remap import RemappedGridArray

        dims = interp_dims(self, other.dims)
        missing = [d for d in dims if d not in other.coords]
        if missing:
            raise ValueError(f"`other` has no coordinate for dim {missing[0]!r}")
        return RemappedGridArray(self, {d: other.coords[d] for d in dims}, weights, latitude, min_valid, src_bounds, dst_bounds,
                                 scratch_bytes=scratch_bytes)

    def resample(self, indexer=None, scratch_bytes=None, **kwargs):
        """``resample(time='MS').mean()`` / ``.sum()``: pandas' ``DataFrame.resample(rule, **kw)`` bins of the dim's coordinate, reduced
        per cell on the GPU (``xarray``'s ``da.resample(time=rule)`` for these two reductions).  Exactly one dim is named, as a keyword
        or in ``indexer``; every other keyword (``closed``, ``label``, ``offset``, ``origin``) goes to pandas.  NaN samples are skipped;
        a bin without a non-NaN sample gives NaN for ``mean`` and 0.0 for ``sum`` (pandas' rule; xarray's ``sum`` may differ on empty
        bins).  ``scratch_bytes``: device scratch of one block of whole bins (default 1 GiB; a block is at least one bin).
        -> ``GridResample``, whose ``mean()`` / ``sum()`` give a lazy ``ResampledGridArray`` (float64)."""
        from .resample import DEFAULT_SCRATCH_BYTES, GridResample

        named = dict(indexer or {}, **{k: kwargs.pop(k) for k in list(kwargs) if k in self.dims})
        if len(named) != 1:
            raise ValueError(f"resample needs exactly one dim=rule, got {sorted(named)} (dims of this array: {self.dims})")
        (dim, rule), = named.items()
        return GridResample(self, dim, rule, kwargs, DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def groupby(self, group=None, scratch_bytes=None, name="group", **named):
        """``groupby("time.month").mean()`` / ``.sum()`` and ``gb - clim`` / ``+`` / ``*`` / ``/``: climatologies and anomalies per cell
        on the GPU (``xarray``'s ``da.groupby`` for these; pandas' ``DataFrame.groupby(key).mean()`` / ``.sum()`` per cell).  ``group``:
        ``"<dim>.<field>"`` with ``field`` an attribute of the dim's ``DatetimeIndex`` (``month``, ``dayofyear``, ``year``, ``day``,
        ``hour``, ``quarter``, ``dayofweek`` ...) or ``season`` (``DJF`` / ``JJA`` / ``MAM`` / ``SON``): the group dim is named after the
        field.  Or one ``dim=labels`` (one label per step) / ``dim=callable`` (applied to every timestamp: ``MONTH_GROUPER``): the group
        dim is named ``name``.  The groups are the sorted unique labels present.  NaN samples are skipped; a group without a non-NaN
        sample gives NaN for ``mean`` and 0.0 for ``sum``.  ``scratch_bytes``: device scratch of one block of time steps (default
        1 GiB).  -> ``GridGroupBy``: the labels are made, nothing is computed yet."""
        from .groupby import GridGroupBy
        from .resample import DEFAULT_SCRATCH_BYTES

        return GridGroupBy(self, group, named, name, DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def rolling(self, dim=None, center=False, min_periods=None, wrap=False, scratch_bytes=None, **window):
        """``rolling(time=9, center=True, min_periods=1).mean()`` / ``.sum()`` / ``.var(ddof=1)`` / ``.std(ddof=1)``: pandas' fixed
        integer window per cell on the GPU (``rolling({"time": 9}, ...)`` is the same).  The window of step t is the steps
        ``t - (w - 1) .. t``, or ``t - w // 2 .. t - w // 2 + w - 1`` with ``center``, clipped to the array or, with ``wrap=True``, taken
        around its ends (a circular axis such as the day of the year: pandas on the series padded from its other end).  NaN samples are
        skipped; fewer than ``min_periods`` (default: the window) samples give NaN.  Each window is evaluated directly in time order:
        O(window) work per output, and a result that does not depend on how ``scratch_bytes`` (device scratch of one block of time
        steps, default 1 GiB) cuts the axis.  -> ``GridRolling``: nothing is computed yet."""
        from .resample import DEFAULT_SCRATCH_BYTES
        from .rolling import GridRolling

        named = dict(dim or {}) if dim is None or isinstance(dim, dict) else None
        if named is None:
            raise ValueError(f"rolling needs {{dim: window}} or dim=window, got {dim!r}")
        named.update(window)
        if len(named) != 1:
            raise ValueError(f"rolling needs exactly one dim=window, got {sorted(named)} (dims of this array: {self.dims})")
        (d, w), = named.items()
        return GridRolling(self, d, w, center, min_periods, wrap, DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def quantile(self, q, dim="time", by=None, method="linear", skipna=True, name="group", scratch_bytes=None):
        """``quantile(0.9, "time", by="time.dayofyear")``: NumPy's ``np.nanquantile(x, q, method=...)`` per cell over ``dim`` on the GPU
        (``skipna=False``: ``np.quantile``, NaN where a NaN is among the samples), bit for bit for finite samples; ``method`` 'linear'
        | 'lower' | 'higher' | 'nearest' | 'midpoint'; every ``q`` in [0, 1].  ``by``: None for the whole axis, or what ``groupby``
        takes -- ``"<dim>.<field>"`` (``time.month``, ``time.dayofyear``, ``time.season``: the group dim is named after the field), one
        label per step or a callable (the group dim is named ``name``); the groups are the sorted unique labels present.  A scalar
        ``q`` gives the source's dims with ``dim`` dropped, or replaced in place by the group dim; an array ``q`` adds a leading
        ``"quantile"`` dim (xarray's grouped spelling puts it last: ``transpose`` is there).  The whole [T, C] source is held in HBM
        (``T * C * itemsize`` bytes; groups of more than 1 344 steps take as much scratch again, more than 19 456 are refused).
        -> a lazy ``TimeQuantileGridArray`` (float64)."""
        from .order_stats import TimeQuantileGridArray
        from .resample import DEFAULT_SCRATCH_BYTES

        return TimeQuantileGridArray(self, dim, q, by, method, skipna, name,
                                     scratch_bytes=DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def median(self, dim="time", by=None, skipna=True, name="group", scratch_bytes=None):
        """``np.nanmedian`` per cell over ``dim`` on the GPU (``skipna=False``: ``np.median``), per group with ``by`` as for
        ``quantile``.  -> a lazy ``TimeQuantileGridArray`` (float64)."""
        from .order_stats import TimeQuantileGridArray
        from .resample import DEFAULT_SCRATCH_BYTES

        return TimeQuantileGridArray(self, dim, 0.5, by, "median", skipna, name,
                                     scratch_bytes=DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def where(self, op, threshold, dim="time", by=None, name="group", scratch_bytes=None):
        """``where("<", 1.0).resample(time="YS").longest_spell()``: threshold and spell indices per period and cell on the GPU (frost
        days, R1mm, CDD / CWD, WSDI, TX90p).  ``op``: '>' | '>=' | '<' | '<='.  ``threshold``: a number (``by`` must be None); an array
        or ``GridArray`` over the other dims, one value per cell (``by`` None); or, with ``by`` as for ``quantile`` -- ``"<dim>.<field>"``,
        one label per step or a callable (the group dim is then named ``name``) --, a ``[G, *rest]`` array with one field per sorted
        label or a ``GridArray`` carrying the group dim, its rows matched by label as ``gb - other`` matches them (a lazy grouped mean,
        scalar-``q`` quantile or ``rolling`` of one stays in HBM).  A step is valid when neither the sample nor its threshold is NaN
        and a hit when it is valid and ``sample op threshold`` holds as doubles (a float32 sample is widened first: NumPy 2 compares
        with a Python float in float32, so ``np.float32(0.1) > 0.1`` is False there and True here); an invalid step ends a spell.
        -> ``GridCondition``: nothing is computed yet.  Its ``resample(time=rule, **pandas_kw)`` cuts the axis into pandas' bins, each
        evaluated by itself (spells do not span bins); without it the whole axis is one bin, the dim is dropped and the whole field is
        held in HBM (``T * C * itemsize`` bytes).  ``valid()``, ``count()``, ``fraction()`` (NaN for a bin without a valid step),
        ``longest_spell()``, ``spell_days(min_length)``, ``spell_count(min_length)`` give a lazy ``SpellGridArray`` (float64, exact);
        ``indices(names, min_length=1)`` several of them behind a leading ``"index"`` dim from one pass over the field.
        ``scratch_bytes``: device scratch of one block of whole bins (default 1 GiB; a block is at least one bin)."""
        from .resample import DEFAULT_SCRATCH_BYTES
        from .spells import GridCondition

        return GridCondition(self, op, threshold, dim, by, name, DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def compare(self, other, dim="time", scratch_bytes=None):
        """``compare(obs).resample(time="YS").rmse()``: paired skill statistics per period and cell on the GPU, both fields walked in
        lock-step.  ``other``: a ``GridArray`` of any kind, lazy ones included, with the same dims (in any order) and the same size on
        every dim; where both arrays carry a coordinate for ``dim`` the two must be equal.  Nothing is aligned or broadcast: anything
        else is a ``ValueError``.  A step is a valid pair when neither sample is NaN (float32 samples are widened first); every sum
        runs over the valid pairs of a bin in time order.  -> ``GridComparison``: nothing is computed yet.  Its
        ``resample(time=rule, **pandas_kw)`` cuts the axis into pandas' bins; without it the whole axis is one bin, the dim is dropped
        and both whole fields are held in HBM.  ``count()``, ``bias()`` (mean of a - b), ``ratio()`` (sum a / sum b: precipitation's
        relative bias), ``mae()``, ``rmse()``, ``corr()`` (Pearson, NaN for fewer than two pairs or a constant series) and
        ``std_ratio()`` give a lazy ``SkillGridArray`` (float64; NaN for a bin without a valid pair, ``count`` 0); ``indices(names)``
        several of them behind a leading ``"index"`` dim from one call.  The summation order is fixed: the result does not depend on
        ``scratch_bytes`` (device scratch of one block of whole bins of both fields together, default 1 GiB; at least one bin)."""
        from .resample import DEFAULT_SCRATCH_BYTES
        from .skill import GridComparison

        return GridComparison(self, other, dim, DEFAULT_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)

    def disaggregate(self, daily_obs, kind="shift", stat=None, years=None, seed=0, climatology=None, scratch_bytes=1 << 30, dim="time"):
        """Temporal disaggregation of this monthly array on the GPU (the last step of BCSD, Wood et al. 2004): every month becomes
        daily weather by borrowing the daily pattern of a historical month of ``daily_obs`` -- the same one for every cell -- and
        shifting it (``kind='shift'``: the monthly mean equals this array) or scaling it (``kind='scale'`` with ``stat='mean'`` or
        ``'sum'``: that statistic equals this array; a dry borrowed month spreads the value evenly).  ``years``: ``None`` draws the
        source year of every month with ``np.random.default_rng(seed)`` among the years whose month is complete in ``daily_obs``, an
        int array ``[M]`` names them, ``'same'`` takes each label's own year.  ``climatology``: a ``GridArray`` or ndarray
        ``[12, *spatial]`` selected by calendar month when this array holds anomalies (``return_anoms=True`` outputs): added for the
        shift, multiplied for the scale.  ``scratch_bytes``: device scratch of one block of whole months when the field is
        downloaded.  -> a lazy ``DisaggregatedGridArray`` (float64) whose ``dim`` holds all days of the labelled months."""
        from .disagg import DisaggregatedGridArray

        return DisaggregatedGridArray(self, daily_obs, dim, kind, stat, years, seed, climatology, scratch_bytes=scratch_bytes)

    def __repr__(self):
        return f"<GridArray {self.sizes}>"


class LazyGridArray(GridArray):
    """Result of predict / transform / inverse_transform on a spatially chunked GridArray: like the reference's
    ``xr.map_blocks`` result (core.py:256-262, 300-336) the blocks are computed when they are asked for.  ``iter_blocks()``
    yields ``(selection, GridArray)`` one spatial block at a time -- nothing but the current block is held --, ``values``
    assembles (and keeps) the whole field.  Only the first block is computed up front: it tells dims, dtype and the sizes of
    the non-spatial dims."""

    def __init__(self, thunks, first, spatial_dims, sizes, chunksizes, coords, name=None):
        self._thunks = list(thunks)  # [(selection, callable -> GridArray)]
        self._first = first
        self._full = None
        self.dims = tuple(first.dims)
        all_sizes = dict(first.sizes)
        all_sizes.update({d: int(sizes[d]) for d in spatial_dims})
        self._shape = tuple(all_sizes[d] for d in self.dims)
        self._dtype = first.dtype
        self.coords = dict(coords)
        self.name = name
        self.chunksizes = {d: (tuple(chunksizes[d]) if d in chunksizes else (all_sizes[d],)) for d in self.dims}

    @property
    def shape(self):
        return self._shape

    @property
    def dtype(self):
        return self._dtype

    @property
    def sizes(self):
        return dict(zip(self.dims, self._shape))

    @property
    def computed(self):
        return self._full is not None

    def iter_blocks(self):
        """(selection, GridArray) per spatial block.  Once ``values`` has assembled the field the blocks are views of it:
        nothing is computed a second time."""
        for i, (sel, thunk) in enumerate(self._thunks):
            if self._full is not None:
                idx = tuple(sel.get(d, slice(None)) for d in self.dims)
                coords = {k: (np.asarray(v)[sel[k]] if k in sel else v) for k, v in self.coords.items()}
                yield sel, GridArray(self._full[idx], self.dims, coords, self.name)
            elif i == 0 and self._first is not None:
                yield sel, self._first
            else:
                yield sel, thunk()

    @property
    def values(self):
        if self._full is None:
            with np.errstate(invalid="ignore"):
                full = np.full(self._shape, np.nan, dtype=self._dtype)
            for sel, block in self.iter_blocks():
                full[tuple(sel.get(d, slice(None)) for d in self.dims)] = block.values
            self._full, self._first = full, None
        return self._full

    def compute(self):
        return GridArray(self.values, self.dims, self.coords, self.name).chunk({d: self.chunksizes[d][0] for d in self.dims})

    def chunk(self, chunks):
        return self.compute().chunk(chunks)

    def isel(self, **indexers):
        return self.compute().isel(**indexers)

    def transpose(self, *dims):
        return self.compute().transpose(*dims)

    def __repr__(self):
        return f"<LazyGridArray {self.sizes} blocks={len(self._thunks)} computed={self.computed}>"


class DeferredGridArray(GridArray):
    """A float64 field that is computed when it is asked for, the base of what ``interp_like``, ``resample`` and ``disaggregate``
    return.  A subclass sets ``dims``, ``coords`` and ``name`` and gives ``sizes`` and ``_compute_values()``; ``values`` keeps what that
    returned.  ``isel`` and ``transpose`` work on the computed field unless the subclass can stay lazy.

    What a lazy array says of itself as the *source* of another one (``timesource`` reads it): ``_kind`` names the class, ``_row_dim()``
    and ``_block_producer()`` say how its field comes into HBM without crossing the host."""

    _full = None
    _ctx = None
    _kind = None

    def _row_dim(self):
        """the dim along which ``device_field`` gives the field as [rows of that dim, cells of the other dims in their order]; None
        where it does not"""
        return None

    def _block_producer(self, ctx, dim):
        """a ``timesource.RowProducer`` where the field can be produced in HBM as [rows of ``dim``, cells], rows [r0, r1) at a time;
        else None"""
        return None

    def _field_order(self):
        """the dims of ``device_field``, the trailing ones flattened into its cells"""
        raise NotImplementedError

    def _compute_values(self):
        field = self.device_field()
        try:
            return self._in_dims(field.to_host(), self._field_order())
        finally:
            field.free()

    @property
    def shape(self):
        return tuple(self.sizes[d] for d in self.dims)

    @property
    def dtype(self):
        return np.dtype(np.float64)  # float32 sources are widened on the device

    @property
    def computed(self):
        return self._full is not None

    @property
    def values(self):
        if self._full is None:
            self._full = self._compute_values()
        return self._full

    def compute(self):
        return GridArray(self.values, self.dims, self.coords, self.name)

    def isel(self, **indexers):
        return self.compute().isel(**indexers)

    def transpose(self, *dims):
        return self.compute().transpose(*dims)

    def _context(self, ctx=None):
        """``ctx``, else the context the array was made with, else the process-wide one"""
        return ctx or self._ctx or default_context()

    def _in_dims(self, field, order):
        """a host field whose axes are the dims ``order`` (the trailing ones possibly flattened) as an array of ``self.dims``"""
        return field.reshape(tuple(self.sizes[d] for d in order)).transpose([order.index(d) for d in self.dims])


class GridDataset(dict):
    """Ordered mapping name -> GridArray (stand-in for xarray.Dataset)."""

    @property
    def chunksizes(self):
        first = next(iter(self.values()), None)
        return None if first is None else first.chunksizes

    @property
    def chunks(self):
        return self.chunksizes

    def chunk(self, chunks):
        return GridDataset({k: v.chunk(chunks) for k, v in self.items()})


def _is_xarray(obj):
    mod = type(obj).__module__
    return mod.startswith("xarray")


def _to_grid(obj, feature_dim):
    """-> (GridArray, was_xarray)"""
    if isinstance(obj, GridArray):
        return obj, False
    if isinstance(obj, GridDataset):
        names = list(obj)
        first = obj[names[0]]
        vals = np.stack([obj[n].values for n in names], axis=0)
        coords = dict(first.coords)
        coords[feature_dim] = np.array(names)
        return GridArray(vals, (feature_dim,) + first.dims, coords), False
    if _is_xarray(obj):
        import xarray as xr

        if isinstance(obj, xr.Dataset):
            obj = obj.to_array(feature_dim)  # core.py:429-430
        coords = {k: np.asarray(v.values) for k, v in obj.coords.items() if v.ndim <= 1}
        return GridArray(np.asarray(obj.values), obj.dims, coords, obj.name), True
    raise TypeError(f"unsupported input type {type(obj)}; expected xarray.DataArray/Dataset or GridArray")


def _from_grid(g, as_xarray):
    if not as_xarray:
        return g
    import xarray as xr

    coords = {k: ((k,), v) if np.ndim(v) == 1 and k in g.dims else v for k, v in g.coords.items()
              if (k in g.dims) or np.ndim(v) == 0}
    return xr.DataArray(g.values, dims=g.dims, coords=coords)


def _unchunked(obj):
    """a block handed to a child model: plain (loaded) data without chunk structure"""
    if isinstance(obj, GridDataset):
        return GridDataset({k: _unchunked(v) for k, v in obj.items()})
    if hasattr(obj, "unchunked"):  # InterpolatedGridArray: the block stays coarse data + target coordinates
        return obj.unchunked()
    if isinstance(obj, GridArray):
        return GridArray(obj.values, obj.dims, obj.coords, obj.name)
    if _is_xarray(obj):
        return obj.compute() if getattr(obj, "chunks", None) else obj
    return obj


def _time_index(g, dim):
    """core.py:52-64: pandas index of the time coordinate (RangeIndex when absent)."""
    if dim in g.coords:
        v = g.coords[dim]
        return v if isinstance(v, pd.Index) else pd.Index(np.asarray(v))
    return pd.RangeIndex(g.sizes[dim])


def _da_to_df(values_2d, index, columns):
    return pd.DataFrame(values_2d, columns=columns, index=index)


class _BatchedModels:
    """Fitted state of a whole grid held by the engine (replaces the object array of estimators)."""

    def __init__(self, kind, grid_model, mask, spatial_dims, spatial_shape, coords):
        self.kind = kind  # 'bcsd' | 'analog' | 'linreg' | 'qm' | 'cunnane' | 'qmapper' | 'zscore' | 'grouped' | 'arrm' | 'loop'
        self.grid_model = grid_model
        self.mask = mask
        self.spatial_dims = spatial_dims
        self.spatial_shape = spatial_shape
        self.coords = coords


class _BlockedModels:
    """Fitted state of a chunked grid: one fitted PointWiseDownscaler per spatial block (the reference maps
    ``_fit_wrapper`` over the blocks of a dask-backed input, core.py:256-262; the engine then batches the cells of a block)."""

    kind = "blocks"

    def __init__(self, spatial_dims, spatial_shape, chunksizes, blocks):
        self.spatial_dims = tuple(spatial_dims)
        self.spatial_shape = tuple(spatial_shape)
        self.chunksizes = chunksizes  # dim -> tuple of block lengths
        self.blocks = blocks          # list of ({dim: slice}, fitted child)

    @property
    def sizes(self):
        return dict(zip(self.spatial_dims, self.spatial_shape))


def _block_slices(dims, chunksizes):
    """all blocks of a chunked grid as {dim: slice} dicts, last dim fastest"""
    import itertools

    per_dim = []
    for d in dims:
        edges = np.concatenate([[0], np.cumsum(chunksizes[d])]).astype(int)
        per_dim.append([slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])])
    return [dict(zip(dims, combo)) for combo in itertools.product(*per_dim)]


def _isel(obj, sel):
    """positional block selection on GridArray / GridDataset / xarray objects, ignoring dims the object does not have"""
    if isinstance(obj, GridDataset):
        return GridDataset({k: _isel(v, sel) for k, v in obj.items()})
    return obj.isel(**{d: s for d, s in sel.items() if d in obj.dims})


class PointWiseDownscaler:
    """Pointwise downscaling model wrapper (core.py:200-448).

    Parameters
    ----------
    model : estimator implementing fit/predict
    dim : str, dimension to apply the model along (default ``time``)
    """

    def __init__(self, model, dim="time"):
        self._dim = dim
        self._model = model
        self._models = None
        if not hasattr(model, "fit"):
            raise TypeError(f"Type {type(model)} does not have the fit method required by PointWiseDownscaler")

    # ------------------------------------------------------------------------------------------
    def _to_feature_x(self, X, feature_dim=DEFAULT_FEATURE_DIM):
        """core.py:427-440 -> GridArray with dims (time, feature, *spatial)."""
        g, was_x = _to_grid(X, feature_dim)
        if feature_dim not in g.dims:
            vals = np.expand_dims(g.values, 1)
            dims = (g.dims[0], feature_dim) + g.dims[1:] if g.dims[0] == self._dim else None
            if dims is None:  # time is not leading: move it first, then insert the feature axis
                g = g.transpose(self._dim, ...)
                vals = np.expand_dims(g.values, 1)
                dims = (self._dim, feature_dim) + g.dims[1:]
            coords = dict(g.coords)
            coords[feature_dim] = np.array([f"{feature_dim}_0"])
            g = GridArray(vals, dims, coords, g.name)
        return g.transpose(self._dim, feature_dim, ...), was_x

    def _spatial_chunks(self, X, feature_dim):
        """(spatial dims, sizes, dim -> block lengths) of a chunked input, else None.  Time and feature dims are always taken
        whole (the reference needs them in one chunk: core.py:435-437 and the ``time: -1`` of its examples)."""
        if not getattr(X, "chunks", None):
            return None
        cs = X.chunksizes
        probe = X[list(X)[0]] if isinstance(X, GridDataset) else X
        if _is_xarray(X) and not hasattr(X, "dims"):
            return None
        dims = [d for d in probe.dims if d not in (self._dim, feature_dim)]
        sizes = dict(probe.sizes)
        chunksizes = {d: tuple(int(b) for b in cs[d]) if d in cs else (int(sizes[d]),) for d in dims}
        if all(len(chunksizes[d]) == 1 for d in dims):
            return None
        return dims, sizes, chunksizes

    def _apply_blocks(self, method, X, kwargs):
        """predict / transform / inverse_transform of a block-fitted grid: every block through its own fitted child, results
        assembled along the spatial dims (core.py:300-336 maps ``_predict_wrapper`` over the blocks)."""
        mdl = self._models
        was_x = _is_xarray(X)
        feature_dim = kwargs.get("feature_dim", DEFAULT_FEATURE_DIM)

        def run(sel, child):
            rg, _ = _to_grid(getattr(child, method)(_unchunked(_isel(X, sel)), **kwargs), feature_dim)
            return rg

        if not was_x:  # GridArray / GridDataset: blocks on demand (like the reference's map_blocks result)
            thunks = [(sel, (lambda s=sel, c=child: run(s, c))) for sel, child in mdl.blocks]
            first = thunks[0][1]()
            probe = X[list(X)[0]] if isinstance(X, GridDataset) else X
            coords = {k: v for k, v in first.coords.items() if k not in mdl.spatial_dims}
            for k in mdl.spatial_dims:
                if k in getattr(probe, "coords", {}):
                    coords[k] = probe.coords[k]
            return LazyGridArray(thunks, first, mdl.spatial_dims, mdl.sizes, mdl.chunksizes, coords)
        out = None
        for sel, child in mdl.blocks:
            rg = run(sel, child)
            if out is None:
                sizes = dict(rg.sizes)
                sizes.update(mdl.sizes)
                full = np.full([sizes[d] for d in rg.dims], np.nan, dtype=rg.dtype)
                coords = {k: v for k, v in rg.coords.items() if k not in mdl.spatial_dims}
                out = (full, rg.dims, coords)
            out[0][tuple(sel.get(d, slice(None)) for d in out[1])] = rg.values
        full, out_dims, coords = out
        import xarray as xr

        xc = {k: v for k, v in X.coords.items() if set(v.dims) <= set(out_dims)}
        xc.update({k: ((k,), v) for k, v in coords.items() if k in out_dims and k not in xc})
        res = xr.DataArray(full, dims=out_dims, coords=xc)
        try:  # like the reference's map_blocks result: same spatial chunk structure (needs dask; without it the eager array)
            return res.chunk({d: mdl.chunksizes[d] for d in mdl.spatial_dims})
        except Exception:  # noqa: BLE001
            return res

    def _batched(self):
        m = self._model
        if isinstance(m, BcsdBase):
            # every cell's copy runs _pre_fit in the reference ('daily_nasa-nex' swaps the grouper class in, bcsd.py:34-44);
            # the prototype stays untouched
            self._bcsd_proto = copy.deepcopy(m)
            self._bcsd_proto._pre_fit()
            check_supported(self._bcsd_proto)
            return "bcsd"
        if isinstance(m, (PureAnalog, AnalogRegression)):
            if isinstance(m, AnalogRegression):
                m._check()
            else:
                from .gard import check_tree_kwargs

                check_tree_kwargs(m)
            return "analog"
        if isinstance(m, PureRegression):
            m._check()
            return "linreg"
        if isinstance(m, QuantileMappingReressor):
            check_extrapolate(m.extrapolate)
            m._engine_code()
            return "qm"
        if isinstance(m, CunnaneTransformer):
            m._check()
            return "cunnane"
        if isinstance(m, QuantileMapper):
            m._check()
            return "qmapper"
        if isinstance(m, ZScoreRegressor):
            return "zscore"
        if isinstance(m, GroupedRegressor):
            m._check_engine()
            return "grouped"
        if isinstance(m, PiecewiseLinearRegression):
            m._check()
            return "arrm"
        return None

    # ------------------------------------------------------------------------------------------
    def fit(self, X, *args, **kwargs):
        """Fit the model for every cell (core.py:225-264)."""
        kws = {"along_dim": self._dim, "feature_dim": DEFAULT_FEATURE_DIM} | kwargs
        if len(args) > 1:
            raise ValueError(f"Expected at most 1 positional argument, got {len(args)}")
        feature_dim = kws["feature_dim"]
        blocks = self._spatial_chunks(X, feature_dim)
        if blocks is not None:  # chunked input (dask-backed xarray, GridArray.chunk): block by block (core.py:256-262)
            dims, sizes, chunksizes = blocks
            fitted = []
            for sel in _block_slices(dims, chunksizes):
                child = PointWiseDownscaler(copy.deepcopy(self._model), self._dim)
                child.fit(_unchunked(_isel(X, sel)), *[_unchunked(_isel(a, sel)) for a in args], **kwargs)
                fitted.append((sel, child))
            self._models = _BlockedModels(dims, [sizes[d] for d in dims], chunksizes, fitted)
            return
        if self._resident_input(X) and args:
            return self._fit_resident(X, args[0], feature_dim)
        Xg, _ = self._to_feature_x(X, feature_dim)
        spatial_dims, spatial_shape = Xg.dims[2:], Xg.shape[2:]
        yg = self._aligned_y(args[0], Xg.sizes, spatial_dims, feature_dim) if args else None
        T, F = Xg.shape[:2]
        C = int(np.prod(spatial_shape, dtype=np.int64)) if spatial_shape else 1
        Xv = np.ascontiguousarray(Xg.values, dtype=np.float64).reshape(T, F, C)
        mask = ~np.isnan(Xv[0, 0, :])  # core.py:35-37
        index = _time_index(Xg, self._dim)
        kind = self._batched()
        coords = {k: v for k, v in Xg.coords.items() if k in spatial_dims}
        if kind is None:
            self._models = self._fit_loop(Xg, yg, Xv, mask, index, feature_dim, spatial_dims, spatial_shape, coords,
                                          {k: v for k, v in kws.items() if k not in ("along_dim", "feature_dim")})
            return
        m = self._model
        if kind in ("cunnane", "qmapper"):  # transformers: fit(X) only (a y, if given, is ignored like in the reference)
            if F != 1:
                if kind == "cunnane":
                    raise ValueError("CunnaneTransformer.fit() only supports a single feature")
                raise ValueError(f"Found array with {F} features (shape=({T}, {F})) while a maximum of 1 is required")
            gm = (CunnaneGridModel(m.extrapolate, m.n_endpoints) if kind == "cunnane" else QuantileMapperGridModel(detrend=m.detrend)).fit(Xv[:, 0, :])
            gm.status_ = gm.state.export(with_y=False)["status"] if kind == "cunnane" else gm.status_
            self._raise_for_status(gm.status_, Xv[:, 0, :], Xv[:, 0, :])
            self._models = _BatchedModels(kind, gm, mask, spatial_dims, spatial_shape, coords)
            return
        if yg is None:
            raise TypeError(f"{type(self._model).__name__}.fit() missing 1 required positional argument: 'y'")
        yv = np.ascontiguousarray(yg.values, dtype=np.float64).reshape(T, C)
        if kind == "bcsd":
            if F != 1:
                msg = "BCSD only supports up to 4 features, found {}" if m._kind == _lib.BCSD_TAS else "BCSD only supports 1 feature, found {}"
                raise ValueError(msg.format(F))
            gm = self._bcsd_proto._new_grid()
            if Xg.dtype == np.float32 and yg.dtype == np.float32:  # float32 grids cross PCIe as float32 (widened in HBM, exact)
                gm.fit(np.ascontiguousarray(Xg.values).reshape(T, C), np.ascontiguousarray(yg.values).reshape(T, C), index)
            else:
                gm.fit(Xv[:, 0, :], yv, index)
            self._raise_for_status(gm.status_, Xv[:, 0, :], yv)
        elif kind == "zscore":
            if F != 1:
                raise ValueError(f"Zscore only supports 1 feature, found {F}")
            if T == 1:  # zscore.py:51-52: X.squeeze() of one sample is a scalar
                raise TypeError("X.squeeze() must be a pd.Series, got float64")
            gm = ZScoreGridModel(m.window_width).fit(Xv[:, 0, :], yv, index)
            self._raise_for_status(gm.status_, Xv[:, 0, :], yv)
        elif kind == "arrm":
            if F != 1:
                raise ValueError(f"Found array with {F} features (shape=({T}, {F})) while a maximum of 1 is required")
            extra = [k for k in kws if k not in ("along_dim", "feature_dim")]
            if extra:  # the class raises for them, as pwlf's fit_with_breaks would
                raise TypeError(f"fit_with_breaks() got an unexpected keyword argument '{extra[0]}'")
            gm = ArrmGridModel(m.n_segments).fit(Xv[:, 0, :], yv)
            self._raise_for_status(gm.status_, Xv[:, 0, :], yv)
        elif kind == "grouped":
            plan = m._fit_plan(index)
            if plan is None:
                from .grouping import SUPPORTED

                raise NotImplementedError(f"GroupedRegressor on a grid with overlapping groups from {m.fit_grouper!r}: {SUPPORTED}")
            per_step, labels, window = plan
            gm = GroupedGridModel(window).fit_labels(Xv, yv, per_step, labels)
            if not gm.fitted_.all():
                from .grouping import NO_SAMPLES_MESSAGE

                raise ValueError(NO_SAMPLES_MESSAGE.format(F=F))
            bad = mask & (gm.status_ == _lib.CELL_NONFINITE)
            if bad.any():
                c = int(np.flatnonzero(bad)[0])
                self._raise_for_status(np.where(bad, _lib.CELL_NONFINITE, 0), Xv[:, :, c:c + 1].reshape(T, -1), yv[:, c:c + 1], cell=c)
        elif kind == "qm":
            if F != 1:
                raise ValueError(f"Found array with {F} features (shape=({T}, {F})) while a maximum of 1 is required")
            if T < 2 * m.n_endpoints + 1:
                raise ValueError(f"Found array with {T} sample(s) (shape=({T}, 1)) while a minimum of {2 * m.n_endpoints + 1} is required.")
            gm = QmGridModel(m._engine_code(), m.extrapolate, n_endpoints=m.n_endpoints)
            gm.fit(Xv[:, 0, :], yv)
            gm.status_ = gm.state.export()["status"]
            self._raise_for_status(gm.status_, Xv[:, 0, :], yv)
        else:
            gm = RegressionGridModel(thresh=m.thresh).fit(Xv, yv) if kind == "linreg" else AnalogGridModel(m.n_analogs).fit(Xv, yv)
            gm.status_ = np.where(mask, 0, _lib.CELL_MASKED).astype(np.int32)
            if kind == "linreg" and m.thresh is not None:
                e = gm.export()
                live_one_class = mask & (e["status"] == _lib.CELL_ONE_CLASS)
                if (mask & (e["thresh_dropped"] | (e["status"] == _lib.CELL_ONE_CLASS))).any():  # gard.py:426-437, per cell
                    import warnings

                    warnings.warn("Found only one class while attempting logistic regression. Mutating attribute thresh")
                if live_one_class.any():  # the linear model of such a cell gets an empty sample (gard.py:439)
                    from .gard import NO_SAMPLES_MESSAGE

                    raise ValueError(NO_SAMPLES_MESSAGE.format(F=F))
            bad = mask & ~(np.isfinite(Xv).all(axis=(0, 1)) & np.isfinite(yv).all(axis=0))
            if bad.any():
                c = int(np.flatnonzero(bad)[0])
                self._raise_for_status(np.where(bad, _lib.CELL_NONFINITE, 0), Xv[:, :, c:c + 1].reshape(T, -1), yv[:, c:c + 1], cell=c)
        self._models = _BatchedModels(kind, gm, mask, spatial_dims, spatial_shape, coords)

    def _aligned_y(self, y, x_sizes, spatial_dims, feature_dim):
        """the reference selects y[index] by dimension *name* for every cell of X (core.py:86-93): align y to X's cell order"""
        yg, _ = _to_grid(y, feature_dim)
        if set(yg.dims) != {self._dim, *spatial_dims}:
            raise ValueError(f"y has dims {yg.dims}; expected {(self._dim,) + tuple(spatial_dims)} (the spatial dims of X, no feature dim)")
        if tuple(yg.dims) != (self._dim,) + tuple(spatial_dims):  # (a lazy y already in X's order stays lazy)
            yg = yg.transpose(self._dim, *spatial_dims)
        if any(yg.sizes[d] != x_sizes[d] for d in yg.dims):
            raise ValueError(f"y has sizes {yg.sizes}, X has {x_sizes}")
        return yg

    # ---- single-feature BCSD on an interpolated coarse field: the fine X is produced in HBM and never crosses PCIe ----
    def _resident_input(self, X):
        from .regrid import InterpolatedGridArray
        from .resample import ResampledGridArray

        return (isinstance(X, (InterpolatedGridArray, ResampledGridArray)) and isinstance(self._model, BcsdBase) and len(X.dims) == 3
                and X.dims[0] == self._dim)

    def _fit_resident(self, X, y, feature_dim):
        from .resample import ResampledGridArray

        spatial_dims, spatial_shape = tuple(X.dims[1:]), tuple(X.shape[1:])
        yg = self._aligned_y(y, X.sizes, spatial_dims, feature_dim)
        T, C = X.shape[0], int(np.prod(spatial_shape, dtype=np.int64))
        self._batched()
        gm = self._bcsd_proto._new_grid()
        Xd = X.device_field(gm.ctx)
        mask = ~np.isnan(Xd.rows(0, 1).to_host()[0])  # core.py:35-37 on the regridded first time step: one row comes back
        def y_host():
            return np.ascontiguousarray(yg.values, dtype=np.float64).reshape(T, C)

        # (a resampled y is reduced in HBM as well; _aligned_y has brought any other y to X's order on the host)
        yd = yg.device_field(gm.ctx) if isinstance(yg, ResampledGridArray) else gm.ctx.to_device(y_host())
        gm.fit(Xd, yd, _time_index(X, self._dim))
        if np.isin(gm.status_, (_lib.CELL_NONFINITE, _lib.CELL_BAD_CLIMO)).any():  # (the message names X or y: needs the values)
            self._raise_for_status(gm.status_, np.asarray(X.values, dtype=np.float64).reshape(T, C), y_host())
        coords = {k: v for k, v in X.coords.items() if k in spatial_dims}
        self._models = _BatchedModels("bcsd", gm, mask, spatial_dims, spatial_shape, coords)

    def _predict_resident(self, X):
        mdl = self._models
        T, C = X.shape[0], int(np.prod(mdl.spatial_shape, dtype=np.int64))
        out, status = mdl.grid_model.predict(X.device_field(mdl.grid_model.ctx), _time_index(X, self._dim))
        if np.isin(status, (_lib.CELL_NONFINITE, _lib.CELL_BAD_CLIMO)).any():
            Xv = np.asarray(X.values, dtype=np.float64).reshape(T, C)
            self._raise_for_status(status, Xv, Xv)
        vals = out.to_host().reshape((T,) + tuple(mdl.spatial_shape))
        return GridArray(vals, X.dims, dict(X.coords))

    @staticmethod
    def _raise_for_status(status, Xv, yv, cell=None):
        """Raise like the reference would for the first offending cell (base.py:18-20, bcsd.py:140-141)."""
        bad = np.flatnonzero((status == _lib.CELL_NONFINITE) | (status == _lib.CELL_BAD_CLIMO))
        if not len(bad):
            return
        c = int(bad[0])
        if status[c] == _lib.CELL_BAD_CLIMO:
            raise ValueError("Invalid value in target climatology")
        xc = Xv if cell is not None else Xv[:, c]
        yc = yv if cell is not None else yv[:, c]
        for name, a in (("X", xc), ("y", yc)):
            if np.isnan(a).any():
                raise ValueError(f"Input {name} contains NaN.")
            if not np.isfinite(a).all():
                raise ValueError(f"Input {name} contains infinity or a value too large for dtype('float64').")
        raise ValueError("Input contains NaN.")

    def _fit_loop(self, Xg, yg, Xv, mask, index, feature_dim, spatial_dims, spatial_shape, coords, fit_kwargs):
        """The reference's per-cell loop (core.py:69-97) for estimators the engine does not batch."""
        T, F, C = Xv.shape
        columns = list(Xg.coords.get(feature_dim, [f"feature{i}" for i in range(F)]))
        yv = None if yg is None else np.asarray(yg.values).reshape(T, C)
        models = np.full(C, None, dtype=object)
        for c in range(C):
            mod = copy.deepcopy(self._model)
            if not mask[c]:
                continue
            xdf = _da_to_df(Xv[:, :, c], index, columns)
            if yv is not None:
                ydf = _da_to_df(yv[:, c:c + 1], index, [f"{feature_dim}_0"])
                models[c] = mod.fit(xdf, ydf, **fit_kwargs)
            else:
                models[c] = mod.fit(xdf, **fit_kwargs)
        return _BatchedModels("loop", models, mask, spatial_dims, spatial_shape, coords)

    def _align_to_fitted(self, Xg, feature_dim):
        """Bring the spatial dims of a predict / transform input into the fitted order (the reference looks the fitted models
        up by dimension name, core.py:110-141): same dim names required, any order accepted."""
        fitted = tuple(self._models.spatial_dims)
        if set(Xg.dims[2:]) != set(fitted):
            raise ValueError(f"spatial dims {Xg.dims[2:]} do not match the fitted grid's {fitted}")
        Xg = Xg.transpose(self._dim, feature_dim, *fitted)
        if tuple(Xg.shape[2:]) != tuple(self._models.spatial_shape):
            raise ValueError(f"spatial shape {Xg.shape[2:]} does not match the fitted grid {self._models.spatial_shape}")
        return Xg

    # ------------------------------------------------------------------------------------------
    def predict(self, X, **kwargs):
        """Predict for every fitted cell (core.py:266-338); masked cells stay NaN."""
        if self._models is None:
            raise ValueError("PointWiseDownscaler is not fitted: call fit() first")
        if isinstance(self._models, _BlockedModels):
            return self._apply_blocks("predict", X, kwargs)
        kws = {"along_dim": self._dim, "feature_dim": DEFAULT_FEATURE_DIM} | kwargs
        feature_dim = kws["feature_dim"]
        mdl = self._models
        if mdl.kind == "bcsd" and self._resident_input(X) and (tuple(X.dims[1:]), tuple(X.shape[1:])) == (tuple(mdl.spatial_dims), tuple(mdl.spatial_shape)):
            return self._predict_resident(X)
        Xg, was_x = self._to_feature_x(X, feature_dim)
        Xg = self._align_to_fitted(Xg, feature_dim)
        T, F = Xg.shape[:2]
        spatial_dims, spatial_shape = Xg.dims[2:], Xg.shape[2:]
        C = int(np.prod(spatial_shape, dtype=np.int64)) if spatial_shape else 1
        Xv = np.ascontiguousarray(Xg.values, dtype=np.float64).reshape(T, F, C)
        index = _time_index(Xg, self._dim)
        n_outputs = getattr(self._model, "n_outputs", 1)  # core.py:294-298
        output_names = getattr(self._model, "output_names", None)
        mdl = self._models
        coords = {k: v for k, v in Xg.coords.items() if k != feature_dim}
        if mdl.kind == "bcsd":
            if Xg.dtype == np.float32 and F == 1:  # in and out as float32, widened / narrowed on the device
                out, status = mdl.grid_model.predict(np.ascontiguousarray(Xg.values).reshape(T, C), index, out_dtype=np.float32)
            else:
                out, status = mdl.grid_model.predict(Xv[:, 0, :], index)
            self._raise_for_status(status, Xv[:, 0, :], Xv[:, 0, :])
            vals = out.reshape((T,) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            res = GridArray(vals, (self._dim,) + spatial_dims, coords)
        elif mdl.kind == "zscore":
            if F != 1:
                raise ValueError(f"X must have exactly 1 feature, got {F}")
            out, status, _ = mdl.grid_model.predict(Xv[:, 0, :])
            self._raise_for_status(status, Xv[:, 0, :], Xv[:, 0, :])
            vals = out.reshape((T,) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            res = GridArray(vals, (self._dim,) + spatial_dims, coords)
        elif mdl.kind == "arrm":
            if F != 1:
                raise ValueError(f"Found array with {F} features (shape=({T}, {F})) while a maximum of 1 is required")
            out, status = mdl.grid_model.predict(Xv[:, 0, :])
            self._raise_for_status(status, Xv[:, 0, :], Xv[:, 0, :])
            vals = out.reshape((T,) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            res = GridArray(vals, (self._dim,) + spatial_dims, coords)
        elif mdl.kind == "grouped":
            out, status = mdl.grid_model.predict_labels(Xv, self._model._predict_labels(index))
            if (mdl.mask & (status == _lib.CELL_NONFINITE)).any():
                raise ValueError("Input X contains NaN.")
            vals = out.reshape((T,) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            res = GridArray(vals, (self._dim,) + spatial_dims, coords)
        elif mdl.kind == "qm":
            out, status = mdl.grid_model.predict(Xv[:, 0, :])
            self._raise_for_status(status, Xv[:, 0, :], Xv[:, 0, :])
            vals = out.reshape((T,) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            res = GridArray(vals, (self._dim,) + spatial_dims, coords)
        elif mdl.kind in ("analog", "linreg"):
            m = self._model
            if mdl.kind == "linreg":
                out, status = mdl.grid_model.predict(Xv)
            elif isinstance(m, AnalogRegression):
                out, status = mdl.grid_model.predict_regression(Xv, m.thresh)
            else:
                out, status = mdl.grid_model.predict_pure(Xv, m.kind, m.thresh)
            if (status == _lib.CELL_NONFINITE).any():
                raise ValueError("Input X contains NaN.")
            if (status == _lib.CELL_ONE_CLASS).any():  # a query without any analog above the threshold (gard.py:204-207)
                from .gard import ONE_CLASS_MESSAGE

                raise ValueError(ONE_CLASS_MESSAGE)
            vals = out.reshape((T, 3) + tuple(spatial_shape)).astype(Xg.dtype, copy=False)
            coords[feature_dim] = np.array(output_names)
            res = GridArray(vals, (self._dim, feature_dim) + spatial_dims, coords)
        else:
            res = self._predict_loop(Xg, Xv, index, feature_dim, n_outputs, output_names, spatial_dims, spatial_shape,
                                     coords, {k: v for k, v in kws.items() if k not in ("along_dim", "feature_dim")})
        return _from_grid(res, was_x)

    def _predict_loop(self, Xg, Xv, index, feature_dim, n_outputs, output_names, spatial_dims, spatial_shape, coords, kw):
        """core.py:100-143 for estimators the engine does not batch."""
        T, F, C = Xv.shape
        columns = list(Xg.coords.get(feature_dim, [f"feature{i}" for i in range(F)]))
        shape = (T, C) if n_outputs == 1 else (T, n_outputs, C)
        y = np.full(shape, np.nan, dtype=Xg.dtype)
        for c in range(C):
            model = self._models.grid_model[c]
            if model is None:
                continue
            ydf = model.predict(_da_to_df(Xv[:, :, c], index, columns), **kw)
            y[..., c] = np.asarray(ydf).squeeze()
        if n_outputs == 1:
            return GridArray(y.reshape((T,) + tuple(spatial_shape)), (self._dim,) + spatial_dims, coords)
        coords[feature_dim] = np.array(output_names)
        return GridArray(y.reshape((T, n_outputs) + tuple(spatial_shape)), (self._dim, feature_dim) + spatial_dims, coords)

    # ------------------------------------------------------------------------------------------
    def transform(self, X, **kwargs):
        """Apply the fitted per-cell transformers (core.py:340-371)."""
        return self._transform(X, "transform", kwargs)

    def inverse_transform(self, X, **kwargs):
        """Apply the inverse of the fitted per-cell transformers (core.py:373-403)."""
        return self._transform(X, "inverse_transform", kwargs)

    def _transform(self, X, direction, kwargs):
        """core.py:146-171 (``_transform_wrapper``): same dims / shape as the feature-normalised X, masked cells NaN."""
        if self._models is None:
            raise ValueError("PointWiseDownscaler is not fitted: call fit() first")
        if isinstance(self._models, _BlockedModels):
            return self._apply_blocks(direction, X, kwargs)
        kind = self._models.kind
        if kind not in ("loop", "cunnane", "qmapper") or (kind == "qmapper" and direction != "transform"):
            raise AttributeError(f"{type(self._model).__name__} has no {direction}()")
        kws = {"feature_dim": DEFAULT_FEATURE_DIM} | kwargs
        feature_dim = kws.pop("feature_dim")
        Xg, was_x = self._to_feature_x(X, feature_dim)
        Xg = self._align_to_fitted(Xg, feature_dim)
        T, F = Xg.shape[:2]
        spatial_shape = Xg.shape[2:]
        C = int(np.prod(spatial_shape, dtype=np.int64)) if spatial_shape else 1
        if kind != "loop":  # one batched launch for the whole grid
            if F != 1:
                raise ValueError(f"{type(self._model).__name__}.{direction}() only supports a single feature")
            Xb = np.ascontiguousarray(Xg.values, dtype=np.float64).reshape(T, C)
            out, status = getattr(self._models.grid_model, direction)(Xb)
            self._raise_for_status(status, Xb, Xb)
            if kind == "cunnane" and direction == "transform" and np.isinf(out[:, self._models.mask]).any():
                raise AttributeError("'numpy.ndarray' object has no attribute 'values' (CunnaneTransformer.transform of values "
                                     f"outside the fitted range with extrapolate={self._model.extrapolate!r}: quantile.py:497)")
            out = out.reshape(Xg.shape).astype(Xg.dtype, copy=False)
            return _from_grid(GridArray(out, Xg.dims, dict(Xg.coords)), was_x)
        Xv = np.asarray(Xg.values).reshape(T, F, C)
        index = _time_index(Xg, self._dim)
        columns = list(Xg.coords.get(feature_dim, [f"feature{i}" for i in range(F)]))
        out = np.full((T, F, C), np.nan, dtype=Xg.dtype)
        for c in range(C):
            model = self._models.grid_model[c]
            if model is None:
                continue
            res = getattr(model, direction)(_da_to_df(Xv[:, :, c], index, columns), **kws)
            out[:, :, c] = np.asarray(res).reshape(T, F)
        return _from_grid(GridArray(out.reshape(Xg.shape), Xg.dims, dict(Xg.coords)), was_x)

    # ------------------------------------------------------------------------------------------
    def _cell_model(self, c, cache):
        """The fitted estimator of cell ``c`` of an engine-batched grid, rebuilt from the exported state: what the
        reference keeps per cell in its object array (core.py:81-96)."""
        mdl = self._models
        if mdl.kind == "loop":
            return mdl.grid_model[c]
        if not mdl.mask[c]:
            return None
        m = self._model
        if mdl.kind == "bcsd":
            e = cache.setdefault("e", mdl.grid_model.export())
            est = copy.deepcopy(self._bcsd_proto)
            est._adopt(e, c)
            est.n_features_in_ = 1
            return est
        if mdl.kind == "linreg":
            e = cache.setdefault("e", mdl.grid_model.export())
            est = copy.deepcopy(m)
            est.n_features_in_ = e["coef"].shape[0]
            if est.thresh is not None and e["thresh_dropped"][c]:
                est.thresh = None  # gard.py:437
            est._adopt(e, c)
            return est
        if mdl.kind == "zscore":
            e = cache.setdefault("e", mdl.grid_model.export())
            est = copy.deepcopy(m)
            est._adopt(e, c, e["labels"])
            return est
        if mdl.kind in ("grouped", "arrm"):
            e = cache.setdefault("e", mdl.grid_model.export())
            est = copy.deepcopy(m)
            est._adopt(e, c)
            return est
        if mdl.kind == "analog":
            est = copy.deepcopy(m)
            est.k_ = mdl.grid_model.k_
            est.n_features_in_ = mdl.grid_model.state.info()["F"]
            return est
        if mdl.kind == "qm":
            e = cache.setdefault("e", mdl.grid_model.state.export())
            est = copy.deepcopy(m)
            est._X_cdf = est._extended(e["x_sorted"][c])
            est._y_cdf = est._extended(e["y_sorted"][c])
            est.n_features_in_ = 1
            return est
        if mdl.kind == "cunnane":
            from .quantile import Cdf, plotting_positions

            e = cache.setdefault("e", mdl.grid_model.state.export(with_y=False))
            est = copy.deepcopy(m)
            est.cdf_ = Cdf(plotting_positions(e["x_sorted"].shape[1]), e["x_sorted"][c])
            est.n_features_in_ = 1
            return est
        if mdl.kind == "qmapper":
            from .quantile import Cdf, FittedCunnane, plotting_positions

            e = cache.setdefault("e", mdl.grid_model.state.export())
            est = copy.deepcopy(m)
            vals = e["y_sorted"][c]
            est.x_cdf_fit_ = FittedCunnane(Cdf(plotting_positions(len(vals)), vals))
            if est.detrend:
                from .trend import FittedLine, FittedTrend

                est.x_trend_fit_ = FittedTrend(FittedLine(np.array([[e["y_trend"][c, 0, 0]]]), np.array([e["y_trend"][c, 0, 1]])))
            est.n_features_in_ = 1
            return est
        raise NotImplementedError(f"get_attr is not available for {mdl.kind} grids")

    def get_attr(self, key, dtype=np.float64, template_output=None):
        """Get attribute values specified in ``key`` from each of the pointwise models (core.py:405-425, 174-197): an array
        shaped like the model grid, or like ``template_output`` (whose non-spatial dims receive array-valued attributes).
        Engine-batched grids rebuild the per-cell fitted attributes from the exported state.  Extension: without a template,
        the BCSD climatologies ``y_climo_`` / ``_x_climo`` come back as [group, *spatial] fields, the ZScoreRegressor
        parameters ``shift_`` / ``scale_`` as [day, *spatial] fields, and the GroupedRegressor models ``coef_`` / ``intercept_`` as
        [group, feature, *spatial] / [group, *spatial] fields, and the PiecewiseLinearRegression breaks ``fit_breaks_`` as a
        [break, *spatial] field."""
        mdl = self._models
        if mdl is None:
            raise ValueError("PointWiseDownscaler is not fitted: call fit() first")
        if isinstance(mdl, _BlockedModels):
            return self._get_attr_blocks(key, dtype, template_output)
        if mdl.kind == "bcsd" and key in ("y_climo_", "_x_climo") and template_output is None:
            e = mdl.grid_model.export()
            a = e["y_climo" if key == "y_climo_" else "x_climo"].T.astype(dtype)  # [G, C]
            a = np.where(mdl.mask[None, :], a, np.nan)
            coords = dict(mdl.coords)
            coords["group"] = e["keys"]
            return GridArray(a.reshape((a.shape[0],) + tuple(mdl.spatial_shape)), ("group",) + tuple(mdl.spatial_dims), coords)
        if mdl.kind == "grouped" and key in ("coef_", "intercept_") and template_output is None:
            e = mdl.grid_model.export()
            a = np.where(mdl.mask, e[key[:-1]], np.nan).astype(dtype)  # [n, F, C] or [n, C]
            coords = dict(mdl.coords)
            coords["group"] = e["labels"]
            lead = ("group", DEFAULT_FEATURE_DIM) if key == "coef_" else ("group",)
            return GridArray(a.reshape(a.shape[:len(lead)] + tuple(mdl.spatial_shape)), lead + tuple(mdl.spatial_dims), coords)
        if mdl.kind == "arrm" and key == "fit_breaks_" and template_output is None:
            a = np.where(mdl.mask[None, :], mdl.grid_model.export()["breaks"], np.nan).astype(dtype)  # [B, C]
            coords = dict(mdl.coords)
            coords["break"] = np.arange(a.shape[0])
            return GridArray(a.reshape((a.shape[0],) + tuple(mdl.spatial_shape)), ("break",) + tuple(mdl.spatial_dims), coords)
        if mdl.kind == "zscore" and key in ("shift_", "scale_") and template_output is None:
            e = mdl.grid_model.export()
            a = np.where(mdl.mask[None, :], e[key[:-1]], np.nan).astype(dtype)  # [K, C]
            coords = dict(mdl.coords)
            coords["day"] = e["labels"]
            return GridArray(a.reshape((a.shape[0],) + tuple(mdl.spatial_shape)), ("day",) + tuple(mdl.spatial_dims), coords)
        sp_dims, sp_shape = tuple(mdl.spatial_dims), tuple(mdl.spatial_shape)
        was_x = False
        if template_output is None:
            dims, shape, coords = sp_dims, sp_shape, dict(mdl.coords)
        else:
            if _is_xarray(template_output):
                import xarray as xr

                was_x = True
                if isinstance(template_output, xr.Dataset):  # core.py:184-186
                    template_output = template_output[list(template_output.data_vars)[0]]
            elif isinstance(template_output, GridDataset):
                template_output = template_output[list(template_output)[0]]
            tg, _ = _to_grid(template_output, DEFAULT_FEATURE_DIM)
            dims, shape, coords = tg.dims, tg.shape, dict(tg.coords)
            if not set(sp_dims) <= set(dims):
                raise ValueError(f"template_output dims {dims} do not contain the model grid's dims {sp_dims}")
        other = tuple(d for d in dims if d not in sp_dims)
        C = int(np.prod(sp_shape, dtype=np.int64)) if sp_shape else 1
        sizes = dict(zip(dims, shape))
        with np.errstate(invalid="ignore"):
            flat = np.full(tuple(sizes[d] for d in other) + (C,), np.nan, dtype=dtype)  # core.py:191
        cache = {}
        for c in range(C):
            est = self._cell_model(c, cache)
            if est is None:
                continue
            flat[..., c] = np.asarray(getattr(est, key)).reshape(flat.shape[:-1])  # core.py:194-196
        full = flat.reshape(tuple(sizes[d] for d in other) + sp_shape)
        g = GridArray(full, other + sp_dims, coords).transpose(*dims)
        return _from_grid(g, was_x)

    def _get_attr_blocks(self, key, dtype, template_output):
        mdl = self._models
        out = None
        for sel, child in mdl.blocks:
            tmpl = None if template_output is None else _unchunked(_isel(template_output, sel))
            res, _ = _to_grid(child.get_attr(key, dtype, tmpl), DEFAULT_FEATURE_DIM)
            if out is None:
                sizes = dict(res.sizes)
                sizes.update(mdl.sizes)
                with np.errstate(invalid="ignore"):
                    full = np.full([sizes[d] for d in res.dims], np.nan, dtype=dtype)
                out = (full, res.dims, {k: v for k, v in res.coords.items() if k not in mdl.spatial_dims})
            out[0][tuple(sel.get(d, slice(None)) for d in out[1])] = res.values
        return _from_grid(GridArray(*out), template_output is not None and _is_xarray(template_output))

    def __repr__(self):
        summary = [f"<skdownscale.{self.__class__.__name__}>", f"  Fit Status: {self._models is not None}",
                   f"  Model:\n    {self._model}"]
        return "\n".join(summary)
