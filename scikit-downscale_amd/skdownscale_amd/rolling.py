"""Rolling windows over the time axis on the GPU: the sliding statistics the reference takes per cell with pandas
(``x.rolling(9, center=True, min_periods=1).mean()`` of the BCSD trend, ``series.rolling(w, center=True).mean()`` / ``.std()`` of
``ZScoreRegressor``) and the workflow around it wants on whole grids: a day-of-year climatology smoothed by a circular 31-day window,
an n-day precipitation accumulation, the running mean and spread of a future series.

``GridRolling`` is what ``GridArray.rolling`` returns and ``RolledGridArray`` what its ``mean()`` / ``sum()`` / ``var()`` / ``std()``
return: the source and the window, computed when the field is asked for -- on the host through ``values``, or as a ``[T, C]``
``DeviceArray`` through ``device_field``.  The source is walked in blocks of time steps that carry the rows their windows reach
(``timesource.walk`` with a halo): a block of ``coarse.interp_like(obs)`` is regridded into device scratch, a block of a host
array is uploaded into it (float32 as float32), and a lazy ``resample`` / ``groupby`` / ``rolling`` result is taken from its own
``device_field``; none of them crosses PCIe as a fine float64 field.

The rule is pandas' fixed integer window per cell.  The window of step ``t`` is the steps ``t - back .. t - back + w - 1`` with
``back = w - 1`` (``w // 2`` with ``center=True``), clipped to the array -- or, with ``wrap=True``, taken modulo its length: pandas on
the series padded from its other end, for circular axes such as the day of the year.  NaN samples are skipped; fewer than
``min_periods`` (default ``w``) samples give NaN.  Each window is evaluated directly, in time order -- not by pandas' online
add / remove update --, so a result depends on its own window only and not on how ``scratch_bytes`` cuts the axis; the price is O(w)
work per output.  pandas' update carries rounding from the windows before, so the two differ by a few ulp of the series' scale.  The
result is float64 whatever the source.
"""
from __future__ import annotations

from .core import DeferredGridArray, chunk_lengths
from .resample import DEFAULT_SCRATCH_BYTES
from .timesource import walk

OPS = ("mean", "sum", "var", "std")
# what pandas' rolling offers beyond the four statistics the engine has: asked for by name, refused by name
_OTHER_REDUCTIONS = ("max", "min", "median", "count", "quantile", "apply", "construct", "agg", "aggregate", "sem", "skew", "kurt", "cov",
                     "corr", "rank", "prod", "reduce", "first", "last", "argmax", "argmin")


def window_back(window, center):
    """how many steps before ``t`` the window of ``t`` starts: pandas' trailing window ends at ``t``; the centred one of an even
    ``window`` has one step more before ``t`` than after it"""
    return window // 2 if center else window - 1


def check_window(window, min_periods):
    """``(window, min_periods)`` as ints, ``min_periods`` defaulting to ``window``; ValueError in pandas' words"""
    if isinstance(window, bool) or int(window) != window or window < 1:
        raise ValueError(f"window must be an integer 1 or greater, got {window!r}")
    window = int(window)
    if min_periods is None:
        return window, window
    if isinstance(min_periods, bool) or int(min_periods) != min_periods:
        raise ValueError("min_periods must be an integer")
    if min_periods < 0:
        raise ValueError("min_periods must be >= 0")
    if min_periods > window:
        raise ValueError(f"min_periods {int(min_periods)} must be <= window {window}")
    return window, int(min_periods)


class GridRolling:
    """``GridArray.rolling(time=w, ...)``: the window is checked, nothing is computed yet.  ``mean()`` / ``sum()`` / ``var(ddof=1)`` /
    ``std(ddof=1)`` -> ``RolledGridArray``."""

    def __init__(self, source, dim, window, center=False, min_periods=None, wrap=False, scratch_bytes=DEFAULT_SCRATCH_BYTES):
        if dim not in source.dims:
            raise ValueError(f"dim {dim!r} is not a dim of this array {source.dims}")
        self._window, self._min_periods = check_window(window, min_periods)
        T = source.sizes[dim]
        if T == 0:
            raise ValueError(f"nothing to roll over: dim {dim!r} has length 0")
        if wrap and self._window > T:
            raise ValueError(f"wrap=True: the window of {self._window} steps is longer than the {T} steps of dim {dim!r}")
        self._source, self._dim, self._center, self._wrap, self._scratch_bytes = source, dim, bool(center), bool(wrap), int(scratch_bytes)

    @property
    def dim(self):
        return self._dim

    @property
    def window(self):
        return self._window

    def _reduce(self, op, ddof=1):
        return RolledGridArray(self._source, self._dim, self._window, op, self._center, self._min_periods, ddof, self._wrap,
                               scratch_bytes=self._scratch_bytes)

    def mean(self):
        return self._reduce("mean")

    def sum(self):
        return self._reduce("sum")

    def var(self, ddof=1):
        return self._reduce("var", ddof)

    def std(self, ddof=1):
        return self._reduce("std", ddof)

    def __getattr__(self, name):
        if name in _OTHER_REDUCTIONS:
            def refuse(*args, **kwargs):
                raise NotImplementedError(f"rolling(...).{name}(): only mean(), sum(), var() and std() are implemented")

            return refuse
        raise AttributeError(name)

    def __repr__(self):
        return (f"<GridRolling {self._dim}={self._window} center={self._center} min_periods={self._min_periods} wrap={self._wrap} "
                f"over {self._source.sizes[self._dim]} steps>")


class RolledGridArray(DeferredGridArray):
    """A ``GridArray`` whose every step is a statistic of the window of steps around it along ``dim``: dims, coords and sizes are the
    source's."""

    _kind = "rolling"

    def __init__(self, source, dim, window, op="mean", center=False, min_periods=None, ddof=1, wrap=False, ctx=None,
                 scratch_bytes=DEFAULT_SCRATCH_BYTES, chunksizes=None):
        if op not in OPS:
            raise NotImplementedError(f"rolling statistic {op!r}: only mean, sum, var and std are implemented")
        if isinstance(ddof, bool) or int(ddof) != ddof or ddof < 0:
            raise ValueError(f"ddof must be an integer >= 0, got {ddof!r}")
        self._window, self._min_periods = check_window(window, min_periods)
        self._source, self._dim, self._op, self._center, self._ddof, self._wrap = source, dim, op, bool(center), int(ddof), bool(wrap)
        self._ctx, self._scratch_bytes = ctx, int(scratch_bytes)
        self.dims = tuple(source.dims)
        self.coords = dict(source.coords)
        self.name = source.name
        self.chunksizes = chunksizes

    def _like(self, source=None, chunksizes=None):
        return RolledGridArray(self._source if source is None else source, self._dim, self._window, self._op, self._center, self._min_periods,
                               self._ddof, self._wrap, self._ctx, self._scratch_bytes, chunksizes)

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        return dict(self._source.sizes)

    @property
    def source(self):
        return self._source

    @property
    def window(self):
        return self._window

    def chunk(self, chunks):
        return self._like(chunksizes=chunk_lengths(self.sizes, chunks))

    def unchunked(self):
        return self if self.chunksizes is None else self._like()

    def isel(self, **indexers):
        """slices along the other dims select from the source (the result stays lazy); a selection along the rolled dim is made on
        the computed field"""
        if self._dim in indexers:
            return self.compute().isel(**indexers)
        return self._like(source=self._source.isel(**indexers))

    # ---- the rolled field ----
    def _rest_dims(self):
        return tuple(d for d in self.dims if d != self._dim)

    def _row_dim(self):
        return self._dim

    def _field_order(self):
        return (self._dim,) + self._rest_dims()

    def device_field(self, ctx=None):
        """the field as a [T, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest).  The source is
        walked in blocks of time steps of at most ``scratch_bytes``, each with the steps its windows reach before and behind it; a
        window is evaluated from its own samples only, so the result does not depend on the block size.  ``wrap`` needs the whole
        axis in one block."""
        ctx = self._context(ctx)
        T = self._source.sizes[self._dim]
        back = window_back(self._window, self._center)
        with walk(self._source, self._dim, ctx, self._scratch_bytes, "rolling", halo=(back, self._window - 1 - back)) as w:
            out = w.result((T, w.cells))
            for r0, r1, block, b0 in w:
                if self._wrap and (r0, r1, block.shape[0]) != (0, T, T):
                    raise ValueError(f"wrap=True needs the {T} steps of dim {self._dim!r} in one block: scratch_bytes={self._scratch_bytes} "
                                     f"holds {block.shape[0]} of them; raise scratch_bytes")
                # the block holds every row a window of r0 .. r1 - 1 touches inside the array: clipping to the block is clipping to the array
                ctx.rolling(block, self._window, self._op, back, self._min_periods, self._ddof, self._wrap, t0=r0 - b0, n_out=r1 - r0,
                            out=out.rows(r0, r1))
        return out

    def __repr__(self):
        return (f"<RolledGridArray {self.sizes} {self._op} over {self._dim}={self._window} center={self._center} wrap={self._wrap} "
                f"computed={self.computed}>")
