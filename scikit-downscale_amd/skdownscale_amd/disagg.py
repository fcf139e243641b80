"""Temporal disaggregation on the GPU: the last step of BCSD (Wood et al. 2004; the reference's driver ends with it,
``scripts/run_bcsd.py``: ``disagg(ds_obs_daily[obs_var], anoms[obs_var], var=obs_var)``).  Every downscaled month becomes daily weather
by borrowing the daily pattern of a historical month of the same calendar month from the observations and shifting it (temperature) or
scaling it (precipitation) so that its monthly statistic equals the downscaled value.  Every cell borrows the same historical month, so
the weather stays spatially coherent.

``time_map`` makes the calendar -- it is the only place that touches pandas --, ``DisaggregatedGridArray`` is what
``GridArray.disaggregate`` returns: the monthly field, the observations and the row map, computed when the field is asked for -- on the
host through ``values`` (block by block: the device holds the observations and one block), or as a ``[Tout, C]`` ``DeviceArray``
through ``device_field``.

The rule, per output month and cell, with ``x_t`` the borrowed samples in time order, ``acc`` their plain sum without the NaN ones and
``cnt`` the number of those: ``shift`` gives ``x_t + (tgt - acc / cnt)``; ``scale`` with ``stat='mean'`` gives ``x_t * (tgt / (acc /
cnt))``, with ``stat='sum'`` ``x_t * (tgt / acc)``; a dry borrowed month (statistic 0) gives every non-NaN day ``tgt`` (mean) or ``tgt /
cnt`` (sum).  A NaN sample stays NaN; a month without a sample and a month with a NaN target are NaN.  The result is float64.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _lib
from .core import DeferredGridArray, GridArray
from .resample import DEFAULT_SCRATCH_BYTES
from .timesource import _bin_blocks, takes_whole

KINDS = ("shift", "scale")


def _datetime_index(time, what):
    index = time if isinstance(time, pd.Index) else pd.Index(np.asarray(time))
    if not isinstance(index, pd.DatetimeIndex):
        raise ValueError(f"the {what} time coordinate must be a DatetimeIndex, got {type(index).__name__} of {index.dtype} "
                         "(cftime calendars are not supported)")
    return index


def time_map(monthly_time, daily_time, years=None, seed=0):
    """The calendar of a disaggregation: ``(out_time, src_row, offsets)``.  ``out_time`` holds all calendar days of every labelled month
    of ``monthly_time`` (``Tout`` entries; the day within the month of a label is ignored, gaps between months are allowed), ``offsets``
    int64 ``[M + 1]`` the rows of each month in it, and ``src_row`` int64 ``[Tout]`` the position in ``daily_time`` every output day
    borrows.  A month (year, month) of ``daily_time`` is eligible as a source if ``daily_time`` holds every calendar day of it exactly
    once.  ``years`` chooses the source year of every output month: ``None`` draws with ``np.random.default_rng(seed).choice`` among
    the eligible years of that calendar month, one draw per output month, in order; an int array ``[M]`` is taken as given;
    ``'same'`` takes the label's own year.  Output day ``d`` borrows source day ``min(d, n_src - 1)``: a 29-day month on a 28-day
    source repeats the last day, a 28-day month on a 29-day source drops it."""
    monthly, daily = _datetime_index(monthly_time, "monthly"), _datetime_index(daily_time, "daily")
    M = len(monthly)
    if M == 0 or len(daily) == 0:
        raise ValueError(f"nothing to disaggregate: {M} months, {len(daily)} daily samples")
    dv = daily.asi8
    back = np.flatnonzero(dv[1:] <= dv[:-1])
    if len(back) or daily.hasnans:
        i = int(back[0]) + 1 if len(back) else int(np.flatnonzero(daily.isna())[0])
        raise ValueError(f"the daily time coordinate is not strictly increasing at position {i} ({daily[i]})")
    if monthly.hasnans:
        raise ValueError("the monthly time coordinate holds NaT")
    mkey = monthly.year.to_numpy().astype(np.int64) * 12 + (monthly.month.to_numpy() - 1)
    back = np.flatnonzero(mkey[1:] <= mkey[:-1])
    if len(back):
        i = int(back[0]) + 1
        raise ValueError(f"the monthly labels must have strictly increasing (year, month): position {i} ({monthly[i]}) does not lie "
                         f"after position {i - 1} ({monthly[i - 1]})")
    # the eligible source months: (year, month) -> first row, for the months whose days are exactly 1 .. days_in_month
    dkey = daily.year.to_numpy().astype(np.int64) * 12 + (daily.month.to_numpy() - 1)
    day, dim = daily.day.to_numpy(), daily.days_in_month.to_numpy()
    starts = np.concatenate([[0], np.flatnonzero(np.diff(dkey)) + 1, [len(daily)]])
    first_row, length = {}, {}
    for a, b in zip(starts[:-1], starts[1:]):
        if b - a == dim[a] and np.array_equal(day[a:b], np.arange(1, b - a + 1)):
            first_row[int(dkey[a])], length[int(dkey[a])] = int(a), int(b - a)
    eligible = {mo: np.array(sorted(k // 12 for k in first_row if k % 12 == mo), dtype=np.int64) for mo in range(12)}

    if years is None:
        rng = np.random.default_rng(seed)
        chosen = []
        for i in range(M):
            pool = eligible[int(mkey[i] % 12)]
            if len(pool) == 0:
                raise ValueError(f"the observations hold no complete month to borrow for {monthly[i]:%Y-%m}")
            chosen.append(int(rng.choice(pool)))
        chosen = np.array(chosen, dtype=np.int64)
    elif isinstance(years, str):
        if years != "same":
            raise ValueError(f"years={years!r}: expected None, 'same' or one year per month")
        chosen = mkey // 12
    else:
        chosen = np.asarray(years)
        if chosen.shape != (M,) or not np.issubdtype(chosen.dtype, np.integer):
            raise ValueError(f"years: expected {M} integer years, one per month, got shape {chosen.shape} of {chosen.dtype}")
        chosen = chosen.astype(np.int64)
    n_out = monthly.days_in_month.to_numpy().astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    src_row = np.empty(int(offsets[-1]), dtype=np.int64)
    for i in range(M):
        key = int(chosen[i] * 12 + mkey[i] % 12)
        if key not in first_row:
            raise ValueError(f"the observations do not hold every day of {int(chosen[i]):04d}-{int(mkey[i] % 12) + 1:02d} exactly once: it "
                             f"cannot be borrowed for {monthly[i]:%Y-%m}")
        src_row[offsets[i]:offsets[i + 1]] = first_row[key] + np.minimum(np.arange(n_out[i]), length[key] - 1)
    wall = monthly if monthly.tz is None else monthly.tz_localize(None)  # (days are counted on the wall clock)
    first_day = (wall.normalize() - pd.to_timedelta(wall.day.to_numpy() - 1, unit="D")).to_numpy().astype("datetime64[D]")
    out_time = pd.DatetimeIndex(np.concatenate([first_day[i] + np.arange(n_out[i]) for i in range(M)]).astype("datetime64[ns]"))
    return (out_time if monthly.tz is None else out_time.tz_localize(monthly.tz)), src_row, offsets


def disagg_op(kind, stat=None):
    """the engine's op of ``GridArray.disaggregate(kind=, stat=)``"""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: expected 'shift' or 'scale'")
    if kind == "shift":
        if stat not in (None, "mean"):
            raise ValueError(f"kind='shift' matches the monthly mean; stat={stat!r} is not offered")
        return "shift"
    if stat not in ("mean", "sum"):
        raise ValueError(f"kind='scale' needs stat='mean' or stat='sum' (the statistic the monthly field holds), got stat={stat!r}")
    return "scale_" + stat


class DisaggregatedGridArray(DeferredGridArray):
    """A monthly ``GridArray`` turned into daily weather: same dims, ``dim`` at the number of days of the labelled months with the
    daily coordinate."""

    _kind = "disagg"

    def __init__(self, monthly, daily_obs, dim="time", kind="shift", stat=None, years=None, seed=0, climatology=None, ctx=None,
                 scratch_bytes=DEFAULT_SCRATCH_BYTES):
        self._op = disagg_op(kind, stat)
        if not isinstance(daily_obs, GridArray):
            raise ValueError(f"daily_obs: expected a GridArray, got {type(daily_obs).__name__}")
        for name, a in (("this array", monthly), ("daily_obs", daily_obs)):
            if dim not in a.dims:
                raise ValueError(f"dim {dim!r} is not a dim of {name} {a.dims}")
            if dim not in a.coords:
                raise ValueError(f"{name} has no coordinate for dim {dim!r}")
        rest = tuple(d for d in monthly.dims if d != dim)
        if set(daily_obs.dims) != {dim, *rest} or any(daily_obs.sizes[d] != monthly.sizes[d] for d in rest):
            raise ValueError(f"daily_obs has sizes {daily_obs.sizes}; expected the dims {rest} of this array at its sizes "
                             f"{ {d: monthly.sizes[d] for d in rest} } and {dim!r}")
        self._monthly, self._obs, self._dim, self._rest = monthly, daily_obs, dim, rest
        self._ctx, self._scratch_bytes = ctx, int(scratch_bytes)
        self._time, self._src_row, self._offsets = time_map(monthly.coords[dim], daily_obs.coords[dim], years, seed)
        self._climo = self._group = None
        if climatology is not None:
            shape = (12,) + tuple(monthly.sizes[d] for d in rest)
            if isinstance(climatology, GridArray):
                lead = [d for d in climatology.dims if d not in rest]
                if len(lead) != 1 or set(climatology.dims) != {lead[0], *rest}:
                    raise ValueError(f"climatology has dims {climatology.dims}; expected a month dim and {rest}")
                climatology = climatology.transpose(lead[0], *rest).values
            c = np.asarray(climatology, dtype=np.float64)
            if c.shape != shape:
                raise ValueError(f"climatology has shape {c.shape}; expected {shape}: one field per calendar month")
            self._climo = np.ascontiguousarray(c).reshape(12, -1)
            self._group = (_datetime_index(monthly.coords[dim], "monthly").month.to_numpy() - 1).astype(np.int32)
        self.dims = tuple(monthly.dims)
        self.coords = dict(monthly.coords)
        self.coords[dim] = self._time
        self.name = monthly.name

    # ---- the GridArray surface ----
    @property
    def sizes(self):
        s = dict(self._monthly.sizes)
        s[self._dim] = len(self._time)
        return s

    @property
    def src_row(self):
        return self._src_row

    @property
    def offsets(self):
        return self._offsets

    # ---- the daily field ----
    def _obs_rows(self):
        """the observations as a host [To, C] array in this array's cell order; float32 stays float32"""
        order = (self._dim,) + self._rest
        src = self._obs if tuple(self._obs.dims) == order else self._obs.transpose(*order)
        v = _lib.as_field(src.values)
        return v.reshape(v.shape[0], -1)

    def _target(self, ctx):
        """the monthly field as an [M, C] float64 DeviceArray: a resampled field in this order is reduced in HBM, any other goes up once"""
        order = (self._dim,) + self._rest
        m = self._monthly
        if takes_whole(m, "target", self._dim) and tuple(m.dims) == order:
            return m.device_field(ctx)
        v = _lib.as_f64((m if tuple(m.dims) == order else m.transpose(*order)).values)
        return ctx.to_device(v.reshape(v.shape[0], -1))

    def _row_dim(self):
        return self._dim

    def _make(self, ctx, to_host):
        """the daily field, made in blocks of whole months of at most ``scratch_bytes`` of output: as a [Tout, C] DeviceArray, or with
        ``to_host`` through one block of device scratch as a host array.  A month is always made within one block by the same lane:
        the result does not depend on the block size."""
        off, M, Tout = self._offsets, len(self._offsets) - 1, len(self._time)
        obs = self._obs_rows()
        C = obs.shape[1]
        if C < 1:
            raise ValueError(f"nothing to disaggregate: the array has sizes {self._monthly.sizes}")
        blocks = [(a, b, int(off[a]), int(off[b])) for a, b in _bin_blocks(off, max(1, self._scratch_bytes // (C * 8)))]
        d_obs = target = climo = out = None
        kept = False
        try:
            d_obs = ctx.to_device(obs, obs.dtype)
            target = self._target(ctx)
            assert target.shape == (M, C), (target.shape, M, C)
            climo = None if self._climo is None else ctx.to_device(self._climo)
            out = ctx.empty((max(r1 - r0 for _, _, r0, r1 in blocks) if to_host else Tout, C))
            host = np.empty((Tout, C)) if to_host else None
            for a, b, r0, r1 in blocks:
                block = out.rows(0, r1 - r0) if to_host else out.rows(r0, r1)
                ctx.disaggregate(target.rows(a, b), d_obs, self._src_row[r0:r1], off[a:b + 1] - r0, self._op, climo,
                                 None if climo is None else self._group[a:b], out=block)
                if to_host:
                    host[r0:r1] = block.to_host()
            kept = not to_host
            return host if to_host else out
        finally:
            for d in (d_obs, target, climo, None if kept else out):
                if d is not None:
                    d.free()

    def device_field(self, ctx=None):
        """the daily field as a [Tout, C] float64 DeviceArray (C = cells of the other dims in their order, the last fastest)"""
        return self._make(self._context(ctx), False)

    def _compute_values(self):
        return self._in_dims(self._make(self._context(), True), (self._dim,) + self._rest)

    def __repr__(self):
        return (f"<DisaggregatedGridArray {self.sizes} {self._op} of {self._monthly.sizes} on {self._obs.sizes} "
                f"computed={self.computed}>")
