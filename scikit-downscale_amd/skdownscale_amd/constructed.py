"""Constructed analogs on the GPU (Hidalgo et al. 2008; Maurer et al. 2010): the spatial operation under BCCA, MACA and LOCA, which the
reference's roadmap names as the missing family ("Other methods, like LOCA, MACA, BCCA, etc, should also be possible").

For each target day the k library days whose coarse pattern is closest are found, the target pattern is regressed on those k patterns,
and the k weights are applied to the fine fields of the same library days.  ``ConstructedAnalogs`` holds the two libraries (``fit``) and
makes the analogs and weights of a coarse target (``predict``); these touch coarse data only and run at once.  What ``predict`` returns,
a ``ConstructedGridArray``, is lazy: the fine field is synthesised in HBM when it is asked for -- whole through ``device_field``
(``compare``, ``quantile``, ``where`` take it from there), or block of target days by block with the fine library resident
(``resample``, ``groupby``, ``rolling``), so that neither the fine library nor the fine result crosses PCIe more than once.

The rule -- fixed-order float64 sums, ties to the earlier day -- is stated in include/sd_downscale.h and restated by
tests/_constructed_oracle.py.  LOCA's per-cell choice of analogs is ``LocalizedAnalogs`` (localized.py).  Out of scope: MACA's epoch
adjustment and multivariate patterns, the bias-correction step of BCCA (``BcsdTemperature`` on the coarse grid does it), cftime
calendars, more than 32 analogs and the sharded path.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _lib
from .core import DeferredGridArray, GridArray
from .remap import LATITUDE_NAMES
from .timesource import RowProducer, host_rows

KINDS = tuple(_lib.CA_KINDS)
WEIGHTS = ("area", "plain")
PERIOD = 366  # of the day-of-year keys


def _datetime_index(time, what):
    index = time if isinstance(time, pd.Index) else pd.Index(np.asarray(time))
    if not isinstance(index, pd.DatetimeIndex):
        raise ValueError(f"the time coordinate of {what} must be a DatetimeIndex, got {type(index).__name__} of {index.dtype} "
                         "(cftime calendars are not supported)")
    return index


def _first_difference(x, y):
    differ = np.asarray(x) != np.asarray(y)
    return int(np.flatnonzero(differ)[0]) if differ.any() else None


class ConstructedAnalogs:
    """``ConstructedAnalogs(n_analogs=30, window=45, kind='regression', ridge=1e-6, exclude_same_year=False, weights='area',
    latitude='auto')``.

    ``n_analogs``: k in [1, 32].  ``window``: a library day is a candidate when its day of year lies within that many days of the
    target's, across the year end (period 366); ``None``: every day is.  ``exclude_same_year``: library days of the target's own year
    are no candidates (a leave-one-year-out hindcast).  ``kind='regression'``: the weights solve the ridge-regularised least squares
    of the target pattern on the k library patterns, ``ridge`` times the mean diagonal of the Gram matrix added to it; ``'mean'``:
    1 / k each.  ``weights``: of the coarse cells in the distance and the regression -- ``'area'`` cos(lat) of the latitude dim
    (``latitude='auto'``: the one named ``lat`` / ``latitude``; or a dim name; without one: ones), ``'plain'`` ones, or an array of the
    coarse grid's shape.  Coarse columns that are NaN anywhere in the library (masked cells) or weigh 0 are left out.

    ``fit(coarse_library, fine_library)`` -- e.g. ``fit(obs.remap_like(gcm), obs)`` -- and ``predict(coarse_target)`` ->
    ``ConstructedGridArray``; ``analog_index_``, ``analog_distance_``, ``weights_`` [Tq, k] and ``status_`` [Tq] are those of the
    last ``predict``."""

    def __init__(self, n_analogs=30, window=45, kind="regression", ridge=1e-6, exclude_same_year=False, weights="area", latitude="auto",
                 dim="time", ctx=None):
        self.n_analogs = int(n_analogs)
        if not 1 <= self.n_analogs <= _lib.CA_MAX_ANALOGS:
            raise ValueError(f"n_analogs={n_analogs!r}: expected 1 to {_lib.CA_MAX_ANALOGS} analogs")
        if window is not None and (int(window) != window or window < 0):
            raise ValueError(f"window={window!r}: expected None or a number of days >= 0")
        self.window = None if window is None else int(window)
        if kind not in KINDS:
            raise ValueError(f"kind={kind!r}: expected one of {', '.join(repr(s) for s in KINDS)}")
        self.kind = kind
        self.ridge = float(ridge)
        if not (self.ridge >= 0.0 and np.isfinite(self.ridge)):
            raise ValueError(f"ridge={ridge!r}: expected a finite factor >= 0")
        self.exclude_same_year = bool(exclude_same_year)
        if isinstance(weights, str) and weights not in WEIGHTS:
            raise ValueError(f"weights={weights!r}: expected 'area', 'plain' or an array of the coarse grid's shape")
        self.weights, self.latitude, self.dim, self._ctx = weights, latitude, dim, ctx
        self._coarse = None

    # ---- fit ----
    def _column_weights(self, coarse, spatial):
        shape = tuple(coarse.sizes[d] for d in spatial)
        if not isinstance(self.weights, str):
            wc = np.asarray(self.weights, dtype=np.float64)
            if wc.shape != shape and wc.shape != (int(np.prod(shape)),):
                raise ValueError(f"weights: expected an array of the coarse grid's shape {shape}, got shape {wc.shape}")
            if not (np.isfinite(wc).all() and (wc >= 0).all()):
                raise ValueError("weights: expected finite weights >= 0")
            return np.ascontiguousarray(wc.reshape(-1))
        lat = self.latitude
        if lat == "auto":
            named = [d for d in spatial if d in LATITUDE_NAMES]
            lat = named[0] if named else None
        elif lat is not None and lat not in spatial:
            raise ValueError(f"latitude={lat!r} is not one of the spatial dims {spatial}")
        wc = np.ones(shape)
        if self.weights == "area" and lat is not None:
            if lat not in coarse.coords:
                raise ValueError(f"the coarse library has no coordinate for dim {lat!r}")
            w = np.cos(np.deg2rad(np.clip(np.asarray(coarse.coords[lat], dtype=np.float64), -90.0, 90.0)))
            wc = wc * np.maximum(w, 0.0).reshape([-1 if d == lat else 1 for d in spatial])
        return np.ascontiguousarray(wc.reshape(-1))

    def fit(self, coarse, fine):
        dim = self.dim
        for name, a in (("coarse library", coarse), ("fine library", fine)):
            if not isinstance(a, GridArray):
                raise ValueError(f"the {name}: expected a GridArray, got {type(a).__name__}")
            if dim not in a.dims:
                raise ValueError(f"dim {dim!r} is not a dim of the {name} {a.dims}")
            if len(a.dims) < 2:
                raise ValueError(f"the {name} has no spatial dim beside {dim!r}: {a.dims}")
            if dim not in a.coords:
                raise ValueError(f"the {name} has no coordinate for dim {dim!r}")
        if coarse.sizes[dim] != fine.sizes[dim]:
            raise ValueError(f"the libraries differ: {coarse.sizes[dim]} coarse and {fine.sizes[dim]} fine steps of {dim!r} (nothing is aligned)")
        if coarse.sizes[dim] == 0 or min(coarse.sizes.values()) == 0 or min(fine.sizes.values()) == 0:
            raise ValueError(f"nothing to fit: the libraries have sizes {coarse.sizes} and {fine.sizes}")
        time = _datetime_index(coarse.coords[dim], "the coarse library")
        at = _first_difference(time, _datetime_index(fine.coords[dim], "the fine library"))
        if at is not None:
            raise ValueError(f"the {dim} coordinates of the libraries differ at step {at}: {time[at]} and {fine.coords[dim][at]} "
                             "(nothing is aligned)")
        if time.hasnans:
            raise ValueError(f"the {dim} coordinate of the libraries holds NaT")
        spatial = tuple(d for d in coarse.dims if d != dim)
        self._wc = self._column_weights(coarse, spatial)
        self._L = np.ascontiguousarray(host_rows(coarse, dim), dtype=np.float64)  # (a lazy coarse library is computed here)
        self._coarse = dict(dims=spatial, sizes={d: coarse.sizes[d] for d in spatial})
        self._fine, self._time = fine, time
        return self

    # ---- predict ----
    def _coarse_target(self, target):
        """the checks of a target -> (its time index, Q [Tq, Cc] in the library's column order, key_l, key_q, excl_l, excl_q)"""
        if self._coarse is None:
            raise ValueError(f"this {type(self).__name__} is not fitted: call fit(coarse_library, fine_library) first")
        dim, spatial = self.dim, self._coarse["dims"]
        if not isinstance(target, GridArray):
            raise ValueError(f"the target: expected a GridArray, got {type(target).__name__}")
        if set(target.dims) != {dim, *spatial} or len(target.dims) != len(spatial) + 1:
            raise ValueError(f"the target has dims {target.dims}; expected {(dim,) + spatial} in any order")
        sizes = {d: target.sizes[d] for d in spatial}
        if sizes != self._coarse["sizes"]:
            raise ValueError(f"the target has sizes {sizes} on the coarse grid; the coarse library has {self._coarse['sizes']}")
        if dim not in target.coords:
            raise ValueError(f"the target has no coordinate for dim {dim!r}")
        tq = _datetime_index(target.coords[dim], "the target")
        if len(tq) == 0:
            raise ValueError(f"nothing to predict: dim {dim!r} has length 0")
        if tq.hasnans:
            raise ValueError(f"the {dim} coordinate of the target holds NaT")
        order = (dim,) + spatial
        Q = np.ascontiguousarray(host_rows(target if tuple(target.dims) == order else target.transpose(*order), dim), dtype=np.float64)
        key_l, key_q = self._time.dayofyear.to_numpy().astype(np.int32), tq.dayofyear.to_numpy().astype(np.int32)
        excl_l = self._time.year.to_numpy().astype(np.int32) if self.exclude_same_year else None
        excl_q = tq.year.to_numpy().astype(np.int32) if self.exclude_same_year else None
        return tq, Q, key_l, key_q, excl_l, excl_q

    def _few_candidates(self, status, tq):
        few = np.flatnonzero(status == _lib.CA_FEW_CANDIDATES)
        if len(few):
            q = int(few[0])
            raise ValueError(f"step {q} of the target ({tq[q]}) has fewer than n_analogs={self.n_analogs} candidate days in the library "
                             f"(window={self.window}, exclude_same_year={self.exclude_same_year})")

    def predict(self, target, ctx=None):
        tq, Q, key_l, key_q, excl_l, excl_q = self._coarse_target(target)
        dim, k = self.dim, self.n_analogs
        if ctx is None:
            from .engine import default_context

            ctx = self._ctx or default_context()
        made = []
        try:
            made.append(ctx.to_device(self._L))
            made.append(ctx.to_device(Q))
            Ld, Qd = made
            tables = ctx.ca_select(Ld, Qd, self._wc, k, key_l, key_q, PERIOD, -1 if self.window is None else self.window, excl_l, excl_q)
            made.extend(tables)
            made.append(ctx.ca_weights(Ld, Qd, self._wc, *tables, kind=self.kind, ridge=self.ridge))
            idx, dist, status, weights = (a.to_host() for a in made[2:])
        finally:
            for a in made:
                a.free()
        self.analog_index_, self.analog_distance_, self.weights_, self.status_ = idx, dist, weights, status
        self._few_candidates(status, tq)
        singular = np.flatnonzero(status == _lib.CA_SINGULAR)
        if len(singular):
            q = int(singular[0])
            raise ArithmeticError(f"step {q} of the target ({tq[q]}): the Gram matrix of its {k} analogs is not positive definite "
                                  f"with ridge={self.ridge:g} (duplicate library days?); raise ridge")
        return ConstructedGridArray(self._fine, dim, tq, idx, weights, ctx=self._ctx if ctx is None else ctx, name=target.name)


class ConstructedGridArray(DeferredGridArray):
    """The fine field of a constructed-analog prediction, [target days, *fine cells]: ``out[q] = sum_i weights[q, i] * fine[idx[q, i]]``
    in analog order.  It keeps the fine library and the two [Tq, k] tables; a target day whose first index is -1 (a non-finite
    target pattern) is a NaN row."""

    _kind = "constructed"

    def __init__(self, fine, dim, time, idx, weights, ctx=None, name=None):
        self._fine, self._dim = fine, dim
        self._idx, self._weights = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(weights, dtype=np.float64)
        self._ctx = ctx
        self._spatial = tuple(d for d in fine.dims if d != dim)
        self.dims = (dim,) + self._spatial
        self.coords = {k: v for k, v in fine.coords.items() if k != dim}
        self.coords[dim] = time
        self.name = name if name is not None else fine.name

    @property
    def sizes(self):
        s = {self._dim: len(self._idx)}
        s.update({d: self._fine.sizes[d] for d in self._spatial})
        return s

    @property
    def analog_index(self):
        return self._idx

    @property
    def analog_weights(self):
        return self._weights

    def unchunked(self):
        return self

    def isel(self, **indexers):
        """slices stay lazy: along the spatial dims they select cells of the fine library, along the time dim rows of the tables"""
        unknown = [d for d in indexers if d not in self.dims]
        if unknown:
            raise ValueError(f"dim {unknown[0]!r} is not a dim of this array {self.dims}")
        if not all(isinstance(s, slice) for s in indexers.values()):
            return self.compute().isel(**indexers)
        rows = indexers.get(self._dim, slice(None))
        fine = self._fine.isel(**{d: s for d, s in indexers.items() if d != self._dim})
        return ConstructedGridArray(fine, self._dim, self.coords[self._dim][rows], self._idx[rows], self._weights[rows], self._ctx, self.name)

    # ---- the fine field ----
    def _row_dim(self):
        return self._dim

    def _field_order(self):
        return self.dims

    def _library(self, ctx):
        """the fine library as a [Tl, Cf] DeviceArray, float32 as float32, and the two tables"""
        rows = host_rows(self._fine, self._dim)
        if min(rows.shape) < 1 or len(self._idx) < 1:
            raise ValueError(f"nothing to construct: the array has sizes {self.sizes}")
        made = []
        try:
            made.append(ctx.to_device(rows, rows.dtype))
            made.append(ctx.to_device(self._idx, np.int32))
            made.append(ctx.to_device(self._weights))
        except BaseException:
            for a in made:
                a.free()
            raise
        return made

    def device_field(self, ctx=None):
        """the whole fine field as a [Tq, Cf] float64 DeviceArray (the cells of the fine dims in their order, the last fastest)"""
        ctx = self._context(ctx)
        made = self._library(ctx)
        try:
            return ctx.ca_apply(*made)
        finally:
            for a in made:
                a.free()

    def _block_producer(self, ctx, dim):
        """rows [r0, r1) of the fine field with the fine library resident: it goes up once, when the first block is asked for"""
        if self.computed or dim != self._dim:
            return None
        cells = int(np.prod([self._fine.sizes[d] for d in self._spatial], dtype=np.int64))
        resident = []

        def produce(r0, r1, out):
            if not resident:
                resident.extend(self._library(ctx))
            return ctx.ca_apply(*resident, q0=r0, q1=r1, out=out)

        return RowProducer(len(self._idx), cells, np.dtype(np.float64), produce, False)

    def __repr__(self):
        return f"<ConstructedGridArray {self.sizes} from {self._idx.shape[1]} analogs of {self._fine.sizes} computed={self.computed}>"
