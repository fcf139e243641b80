"""PiecewiseLinearRegression with the reference's surface (skdownscale/pointwise_models/arrm.py), computed by the HIP engine.

``fit_option='arrm'`` is deterministic: ``arrm_breakpoints`` (the breaks sit where the correlation of the two independently
sorted series over a sliding window is lowest) followed by one continuous piecewise-linear least-squares fit on those breaks,
which is what ``pwlf.PiecewiseLinFit.fit_with_breaks`` computes for degree 1.  Both run batched over the cell axis
(csrc/sd_arrm.hip, launch plan in csrc/sd_arrm_plan.h); one estimator is a grid of one cell.  ``pwlf`` is not needed.
``fit_option='auto'`` and ``'fast'`` are pwlf's stochastic optimisers (differential evolution, random multistart) and are not
offered.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, RegressorMixin
from sklearn.exceptions import NotFittedError
from sklearn.utils.validation import check_array, check_X_y

from . import _lib
from .base import check_sklearn_kwargs
from .engine import default_context

WINDOW_WIDTH = 0.05  # arrm.py:156
MIN_WIDTH = 10  # arrm.py:37
MIN_SAMPLES = 50
MAX_BREAKS = 16
# pwlf.PiecewiseLinFit keywords that cannot change the fitted model
PWLF_NEUTRAL = {"disp_res": None, "lapack_driver": None, "seed": None, "degree": (1,), "weights": (None,)}
EMPTY_RANGE_MESSAGE = "attempt to get argmin of an empty sequence"  # arrm.py:95, np.argmin(r2[:0])
STOCHASTIC = ("fit_option='{}' runs pwlf's stochastic optimiser ({}), which the HIP engine does not offer: use fit_option='arrm', "
              "the deterministic breakpoint search")


def check_max_features(array, n=1):
    """utils.py:10-25 of the reference"""
    if array.ndim == 1:
        pass
    elif array.ndim == 2:
        n_features = array.shape[1]
        if n_features > n:
            raise ValueError(f"Found array with {n_features} features (shape={array.shape}) while a maximum of {n} is required")
    else:
        raise ValueError(f"Found array with {array.ndim} dimensions. Unclear which should be the feature dim.")
    return array


def check_sizes(T, max_breakpoints):
    """what the engine supports (csrc/sd_arrm_plan.h): at least 50 samples, 2 .. 16 breaks"""
    if T < MIN_SAMPLES:
        raise ValueError(f"ARRM needs at least {MIN_SAMPLES} samples, got {T}: the first window would start before the series")
    B = 2 * (int(max_breakpoints) // 2)
    if not 2 <= B <= MAX_BREAKS:
        raise ValueError(f"max_breakpoints={max_breakpoints} gives {max(B, 0)} breaks, supported are 2 .. {MAX_BREAKS}")
    return B


def _python_round(v):
    return int(round(v))


class ArrmGridModel:
    """Batched ARRM fit over the cell axis: X, y [T, C] (numpy or DeviceArray), Xq [Tq, C]."""

    def __init__(self, max_breakpoints=7, ctx=None):
        self.ctx = ctx or default_context()
        self.max_breakpoints = int(max_breakpoints)
        self.state = None

    def fit(self, X, y, with_r2=False):
        check_sizes(X.shape[0], self.max_breakpoints)
        res = self.ctx.arrm_fit(X, y, self.max_breakpoints, with_r2=with_r2)
        self.state, self.r2_ = res if with_r2 else (res, None)
        self.status_ = self.state.status()
        # arrm.py:95: a cell whose smallest upper pick is 6 leaves r2[:0] for the lower picks, and the reference's np.argmin raises.
        # The per-cell loop stops at the first cell that fails: a non-finite cell before it is the caller's to report.
        empty = np.flatnonzero(self.status_ == _lib.CELL_EMPTY_RANGE)
        if len(empty) and not (self.status_[:empty[0]] == _lib.CELL_NONFINITE).any():
            self.state.close()
            self.state = None
            raise ValueError(EMPTY_RANGE_MESSAGE)
        return self

    def predict(self, Xq, out=None):
        if self.state is None:
            raise NotFittedError("This ARRM grid model is not fitted yet.")
        return self.ctx.arrm_predict(self.state, Xq, out=out)

    def export(self):
        return self.state.export()

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_export"] = self.export()
        d.pop("state", None)
        d.pop("ctx", None)
        return d

    def __setstate__(self, d):
        e = d.pop("_export")
        self.__dict__.update(d)
        self.ctx = default_context()
        self.state = self.ctx.arrm_import(e)


def arrm_breakpoints(X, y, window_width, max_breakpoints):
    """Calculate breakpoints in x and y (arrm.py:19-105): X [n, 1], y [n]; one cell through the engine.

    The engine's window is the reference's own ``window_width=0.05`` (``PiecewiseLinearRegression`` passes nothing else); a
    fraction that gives another window is refused.
    """
    X, y = np.asarray(X), np.asarray(y)
    n = len(X)
    if len(X) != len(y):
        raise ValueError(f"X and y must have the same length, got {len(X)} and {len(y)}")
    if X.shape[1] != 1:
        raise ValueError(f"X must have exactly 1 feature, got {X.shape[1]}")
    if max(_python_round(window_width * n), MIN_WIDTH) != max(_python_round(WINDOW_WIDTH * n), MIN_WIDTH):
        raise NotImplementedError(f"window_width={window_width}: the HIP engine computes the window of window_width={WINDOW_WIDTH}")
    grid = ArrmGridModel(max_breakpoints).fit(np.ascontiguousarray(X[:, :1], dtype=np.float64),
                                              np.ascontiguousarray(y, dtype=np.float64).reshape(n, 1))
    e = grid.export()
    if e["status"][0] != _lib.CELL_OK:
        raise ValueError("Input contains NaN.")
    return e["breaks"][:, 0]


class FittedPiecewiseModel:
    """``model_`` stand-in: the numbers of pwlf's fitted PiecewiseLinFit (degree 1)."""

    def __init__(self, fit_breaks, beta, ssr):
        self.fit_breaks = np.asarray(fit_breaks, dtype=np.float64)
        self.beta = np.asarray(beta, dtype=np.float64)
        self.n_segments = len(self.fit_breaks) - 1
        self.n_parameters = len(self.beta)
        self.ssr = float(ssr)

    def predict(self, x):
        x = np.asarray(x, dtype=np.float64)
        b = self.fit_breaks
        out = self.beta[0] + self.beta[1] * (x - b[0])
        for j in range(1, self.n_segments):
            out = out + self.beta[j + 1] * np.where(x > b[j], x - b[j], 0.0)
        return out


class PiecewiseLinearRegression(RegressorMixin, BaseEstimator):
    """Piecewise Linear Regression (arrm.py:108-177).

    Parameters
    ----------
    n_segments : int, default=7 -- with ``fit_option='arrm'`` the number of breaks is ``2 * (n_segments // 2)``
    fit_option : {"auto", "fast", "arrm"}, default='auto' -- only "arrm" runs here; "auto" and "fast" raise NotImplementedError
    pwlf_kwargs : dict, default=None -- keywords of ``pwlf.PiecewiseLinFit`` that do not change the model are accepted

    Attributes
    ----------
    fit_breaks_ : the breaks, ascending
    model_ : fit_breaks, beta, n_segments, n_parameters, ssr, predict(x)
    X_, y_ : the validated training data
    """

    _fit_attributes = ["model_", "fit_breaks_"]

    def __init__(self, n_segments=7, fit_option="auto", pwlf_kwargs=None):
        self.n_segments = n_segments
        self.fit_option = fit_option
        self.pwlf_kwargs = pwlf_kwargs

    def _check(self):
        check_sklearn_kwargs(self.pwlf_kwargs, PWLF_NEUTRAL, "pwlf_kwargs", "an unweighted continuous piecewise-linear fit of degree 1")
        if self.fit_option == "auto":
            raise NotImplementedError(STOCHASTIC.format("auto", "differential evolution"))
        if self.fit_option == "fast":
            raise NotImplementedError(STOCHASTIC.format("fast", "random multistart"))
        if self.fit_option != "arrm":
            raise ValueError(f"unsupported fit_option '{self.fit_option}'")

    def _adopt(self, e, c):
        """fitted attributes of cell ``c`` of an exported state (X_ and y_ are the caller's)"""
        self.fit_breaks_ = e["breaks"][:, c].copy()
        self.model_ = FittedPiecewiseModel(self.fit_breaks_, e["beta"][:, c], e["ssr"][c])
        self._break_index = e["break_index"][:, c].copy()
        self.n_features_in_ = 1
        self.__dict__.pop("_grid", None)

    def fit(self, X, y, **kwargs):
        X, y = check_X_y(X, y, y_numeric=True)
        X = check_max_features(X)
        self._check()
        if kwargs:
            raise TypeError(f"fit_with_breaks() got an unexpected keyword argument '{next(iter(kwargs))}'")
        T = X.shape[0]
        check_sizes(T, self.n_segments)
        grid = ArrmGridModel(self.n_segments).fit(np.ascontiguousarray(X[:, :1], dtype=np.float64),
                                                  np.ascontiguousarray(y, dtype=np.float64).reshape(T, 1))
        e = grid.export()
        if e["status"][0] != _lib.CELL_OK:  # (validation has refused non-finite input: nothing else may pass silently)
            raise ValueError(f"PiecewiseLinearRegression.fit: the engine reported status {int(e['status'][0])}")
        self._adopt(e, 0)
        self._grid = grid
        self.X_ = X
        self.y_ = y
        return self

    def _fitted_grid(self):
        if getattr(self, "_grid", None) is None:  # unpickled / rebuilt per cell: the device state from the fitted numbers
            m = self.model_
            B = len(m.beta)
            index = getattr(self, "_break_index", None)
            e = dict(breaks=m.fit_breaks.reshape(B, 1), beta=m.beta.reshape(B, 1), ssr=np.array([m.ssr]),
                     break_index=(np.full((B, 1), -1, np.int32) if index is None else np.asarray(index, np.int32).reshape(B, 1)),
                     status=np.zeros(1, np.int32), T=0 if getattr(self, "X_", None) is None else len(self.X_))
            grid = ArrmGridModel(self.n_segments)
            grid.state = grid.ctx.arrm_import(e)
            self._grid = grid
        return self._grid

    def predict(self, X):
        if not hasattr(self, "model_"):
            raise NotFittedError(f"This {type(self).__name__} instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 "using this estimator.")
        X = check_array(X)
        X = check_max_features(X)
        out, status = self._fitted_grid().predict(np.ascontiguousarray(X[:, :1], dtype=np.float64))
        if status[0] != _lib.CELL_OK:
            raise ValueError(f"PiecewiseLinearRegression.predict: the engine reported status {int(status[0])}")
        return out[:, 0]

    def __getstate__(self):
        d = dict(super().__getstate__())
        d.pop("_grid", None)
        return d
