"""ZScoreRegressor with the reference's surface (skdownscale/pointwise_models/zscore.py), computed by the HIP engine.

fit: the mean and population std of X and of y over centred day-of-year windows pooled across the years
(zscore.py:123-189), shift_ = y_mean - X_mean, scale_ = y_std / X_std (zscore.py:237-238).  predict: pandas' centred rolling
mean / std (ddof = 1) of the future series, its z score, and the fitted parameters expanded by position over the series
(zscore.py:241-354).  Both passes are batched over the cell axis (csrc/sd_zscore.hip, the day-window plan in
csrc/sd_zscore_plan.h); one estimator is a grid of one cell.  No xarray is needed: the day-of-year grid is built from the
pandas DatetimeIndex directly.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from sklearn.exceptions import NotFittedError

from . import _lib
from .base import TimeSynchronousDownscaler
from .engine import default_context

DT_ACCESSOR_MESSAGE = ".dt accessor only available for DataArray with datetime64 timedelta64 dtype or for arrays containing cftime datetime objects."
EXPAND_MESSAGE = "positional indexers are out-of-bounds"


def day_grid(index):
    """(labels [D], day_idx [T], year [T]) of a time index: the sorted days of year that occur, each sample's position among
    them and its year (zscore.py:145-151: the yearly groups re-labelled by day of year and aligned on their union)."""
    if not isinstance(index, pd.DatetimeIndex):
        raise AttributeError(DT_ACCESSOR_MESSAGE)
    labels, day_idx = np.unique(np.asarray(index.dayofyear, dtype=np.int64), return_inverse=True)
    return labels, day_idx.astype(np.int32).ravel(), np.asarray(index.year, dtype=np.int32)


def kept_labels(labels, window_width):
    """day-of-year labels of the kept windows (zscore.py:155-159, 185-189): the positions n .. L-n-1 of the extended day axis
    M[-ceil(w/2):] ++ M ++ M[:w/2], n = w // 2 + 1 (the rule of csrc/sd_zscore_plan.h)"""
    w = int(window_width)
    ext = np.concatenate([labels[-((w + 1) // 2):], labels, labels[:w // 2]])
    n = w // 2 + 1
    return ext[n:len(ext) - n]


class ZScoreGridModel:
    """Batched ZScoreRegressor over the cell axis: X, y [T, C] (numpy or DeviceArray) on one time index, Xp [Tp, C]."""

    def __init__(self, window_width=31, ctx=None):
        self.ctx = ctx or default_context()
        self.window_width = int(window_width)
        self.state = None

    def fit(self, X, y, index):
        labels, day_idx, year = day_grid(index)
        self.state = self.ctx.zscore_fit(X, y, self.window_width, day_idx, year, len(labels))
        self.labels_ = kept_labels(labels, self.window_width)
        self.status_ = self.state.status()
        return self

    def check_expand(self, Tp):
        """zscore.py:300-313: the parameters are read at positions t % min(Tp, 364); pandas raises past the fitted entries"""
        if min(int(Tp), 364) > len(self.labels_):
            raise IndexError(EXPAND_MESSAGE)

    def predict(self, Xp, out=None, with_stats=False):
        if self.state is None:
            raise NotFittedError("This ZScore grid model is not fitted yet.")
        self.check_expand(Xp.shape[0])
        return self.ctx.zscore_predict(self.state, Xp, out=out, with_stats=with_stats)

    def export(self):
        e = self.state.export()
        e["labels"] = self.labels_
        return e

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
        self.state = self.ctx.zscore_import(e)


def _series(values, labels, name):
    return pd.Series(np.asarray(values, dtype=np.float64), index=pd.Index(np.asarray(labels, dtype=np.int64), name="day"), name=name)


class ZScoreRegressor(TimeSynchronousDownscaler):
    """Z Score Regressor bias correction (zscore.py:11-121).

    Parameters
    ----------
    window_width : int -- width of the centred day window of fit and of the rolling window of predict (default 31)

    Attributes
    ----------
    shift_, scale_ : pd.Series over the kept day-of-year labels
    fit_stats_dict_ : X_mean, X_std, y_mean, y_std (pd.Series, same index)
    predict_stats_dict_ : meani, stdi, meanf, stdf of the last predict (pd.Series on its index)
    """

    _fit_attributes = ["shift_", "scale_"]
    _timestep = "M"

    def __init__(self, window_width: int = 31) -> None:
        if window_width <= 0:
            raise ValueError(f"window_width must be positive, got {window_width}")
        self.window_width = window_width

    def _adopt(self, e, c, labels, names=(0, 0)):
        """fitted attributes of cell ``c`` of an exported state"""
        xn, yn = names
        st = {"X_mean": _series(e["x_mean"][:, c], labels, xn), "X_std": _series(e["x_std"][:, c], labels, xn),
              "y_mean": _series(e["y_mean"][:, c], labels, yn), "y_std": _series(e["y_std"][:, c], labels, yn)}
        self.fit_stats_dict_ = st
        self.shift_ = _series(e["shift"][:, c], labels, xn if xn == yn else None)
        self.scale_ = _series(e["scale"][:, c], labels, xn if xn == yn else None)
        self.n_features_in_ = 1

    def fit(self, X, y):
        X2, y2, index = self._check_X_y(X, y)
        if self.n_features_in_ != 1:
            raise ValueError(f"Zscore only supports 1 feature, found {self.n_features_in_}")
        if len(X2) == 1:  # X.squeeze() of one sample is a scalar (zscore.py:51-52)
            raise TypeError("X.squeeze() must be a pd.Series, got float64")
        if y2.shape[1] != 1:
            raise TypeError("y.squeeze() must be a pd.Series, got DataFrame")
        if index.name not in (None, "time", "index"):  # Series.to_xarray names the coordinate after the index (zscore.py:141-144)
            raise ValueError('Input array must have a "time" coordinate')
        day_grid(index)  # (a time index without dates fails here, before the engine is reached)
        names = (X.columns[0] if isinstance(X, pd.DataFrame) else 0, y.columns[0] if isinstance(y, pd.DataFrame) else 0)
        grid = ZScoreGridModel(self.window_width).fit(np.ascontiguousarray(X2[:, :1]), np.ascontiguousarray(y2[:, :1]), index)
        e = grid.export()
        if e["status"][0] != _lib.CELL_OK:  # (validation has refused non-finite input: nothing else may pass silently)
            raise ValueError(f"ZScoreRegressor.fit: the engine reported status {int(e['status'][0])}")
        self._adopt(e, 0, grid.labels_, names)
        self._grid = grid
        return self

    def _fitted_grid(self):
        if getattr(self, "_grid", None) is None:  # unpickled / rebuilt per cell: the device state from the fitted numbers
            K = len(self.shift_)
            st = getattr(self, "fit_stats_dict_", None) or {k: np.full(K, np.nan) for k in ("X_mean", "X_std", "y_mean", "y_std")}
            e = dict(x_mean=np.asarray(st["X_mean"]), x_std=np.asarray(st["X_std"]), y_mean=np.asarray(st["y_mean"]),
                     y_std=np.asarray(st["y_std"]), shift=np.asarray(self.shift_), scale=np.asarray(self.scale_))
            e = {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 1) for k, v in e.items()}
            grid = ZScoreGridModel(self.window_width)
            grid.state = grid.ctx.zscore_import(dict(e, status=np.zeros(1, np.int32), window_width=self.window_width))
            grid.labels_ = np.asarray(self.shift_.index)
            self._grid = grid
        return self._grid

    def predict(self, X):
        if not hasattr(self, "shift_"):
            raise NotFittedError(f"This {type(self).__name__} instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 "using this estimator.")
        X2, index = self._check_array(X, reset_features=True)
        if X2.shape[1] != 1:
            raise ValueError(f"X must have exactly 1 feature, got {X2.shape[1]}")
        name = X.columns[0] if isinstance(X, pd.DataFrame) else 0
        out, status, stats = self._fitted_grid().predict(np.ascontiguousarray(X2), with_stats=True)
        if status[0] != _lib.CELL_OK:
            raise ValueError(f"ZScoreRegressor.predict: the engine reported status {int(status[0])}")
        self.predict_stats_dict_ = {k: pd.Series(v[:, 0], index=index, name=name) for k, v in stats.items()}
        return pd.DataFrame({name: out[:, 0]}, index=index)

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_grid", None)
        return d

    def __sklearn_tags__(self):
        from dataclasses import replace

        tags = super().__sklearn_tags__()
        return replace(tags, _skip_test="ZScore only supports 1 feature and temporal order matters")
