"""GroupedRegressor and its day-of-year grouper with the reference's surface (skdownscale/pointwise_models/grouping.py).

``GroupedRegressor(LinearRegression, PaddedDOYGrouper, predict_grouper, fit_grouper_kwargs={"window": w})`` fits one
least-squares model per day of year on the samples within +-w days of it and predicts every sample with the model of its own
day: a seasonally varying regression.  The reference runs one sklearn fit and one predict per group; here all groups of all
cells are fitted by two kernels that read X and y once and predicted by one (csrc/sd_grouped.hip).  The same kernels fit
disjoint groups (window 0: one model per month, per season, ...).  Any other estimator or grouping of a single series runs
the reference's loop over the groups on the host, calling the estimator that was given.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from sklearn.exceptions import NotFittedError

from . import _lib
from .base import LINEAR_NEUTRAL, _finite_error, check_sklearn_kwargs
from .engine import default_context
from .groupers import group_keys

NO_SAMPLES_MESSAGE = "Found array with 0 sample(s) (shape=(0, {F})) while a minimum of 1 is required by LinearRegression."
SUPPORTED = ("the HIP engine batches estimator=sklearn.linear_model.LinearRegression (or 'LinearRegression') with default "
             "estimator_kwargs and fit_grouper=grouping.PaddedDOYGrouper or a grouper whose .groups are disjoint and cover the index")


def doy_keys(index):
    """(key [T] in [0, n), n) of a time index for the engine: day of year - 1 and the largest day of year (grouping.py:122-123:
    one calendar for all years)"""
    doy = np.asarray(index.dayofyear, dtype=np.int64)
    return (doy - 1).astype(np.int32), int(doy.max())


def check_window(window, n):
    """the reference wraps its window once (grouping.py:128-130): window >= n indexes outside the calendar there"""
    if not 0 <= int(window) < n:
        raise ValueError(f"window={window} must lie in [0, {n}): the day-of-year window wraps around the calendar once only")
    return int(window)


class PaddedDOYGrouper:
    """Grouper to group an Index by day-of-year +/- pad (grouping.py:106-138): ``groups`` maps every day of year
    1 .. n = index.dayofyear.max() to the positions of the samples whose day of year lies within ``window`` days of it on a
    circular calendar of n days (one calendar for all years), every sample at most once per group.

    Not the ``PaddedDOYGrouper`` of ``groupers.py`` (leap / non-leap calendars, used by BCSD): that one keeps the top-level name.
    """

    def __init__(self, index: pd.DatetimeIndex, window: int) -> None:
        self.index = index
        self.window = window
        key, n = doy_keys(index)
        w = check_window(window, n)
        dist = np.abs(np.arange(n, dtype=np.int64)[:, None] - key[None, :])
        member = np.minimum(dist, n - dist) <= w  # [n, T]
        self._groups = {doy: np.nonzero(member[doy - 1])[0] for doy in range(1, n + 1)}

    @property
    def groups(self):
        """Dict {doy -> group indicies}."""
        return self._groups


class GroupedGridModel:
    """Batched grouped linear regression over the cell axis: X [T, F, C], y [T, C], Xq [Tq, F, C] (numpy or DeviceArray) on one
    time index.  Group labels default to the days of year 1 .. n of ``grouping.PaddedDOYGrouper``; with ``grouper`` (a function
    of an index label, like ``groupers.MONTH_GROUPER``) the labels are the sorted keys that occur in the fit index.  A group is
    fitted on the samples whose label lies within ``window`` positions of its own on the circular label axis."""

    def __init__(self, window=0, ctx=None, grouper=None):
        self.ctx = ctx or default_context()
        self.window = int(window)
        self.grouper = grouper
        self.state = None

    def _labels_of(self, index):
        if self.grouper is None:
            return np.asarray(index.dayofyear, dtype=np.int64)
        return group_keys(index, self.grouper)

    def fit(self, X, y, index):
        per_step = self._labels_of(index)
        labels = np.arange(1, int(per_step.max()) + 1) if self.grouper is None else np.unique(per_step)
        return self.fit_labels(X, y, per_step, labels)

    def fit_labels(self, X, y, per_step, labels):
        """``per_step`` [T]: the group label of every time step; ``labels`` [n]: the labels in model order"""
        labels = np.asarray(labels)
        n = len(labels)
        check_window(self.window, n)
        self.labels_ = labels
        self.fitted_ = np.ones(n, dtype=bool)  # (every label is a group; the engine reports the empty ones)
        key = self.keys_of(per_step)
        self.state = self.ctx.grouped_fit(X, y, key, n, self.window)
        self.labels_ = labels
        self.fitted_ = self.state.fitted()
        self.status_ = self.state.status()
        return self

    def keys_of(self, per_step):
        """model index of every time step of a predict call; KeyError(label) for the smallest label without a fitted model
        (grouping.py:100-101: pandas visits the keys in sorted order)"""
        uniq, inv = np.unique(np.asarray(per_step), return_inverse=True)
        lookup = {_plain(k): g for g, k in enumerate(self.labels_)}
        at = np.empty(len(uniq), dtype=np.int32)
        for i, k in enumerate(uniq):
            g = lookup.get(_plain(k))
            if g is None or not self.fitted_[g]:
                raise KeyError(k)  # (the key as NumPy / pandas hold it, like the reference's dict lookup)
            at[i] = g
        return at[inv.ravel()]

    def predict(self, Xq, index, out=None):
        return self.predict_labels(Xq, self._labels_of(index), out=out)

    def predict_labels(self, Xq, per_step, out=None):
        if self.state is None:
            raise NotFittedError("This grouped grid model is not fitted yet.")
        return self.ctx.grouped_predict(self.state, Xq, self.keys_of(per_step), out=out)

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
        self.state = self.ctx.grouped_import(e)


def _plain(k):
    return k.item() if isinstance(k, np.generic) else k


class _FittedGroupModel:
    """``estimators_[key]`` stand-in: the numbers of the group's fitted sklearn LinearRegression for a DataFrame ``y``
    (coef_ (n_targets, F), intercept_ (n_targets,))."""

    def __init__(self, coef, intercept):
        self.coef_ = coef
        self.intercept_ = intercept

    def predict(self, X):
        return np.asarray(X, dtype=np.float64) @ self.coef_.T + self.intercept_


def default_none_kwargs(kwargs):
    return {} if kwargs is None else kwargs


class GroupedRegressor:
    """Grouped Regressor (grouping.py:12-103): fits separate estimators on distinct (or overlapping) groups.

    Parameters
    ----------
    estimator : estimator class; ``sklearn.linear_model.LinearRegression`` (or its name) runs on the HIP engine
    fit_grouper : class whose instances ``fit_grouper(index, **fit_grouper_kwargs)`` carry ``.groups`` {key -> positions}
    predict_grouper : anything ``DataFrame.groupby`` accepts; evaluated on the index of the predict input
    estimator_kwargs, fit_grouper_kwargs, predict_grouper_kwargs : dict, optional

    Attributes
    ----------
    targets_ : list, the columns of y
    estimators_ : dict {key -> fitted estimator}; on the engine path a stand-in with ``coef_`` and ``intercept_``
    """

    def __init__(self, estimator, fit_grouper, predict_grouper, estimator_kwargs=None, fit_grouper_kwargs=None,
                 predict_grouper_kwargs=None):
        self.estimator = estimator
        self.estimator_kwargs = estimator_kwargs
        self.fit_grouper = fit_grouper
        self.fit_grouper_kwargs = fit_grouper_kwargs
        self.predict_grouper = predict_grouper
        self.predict_grouper_kwargs = predict_grouper_kwargs

    # ---- which path ----
    def _is_linear(self):
        from sklearn.linear_model import LinearRegression

        return self.estimator is LinearRegression or self.estimator == "LinearRegression"

    def _estimator_class(self):
        if self.estimator == "LinearRegression":
            from sklearn.linear_model import LinearRegression

            return LinearRegression
        return self.estimator

    def _is_doy(self):
        return isinstance(self.fit_grouper, type) and issubclass(self.fit_grouper, PaddedDOYGrouper)

    def _check_engine(self):
        """NotImplementedError unless the engine can batch this combination (grids have no host loop)"""
        if not self._is_linear():
            raise NotImplementedError(f"GroupedRegressor(estimator={self.estimator!r}) on a grid: {SUPPORTED}")
        check_sklearn_kwargs(self.estimator_kwargs, LINEAR_NEUTRAL, "estimator_kwargs", "plain OLS with intercept")

    def _fit_plan(self, index):
        """(label of every time step, labels in model order, window), or None when the groups overlap otherwise"""
        kw = default_none_kwargs(self.fit_grouper_kwargs)
        if self._is_doy():
            if set(kw) != {"window"}:
                return None  # (the host loop meets the constructor's TypeError)
            key, n = doy_keys(index)
            check_window(kw["window"], n)
            return key.astype(np.int64) + 1, np.arange(1, n + 1), int(kw["window"])
        groups = self.fit_grouper(index, **kw).groups
        pos = [np.asarray(v, dtype=np.int64) for v in groups.values()]
        flat = np.concatenate(pos) if pos else np.zeros(0, np.int64)
        if len(flat) != len(index) or not np.array_equal(np.sort(flat), np.arange(len(index))):
            return None  # overlapping groups, or samples outside every group
        labels = list(groups)
        per_step = np.empty(len(index), dtype=object)
        for k, p in zip(labels, pos):
            per_step[p] = k
        out = np.empty(len(labels), dtype=object)
        out[:] = labels
        return per_step, out, 0

    # ---- fit ----
    def fit(self, X, y, **fit_kwargs):
        """Fit the grouped regressor: X DataFrame (n_samples, n_features), y DataFrame (n_samples, n_targets)."""
        self.__dict__.pop("_grid", None)
        plan = None
        if self._is_linear() and not fit_kwargs and isinstance(X, pd.DataFrame) and isinstance(y, pd.DataFrame):
            check_sklearn_kwargs(self.estimator_kwargs, LINEAR_NEUTRAL, "estimator_kwargs", "plain OLS with intercept")
            if X.index.equals(y.index):
                plan = self._fit_plan(X.index)
        if plan is None:
            return self._fit_host(X, y, fit_kwargs)
        per_step, labels, window = plan
        Xv, yv = np.asarray(X.values, dtype=np.float64), np.asarray(y.values, dtype=np.float64)
        for name, a in (("X", Xv), ("y", yv)):
            if not np.isfinite(a).all():
                raise _finite_error(name, a)
        T, F = Xv.shape
        K = yv.shape[1]
        grid = GroupedGridModel(window)
        # several target columns are several cells that share the features
        grid.fit_labels(np.ascontiguousarray(np.broadcast_to(Xv[:, :, None], (T, F, K))), np.ascontiguousarray(yv), per_step, labels)
        if not grid.fitted_.all():  # a day-of-year group whose window holds no sample (sklearn refuses the empty fit)
            raise ValueError(NO_SAMPLES_MESSAGE.format(F=F))
        e = grid.export()
        if (e["status"] != _lib.CELL_OK).any():  # (validation has refused non-finite input: nothing else may pass silently)
            raise ValueError(f"GroupedRegressor.fit: the engine reported status {e['status'].tolist()}")
        self.targets_ = list(y.keys())
        self.estimators_ = {_plain(k): _FittedGroupModel(np.ascontiguousarray(e["coef"][g].T), e["intercept"][g].copy())
                            for g, k in enumerate(labels)}
        self.n_features_in_ = F
        self._engine = dict(window=window)
        self._grid = grid
        return self

    def _adopt(self, e, c, targets=("variable_0",)):
        """fitted attributes of cell ``c`` of an exported grid state"""
        self.targets_ = list(targets)
        self.estimators_ = {_plain(k): _FittedGroupModel(np.ascontiguousarray(e["coef"][g, :, c:c + 1].T), e["intercept"][g, c:c + 1].copy())
                            for g, k in enumerate(e["labels"]) if e["fitted"][g]}
        self.n_features_in_ = e["coef"].shape[1]
        self._engine = dict(window=int(e["window"]))

    def _fit_host(self, X, y, fit_kwargs):
        """grouping.py:67-80: the meta-estimator itself, one estimator per group"""
        self.__dict__.pop("_engine", None)
        est = self._estimator_class()
        kw = default_none_kwargs(self.fit_grouper_kwargs)
        x_groups = self.fit_grouper(X.index, **kw).groups
        y_groups = self.fit_grouper(y.index, **kw).groups
        self.targets_ = list(y.keys())
        ekw = default_none_kwargs(self.estimator_kwargs)
        self.estimators_ = {key: est(**ekw) for key in x_groups}
        for x_key, x_inds in x_groups.items():
            self.estimators_[x_key].fit(X.iloc[x_inds], y.iloc[y_groups[x_key]], **fit_kwargs)
        return self

    # ---- predict ----
    def _fitted_grid(self):
        if getattr(self, "_grid", None) is None:  # unpickled: the device state from the fitted numbers
            labels = np.empty(len(self.estimators_), dtype=object)
            labels[:] = list(self.estimators_)
            coef = np.stack([np.asarray(m.coef_, dtype=np.float64).T for m in self.estimators_.values()])          # [n, F, K]
            icpt = np.stack([np.asarray(m.intercept_, dtype=np.float64) for m in self.estimators_.values()])       # [n, K]
            grid = GroupedGridModel(self._engine["window"])
            grid.state = grid.ctx.grouped_import(dict(coef=coef, intercept=icpt, fitted=np.ones(len(labels), np.int32),
                                                      status=np.zeros(coef.shape[2], np.int32), window=grid.window))
            grid.labels_ = labels
            grid.fitted_ = np.ones(len(labels), dtype=bool)
            self._grid = grid
        return self._grid

    def _predict_labels(self, index, frame=None):
        """the key of every time step (grouping.py:97-98), evaluated once on the index"""
        kw = default_none_kwargs(self.predict_grouper_kwargs)
        if callable(self.predict_grouper) and not kw:
            return group_keys(index, self.predict_grouper)
        frame = pd.DataFrame(index=index) if frame is None else frame
        per_step = np.empty(len(index), dtype=object)
        for k, inds in frame.groupby(self.predict_grouper, **kw).indices.items():
            per_step[inds] = k
        return per_step

    def predict(self, X):
        """Predict estimator target for X: ndarray (n_samples, n_targets)."""
        if not hasattr(self, "estimators_"):
            raise NotFittedError("This GroupedRegressor instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 "using this estimator.")
        if getattr(self, "_engine", None) is None:
            return self._predict_host(X)
        Xv = np.asarray(X.values, dtype=np.float64)
        if Xv.ndim != 2 or Xv.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {Xv.shape[1] if Xv.ndim == 2 else '?'} features, but LinearRegression is expecting "
                             f"{self.n_features_in_} features as input.")
        if not np.isfinite(Xv).all():
            raise _finite_error("X", Xv)
        grid = self._fitted_grid()
        T, F = Xv.shape
        K = len(self.targets_)
        out, status = grid.predict_labels(np.ascontiguousarray(np.broadcast_to(Xv[:, :, None], (T, F, K))),
                                          self._predict_labels(X.index, X))
        if (status != _lib.CELL_OK).any():
            raise ValueError(f"GroupedRegressor.predict: the engine reported status {status.tolist()}")
        return out

    def _predict_host(self, X):
        """grouping.py:96-103"""
        grouper = X.groupby(self.predict_grouper, **default_none_kwargs(self.predict_grouper_kwargs))
        result = np.empty((len(X), len(self.targets_)))
        for key, inds in grouper.indices.items():
            result[inds, ...] = self.estimators_[key].predict(X.iloc[inds])
        return result

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_grid", None)
        return d
