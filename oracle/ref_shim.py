"""TEST INFRASTRUCTURE ONLY -- import shim for the *reference* scikit-downscale.

``load()`` needs a checkout of the reference (``SKDOWNSCALE_REFERENCE``).  It is used by
``tests/golden/make_golden.py`` to generate golden vectors, and through ``Recorder`` / ``Replay``
below by the cross-check tests, which run on the reference's recorded results.  Nothing under
``scikit-downscale_amd/`` may import this module.

``import skdownscale.pointwise_models`` fails here because ``core.py``/``zscore.py``
import xarray (not installed).  We register empty stub packages whose ``__path__``
points into the reference tree so the numeric modules (bcsd, quantile, gard, groupers,
base, utils, trend) import and run unmodified.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

REF_ROOT = os.environ.get("SKDOWNSCALE_REFERENCE", "/root/reference")


def available() -> bool:
    return os.path.isdir(os.path.join(REF_ROOT, "skdownscale", "pointwise_models"))


def load():
    """Return a namespace with the reference's hot-path classes."""
    if not available():
        raise RuntimeError(f"reference tree not found at {REF_ROOT}")
    if "skdownscale" not in sys.modules or not getattr(sys.modules["skdownscale"], "_sd_shim", False):
        pkg = types.ModuleType("skdownscale")
        pkg.__path__ = [os.path.join(REF_ROOT, "skdownscale")]
        pkg._sd_shim = True
        sub = types.ModuleType("skdownscale.pointwise_models")
        sub.__path__ = [os.path.join(REF_ROOT, "skdownscale", "pointwise_models")]
        sys.modules["skdownscale"] = pkg
        sys.modules["skdownscale.pointwise_models"] = sub
    ns = types.SimpleNamespace()
    for name in ("utils", "trend", "quantile", "groupers", "base", "bcsd", "gard"):
        setattr(ns, name, importlib.import_module(f"skdownscale.pointwise_models.{name}"))
    ns.BcsdTemperature = ns.bcsd.BcsdTemperature
    ns.BcsdPrecipitation = ns.bcsd.BcsdPrecipitation
    ns.PureAnalog = ns.gard.PureAnalog
    ns.AnalogRegression = ns.gard.AnalogRegression
    ns.QuantileMapper = ns.quantile.QuantileMapper
    ns.CunnaneTransformer = ns.quantile.CunnaneTransformer
    return ns


# ---- recorded reference calls: tests/test_oracle_vs_reference.py runs on what the reference returned, stored under tests/golden/ ----

def _leaf(v):
    """(kind, array) for a value the caller reads (arrays, frames, scalars); ('obj', None) for anything it calls into further"""
    import numpy as np
    import pandas as pd

    if isinstance(v, pd.DataFrame):
        return "frame", np.asarray(v.values)
    if isinstance(v, pd.Series):
        return "series", np.asarray(v.values)
    if isinstance(v, (np.ndarray, np.generic, bool, int, float, str)):
        return ("array" if isinstance(v, np.ndarray) else "scalar"), np.asarray(v)
    return "obj", None


def _unwrap(v):
    if isinstance(v, Recorder):
        return object.__getattribute__(v, "_target")
    if isinstance(v, (list, tuple)):
        return type(v)(_unwrap(x) for x in v)
    if isinstance(v, dict):
        return {k: _unwrap(x) for k, x in v.items()}
    return v


class Recorder:
    """Wraps the live reference (``load()``): attribute reads and calls go through, and every value the caller gets back (arrays,
    frames, scalars) is logged in order, so that ``Replay`` can hand out the same values without the reference."""

    def __init__(self, target, log=None):
        object.__setattr__(self, "_target", target)
        object.__setattr__(self, "_log", [] if log is None else log)

    def _wrap(self, op, v):
        kind, val = _leaf(v)
        log = object.__getattribute__(self, "_log")
        log.append((op, kind, val))
        return Recorder(v, log) if kind == "obj" else v

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self._wrap("." + name, getattr(object.__getattribute__(self, "_target"), name))

    def __call__(self, *args, **kwargs):
        return self._wrap("()", object.__getattribute__(self, "_target")(*_unwrap(args), **_unwrap(kwargs)))

    def arrays(self, key):
        """the log as npz members under ``key/``"""
        import numpy as np

        log = object.__getattribute__(self, "_log")
        out = {f"{key}/ops": np.array([op for op, _, _ in log], dtype=str), f"{key}/kinds": np.array([k for _, k, _ in log], dtype=str)}
        for i, (_, kind, val) in enumerate(log):
            if kind != "obj":
                out[f"{key}/{i}"] = val
        return out


class Replay:
    """Stands in for the reference namespace: hands out, in order, the values a ``Recorder`` logged for the same sequence of
    attribute reads and calls (a different sequence is an error)."""

    def __init__(self, npz, key, pos=None):
        self._npz, self._key = npz, key
        self._ops = [str(s) for s in npz[f"{key}/ops"]] if pos is None else None
        self._kinds = [str(s) for s in npz[f"{key}/kinds"]] if pos is None else None
        self._pos = [0, self._ops, self._kinds] if pos is None else pos

    def _next(self, op):
        i, ops, kinds = self._pos
        assert i < len(ops) and ops[i] == op, f"replay of {self._key} out of step at {i}: recorded {ops[i] if i < len(ops) else 'end'}, called {op}"
        self._pos[0] += 1
        if kinds[i] == "obj":
            return Replay(self._npz, self._key, self._pos)
        import pandas as pd

        val = self._npz[f"{self._key}/{i}"]
        return {"frame": pd.DataFrame, "series": pd.Series, "array": lambda a: a, "scalar": lambda a: a[()]}[kinds[i]](val)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return self._next("." + name)

    def __call__(self, *args, **kwargs):
        return self._next("()")

    def finished(self):
        return self._pos[0] == len(self._pos[1])
