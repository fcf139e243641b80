"""Cross-check of the oracles against the real reference, on what the reference returned for these very inputs: every call
into the reference (``ref.X(...).fit(...).predict(...)`` and the fitted attributes read) was recorded by
tests/golden/make_golden.py (``g21_reference_calls``: ``SD_RECORD_REFERENCE=1`` runs this module against the live reference
through ``ref_shim.Recorder``) and is replayed here by ``ref_shim.Replay``; the oracle side runs live.  Inputs of their own (not
the golden cases'), so it also guards the goldens against having been tuned to."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import analog_oracle as ao
import bcsd_oracle as bo
import qm_oracle as qo
import ref_shim
from _cases import GOLDEN, assert_close

RECORD = os.environ.get("SD_RECORD_REFERENCE") == "1"  # make_golden.py: run on the live reference and store what it returned
FUZZ = "test_random_sweep_of_the_oracles_against_the_live_reference"
# golden file -> (which tests' recordings it holds, number of parts: members dealt round-robin, each part under 1 MiB)
FILES = {"g21_reference_calls": (lambda name: name != FUZZ, 1), "g21_reference_fuzz": (lambda name: name == FUZZ, 2)}
_recorded = {}


def _file_of(name):
    return next(f for f, (takes, _) in FILES.items() if takes(name))


def _parts(f):
    n = FILES[f][1]
    return [os.path.join(GOLDEN, f + ".npz")] if n == 1 else [os.path.join(GOLDEN, f"{f}_{i}.npz") for i in range(n)]


@pytest.fixture(scope="module", autouse=True)
def _store_recording():
    yield
    if RECORD:
        for f in FILES:
            arrays = {}
            for name, rec in _recorded.items():
                if _file_of(name) == f:
                    arrays.update(rec.arrays(name))
            paths = _parts(f)
            for i, path in enumerate(paths):
                np.savez_compressed(path, **{k: v for j, (k, v) in enumerate(sorted(arrays.items())) if j % len(paths) == i})


@pytest.fixture
def ref(request):
    """the reference namespace: recorded results (default) or, with SD_RECORD_REFERENCE=1, the live reference being recorded"""
    name = request.node.name
    if RECORD:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rec = ref_shim.Recorder(ref_shim.load())
        _recorded[name] = rec
        yield rec
        return
    stored = {}
    for path in _parts(_file_of(name)):
        with np.load(path, allow_pickle=False) as z:
            stored.update({k: z[k] for k in z.files if k.startswith(name + "/")})
    rep = ref_shim.Replay(stored, name)
    yield rep
    assert rep.finished(), f"{name}: fewer reference calls than recorded"


def frame(a, index):
    return pd.DataFrame(np.asarray(a).reshape(len(index), -1), index=index)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("T,Tp", [(1461, 1461), (1461, 2000), (1461, 500)])
def test_bcsd(ref, kind, T, Tp):
    rng = np.random.default_rng(T + Tp + kind)
    index, index_p = pd.date_range("1990-01-01", periods=T), pd.date_range("1990-01-01", periods=Tp)
    if kind == 0:
        X, y, Xp = (12 + 7 * rng.standard_normal(n) for n in (T, T, Tp))
        cls = ref.BcsdTemperature
    else:
        X, y, Xp = (rng.gamma(0.8, 4.0, n) * (rng.random(n) > 0.4) for n in (T, T, Tp))
        y = y + 0.05
        cls = ref.BcsdPrecipitation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cls().fit(frame(X, index), frame(y, index)).predict(frame(Xp, index_p)).values[:, 0]
    out, status = bo.pointwise_fit_predict(kind, X[:, None], y[:, None], Xp[:, None], bo.month_group_id(index), bo.month_group_id(index_p))
    assert status[0] == 0
    assert_close(out[:, 0], exp, what=f"bcsd kind={kind} {T}->{Tp}")


@pytest.mark.parametrize("kind", [0, 1])
def test_bcsd_qt_kwargs(ref, kind):
    """Random `extrapolate` / `n_endpoints` / `alpha` / `beta` in qm_kwargs={'qt_kwargs': ...}, predict series longer and shorter
    than the fit series: the oracle's tails (and its ignoring of alpha / beta) against the live reference."""
    rng = np.random.default_rng(77 + kind)
    T = 1461
    index = pd.date_range("1990-01-01", periods=T)
    for case in range(8):
        Tp = int(rng.choice([900, 2100, 2600]))
        index_p = pd.date_range("1990-01-01", periods=Tp)
        if kind == 0:
            X, y, Xp = (12 + 7 * rng.standard_normal(n) for n in (T, T, Tp))
            cls = ref.BcsdTemperature
        else:
            X, y, Xp = (rng.gamma(0.8, 4.0, n) * (rng.random(n) > 0.4) for n in (T, T, Tp))
            y = y + 0.05
            cls = ref.BcsdPrecipitation
        kw = dict(extrapolate=[None, "min", "max", "both", "1to1"][int(rng.integers(5))], n_endpoints=int(rng.integers(1, 60)))
        extra = dict(alpha=float(rng.random()), beta=float(rng.random())) if case % 2 else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = cls(qm_kwargs={"qt_kwargs": {**kw, **extra}}).fit(frame(X, index), frame(y, index)).predict(frame(Xp, index_p)).values[:, 0]
        out, status = bo.pointwise_fit_predict(kind, X[:, None], y[:, None], Xp[:, None], bo.month_group_id(index), bo.month_group_id(index_p), **kw)
        assert status[0] == 0
        assert_close(out[:, 0], exp, what=f"bcsd kind={kind} {T}->{Tp} qt_kwargs {kw} {extra}")


def test_bcsd_daily_nasanex(ref):
    rng = np.random.default_rng(3)
    index = pd.date_range("1983-01-01", "1986-12-31")
    index_p = pd.date_range("1984-05-01", "1985-08-31")
    X, y, Xp = (12 + 7 * rng.standard_normal(n) for n in (len(index), len(index), len(index_p)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ref.BcsdTemperature(time_grouper="daily_nasa-nex", return_anoms=False).fit(frame(X, index), frame(y, index))
        exp = m.predict(frame(Xp, index_p)).values[:, 0]
    st, _ = bo.bcsd_fit_cell(bo.TAS, X, y, None, table=bo.padded_doy_table(index), return_anoms=False)
    np.testing.assert_allclose(st["y_climo"], m.y_climo_.values[:, 0], rtol=1e-12)
    out, _ = bo.bcsd_predict_trend_cell(st, Xp, np.asarray(index_p.day) - 1, np.asarray(index_p.month) - 1, return_anoms=False)
    assert_close(out, exp, what="daily_nasa-nex")


@pytest.mark.parametrize("F", [1, 3])
def test_analogs(ref, F):
    rng = np.random.default_rng(F)
    X, Xq = rng.standard_normal((400, F)), rng.standard_normal((60, F))
    y = X.sum(axis=1) + 0.5 * rng.standard_normal(400)
    for kind in ("best_analog", "weight_analogs", "mean_analogs"):
        for thresh in (None, 0.0):
            exp = ref.PureAnalog(n_analogs=25, kind=kind, thresh=thresh).fit(X, y).predict(Xq)
            out, _, _ = ao.pure_analog_predict(X, y, Xq, 25, {"best_analog": ao.KIND_BEST, "weight_analogs": ao.KIND_WEIGHT, "mean_analogs": ao.KIND_MEAN}[kind], thresh)
            assert_close(out, exp, what=f"PureAnalog {kind} thresh={thresh}")
    exp = ref.AnalogRegression(n_analogs=25).fit(X, y).predict(Xq)
    assert_close(ao.analog_regression_predict(X, y, Xq, 25)[0], exp, what="AnalogRegression")
    tight = dict(tol=1e-12, max_iter=100000)
    exp = ref.AnalogRegression(n_analogs=40, thresh=-1.5, logistic_kwargs=tight).fit(X, y).predict(Xq)
    out = ao.analog_regression_thresh_predict(X, y, Xq, 40, -1.5)[0]
    assert_close(out[:, [0, 2]], exp[:, [0, 2]], what="AnalogRegression(thresh)")
    assert np.abs(out[:, 1] - exp[:, 1]).max() < 1e-6
    exp = ref.gard.PureRegression(thresh=0.1, logistic_kwargs=tight).fit(X, y).predict(Xq)
    out = ao.pure_regression_thresh(X, y, Xq, 0.1)[0]
    assert_close(out[:, [0, 2]], exp[:, [0, 2]], what="PureRegression(thresh)")
    assert np.abs(out[:, 1] - exp[:, 1]).max() < 1e-6


@pytest.mark.parametrize("ex", [None, "1to1", "min", "max", "both"])
def test_quantile_mapping_regressors(ref, ex):
    rng = np.random.default_rng(9)
    X, y = 10 + 3 * rng.standard_normal(300), 12 + 4 * rng.standard_normal(300)
    Xp = X.min() + (X.max() - X.min()) * rng.random(300)  # inside the fitted range: every mode is well conditioned
    Q = ref.quantile
    exp = Q.QuantileMappingReressor(extrapolate=ex).fit(X.reshape(-1, 1), y).predict(Xp.reshape(-1, 1))
    assert_close(qo.qmr_predict(qo.qm_fit(X, y, ex), Xp, ex), exp, what=f"QMR {ex}")
    for kind in ("difference", "ratio"):
        exp = Q.EquidistantCdfMatcher(kind=kind, extrapolate=ex).fit(X.reshape(-1, 1), y).predict(Xp.reshape(-1, 1))
        assert_close(qo.ecm_predict(qo.qm_fit(X, y, ex), Xp, kind, ex), exp, what=f"ECM {kind} {ex}")


@pytest.mark.parametrize("model", ["qmr", "ecm"])
def test_trend_aware_regressor(ref, model):
    """TrendAwareQuantileMappingRegressor of the live reference (quantile.py:639-716) vs oracle/qm_oracle.py: trend_aware_predict
    on fresh drifting series"""
    rng = np.random.default_rng(31 + len(model))
    T, Tp = 900, 1300
    index, index_p = pd.date_range("1990-01-01", periods=T), pd.date_range("1995-01-01", periods=Tp)
    X = 10 + 3 * rng.standard_normal(T) + 4e-3 * np.arange(T)
    y = 8 + 4 * rng.standard_normal(T) + 2e-3 * np.arange(T)
    Xp = 11 + 3 * rng.standard_normal(Tp) + 5e-3 * np.arange(Tp)
    inner = ref.quantile.QuantileMappingReressor() if model == "qmr" else ref.quantile.EquidistantCdfMatcher()
    m = ref.quantile.TrendAwareQuantileMappingRegressor(inner).fit(frame(X, index), frame(y, index))
    exp = np.asarray(m.predict(frame(Xp, index_p))).reshape(-1)
    out = qo.trend_aware_predict(model, X, y, Xp)
    assert_close(out, exp, what=f"trend-aware {model}")


def test_random_sweep_of_the_oracles_against_the_live_reference(ref):
    """tools/dev/fuzz_oracle_vs_reference.py: 120 random cases over all eight case types (38 216 passed at the end of round 3), the
    reference's side as recorded from the live reference"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dev"))
    import fuzz_oracle_vs_reference

    assert fuzz_oracle_vs_reference.main(float("inf"), 70000, None, 120, ref=ref) == 0
