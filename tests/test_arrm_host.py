"""PiecewiseLinearRegression on the host: the NumPy restatement (tests/_arrm_oracle.py) pinned to the breakpoints recorded from the
reference's arrm_breakpoints (tests/golden/g23_arrm*.npz) on every cell, its traps, and the surface of the class: signatures,
messages, keyword screening and the paths that are not offered.  Nothing here reaches the engine."""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _arrm_oracle as ao  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return {c: ao.golden_case(c) for c in ao.CASES}


@pytest.mark.parametrize("c", ao.CASES)
def test_oracle_indices_equal_the_reference(golden, c):
    g = golden[c]
    assert g["X"].shape[1] == 67
    for k in range(g["X"].shape[1]):
        o = ao.breakpoints(g["X"][:, k], g["y"][:, k], 0.05, g["mb"])
        assert np.array_equal(o["index"], g["index"][:, k]) and np.array_equal(o["breaks"], g["breaks"][:, k]), (c, k)
        if k < 3:
            assert np.array_equal(o["r2"], g["r2"][:, k], equal_nan=True) and o["margin"] == g["margin"][k]


def test_trap_wrap_gives_duplicate_breaks(golden):
    idx = golden["gauss200"]["index"]
    dup = (np.diff(idx, axis=0) == 0).any(axis=0)
    assert dup.sum() >= 5 and (idx[:, dup].min(axis=0) < 10).all()  # only an index below 10 escapes its own mask


def test_trap_odd_width_leaves_every_other_slot(golden):
    r2 = golden["gauss500"]["r2"]  # width 25
    written = r2[:, 0] != 2
    assert not written[1::2].any() and written[14:480:2].all()


def test_trap_nan_windows_are_picked_first(golden):
    g = golden["halfzero600"]
    assert np.isnan(g["r2"]).any(axis=0).all()
    assert (g["index"][:3] == np.array([[15], [26], [37]])).all()  # the first NaN, then the first NaN beyond each mask


def test_minimum_norm_on_duplicate_breaks(golden):
    g = golden["gauss200"]
    same = np.diff(g["breaks"][1:-1], axis=0) == 0  # hinges j + 1 and j + 2 coincide: a rank-deficient design
    cells = np.flatnonzero(same.any(axis=0))
    assert len(cells) >= 3
    for k in cells:
        j = int(np.flatnonzero(same[:, k])[0])
        beta = g["beta"][:, k]
        assert beta[j + 2] == pytest.approx(beta[j + 3], rel=1e-9)  # gelsd splits the coefficient equally


def test_signatures_and_export():
    import skdownscale_amd as sd
    from skdownscale_amd import _lib, arrm

    assert list(inspect.signature(arrm.arrm_breakpoints).parameters) == ["X", "y", "window_width", "max_breakpoints"]
    p = inspect.signature(arrm.PiecewiseLinearRegression.__init__).parameters
    assert [(k, v.default) for k, v in p.items() if k != "self"] == [("n_segments", 7), ("fit_option", "auto"), ("pwlf_kwargs", None)]
    assert sd.PiecewiseLinearRegression is arrm.PiecewiseLinearRegression and sd.ArrmGridModel is arrm.ArrmGridModel
    assert arrm.PiecewiseLinearRegression._fit_attributes == ["model_", "fit_breaks_"]
    for name in ("fit", "fit_dev", "predict", "predict_dev", "state_info", "state_export", "state_import", "state_destroy"):
        assert f"sd_arrm_{name}" in _lib.SIGNATURES


def test_arrm_breakpoints_errors():
    from skdownscale_amd import arrm_breakpoints

    X, y = np.zeros((60, 1)), np.zeros(59)
    with pytest.raises(ValueError, match="X and y must have the same length, got 60 and 59"):
        arrm_breakpoints(X, y, 0.05, 6)
    with pytest.raises(ValueError, match="X must have exactly 1 feature, got 2"):
        arrm_breakpoints(np.zeros((60, 2)), np.zeros(60), 0.05, 6)
    with pytest.raises(NotImplementedError, match="window_width=0.2"):
        arrm_breakpoints(np.zeros((600, 1)), np.zeros(600), 0.2, 6)


def test_class_errors_before_the_engine():
    from sklearn.base import clone
    from sklearn.exceptions import NotFittedError

    from skdownscale_amd import PiecewiseLinearRegression

    rng = np.random.default_rng(1)
    X, y = rng.normal(size=(80, 1)), rng.normal(size=80)
    m = PiecewiseLinearRegression()  # constructing needs no pwlf
    assert clone(m).get_params() == {"n_segments": 7, "fit_option": "auto", "pwlf_kwargs": None}
    with pytest.raises(NotFittedError):
        m.predict(X)
    with pytest.raises(NotImplementedError, match="differential evolution"):
        m.fit(X, y)
    with pytest.raises(NotImplementedError, match="random multistart"):
        PiecewiseLinearRegression(fit_option="fast").fit(X, y)
    with pytest.raises(ValueError, match="unsupported fit_option 'best'"):
        PiecewiseLinearRegression(fit_option="best").fit(X, y)
    with pytest.raises(ValueError, match=r"Found array with 2 features \(shape=\(80, 2\)\) while a maximum of 1 is required"):
        PiecewiseLinearRegression(fit_option="arrm").fit(np.hstack([X, X]), y)
    with pytest.raises(ValueError, match="Input X contains NaN"):
        PiecewiseLinearRegression(fit_option="arrm").fit(np.where(X > 2, np.nan, X), y)
    with pytest.raises(NotImplementedError, match="pwlf_kwargs={'degree': 2}"):
        PiecewiseLinearRegression(fit_option="arrm", pwlf_kwargs={"degree": 2}).fit(X, y)
    with pytest.raises(NotImplementedError, match="pwlf_kwargs={'weights'"):
        PiecewiseLinearRegression(fit_option="arrm", pwlf_kwargs={"weights": np.ones(80)}).fit(X, y)
    with pytest.raises(TypeError, match=r"fit_with_breaks\(\) got an unexpected keyword argument 'atol'"):
        PiecewiseLinearRegression(fit_option="arrm", pwlf_kwargs={"seed": 3, "lapack_driver": "gelsy", "disp_res": True}).fit(X, y, atol=1)
    with pytest.raises(ValueError, match="at least 50 samples, got 49"):
        PiecewiseLinearRegression(fit_option="arrm").fit(X[:49], y[:49])
    with pytest.raises(ValueError, match="supported are 2 .. 16"):
        PiecewiseLinearRegression(n_segments=1, fit_option="arrm").fit(X, y)
    with pytest.raises(ValueError, match="supported are 2 .. 16"):
        PiecewiseLinearRegression(n_segments=18, fit_option="arrm").fit(X, y)


def test_fitted_model_object_predicts_like_the_oracle(golden):
    from skdownscale_amd.arrm import FittedPiecewiseModel

    g = golden["query101"]
    m = FittedPiecewiseModel(g["breaks"][:, 0], g["beta"][:, 0], g["ssr"][0])
    assert (m.n_segments, m.n_parameters) == (5, 6)
    assert np.allclose(m.predict(g["Xq"][:, 0]), g["pred"][:, 0], rtol=1e-13, atol=0)


@pytest.fixture(scope="module")
def golden_breaks():
    return {c: ao.breaks_case(c) for c in ao.CASES_BREAKS}


@pytest.mark.parametrize("c", ao.CASES_BREAKS)
def test_oracle_reproduces_the_break_goldens(golden_breaks, c):
    """g24: every cell's picks, breaks and start2 recorded from the reference, and the reference's ValueError exactly where the
    ``raises`` flag says (start2 == 0: np.argmin of r2[:0])"""
    g = golden_breaks[c]
    for k in range(g["X"].shape[1]):
        if g["raises"][k]:
            with pytest.raises(ValueError, match="^attempt to get argmin of an empty sequence$"):
                ao.breakpoints(g["X"][:, k], g["y"][:, k], 0.05, g["mb"])
            assert g["start2"][k] == 0 and (g["index"][:, k] == -1).all() and np.isnan(g["breaks"][:, k]).all()
            continue
        o = ao.breakpoints(g["X"][:, k], g["y"][:, k], 0.05, g["mb"])
        assert np.array_equal(o["index"], g["index"][:, k]) and np.array_equal(o["breaks"], g["breaks"][:, k]), (c, k)
        assert o["start2"] == g["start2"][k] != 0 and o["sentinel_picks"] == g["sentinel"][k]
        assert o["margin_computed"] == g["margin_computed"][k] >= o["margin"] == g["margin"][k]
        assert np.array_equal(o["r2"], g["r2"][:, k], equal_nan=True)


def test_break_goldens_cover_their_territory(golden_breaks):
    short = [g for c, g in golden_breaks.items() if c.startswith("short")]
    assert sum(int(g["raises"].sum()) for g in short) >= 1 and all(g["raises"].mean() <= 0.5 for g in short)
    assert any((g["start2"] < 0).any() for g in short) and any((g["sentinel"] > 0).any() for g in short)
    for c, g in golden_breaks.items():
        live = ~g["raises"]
        assert (g["margin_computed"][live] < 1e-6).mean() <= 0.05, c
    assert not any(g["raises"].any() for c, g in golden_breaks.items() if not c.startswith("short"))
    assert np.isnan(golden_breaks["quant300_mb8"]["r2"]).any(axis=0).all()
    widths = {c: max(round(0.05 * len(g["X"])), 10) for c, g in golden_breaks.items()}
    assert [widths[c] for c in ("w210_mb8", "w230_mb12", "w250_mb16", "w270_mb9", "w220_mb8", "w260_mb8")] == [10, 12, 12, 14, 11, 13]


def test_oracle_solve_against_longdouble(golden_breaks):
    """How far the float64 gelsd solve of the oracle is from a least-squares solve in np.longdouble, as a share of the std of the
    predictions: the GPU tests ask 1e-9 of the engine, so the oracle must be good to a tenth of that where they use it"""
    worst = 0.0
    for c in ("short50_mb16", "w250_mb16", "mb17_1000", "quant300_mb8"):
        g = golden_breaks[c]
        for k in np.flatnonzero(~g["raises"])[:4]:
            hp = ao.predict_longdouble(g["X"][:, k], g["y"][:, k], g["breaks"][:, k], g["X"][:, k])
            worst = max(worst, float(np.abs(g["pred"][:, k] - hp).max() / np.std(g["pred"][:, k])))
    print("oracle against longdouble, err / std", worst)
    assert worst <= 1e-10
