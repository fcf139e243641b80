"""GPU parity: PiecewiseLinearRegression(fit_option='arrm') (csrc/sd_arrm.hip through the C ABI, ArrmGridModel, the class and
PointWiseDownscaler) against breakpoints recorded from the reference's arrm_breakpoints (tests/golden/g23_arrm*.npz) and the
NumPy restatement of the fit on them (tests/_arrm_oracle.py).

Tolerances: r2 within 1e-8 (1/100 of the selection margin 1e-6 below which a cell is left out of the break-index assertion, so an
r2 error cannot flip a retained pick); predictions within the project's least-squares tolerance, rtol 1e-9 of the expected
field's std (tests/test_gpu_grouped.py); beta within 1e-9 * cond(A) of its largest entry."""
import pickle

import numpy as np
import pandas as pd
import pytest

import _arrm_oracle as ao
from _cases import assert_close

pytestmark = pytest.mark.gpu
RTOL = 1e-9
R2_TOL = 1e-8
MARGIN = 1e-6
MAX_EXCLUDED = 0.05


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


@pytest.fixture(scope="module")
def golden():
    return {c: ao.golden_case(c) for c in ao.CASES}


@pytest.fixture(scope="module")
def fitted(ctx, golden):
    """every case fitted once through the ABI: (exported state, r2, predictions, predict status)"""
    res = {}
    for c, g in golden.items():
        st, r2 = ctx.arrm_fit(g["X"], g["y"], g["mb"], with_r2=True)
        out, status = ctx.arrm_predict(st, g["Xq"])
        res[c] = (st.export(), r2, out, status)
        st.close()
    return res


@pytest.mark.parametrize("c", ao.CASES)
def test_r2(golden, fitted, c):
    r2, exp = fitted[c][1], golden[c]["r2"]
    assert np.array_equal(np.isnan(r2), np.isnan(exp)), f"{c}: NaN positions of r2 differ"
    err = np.abs(r2 - exp)[~np.isnan(exp)].max()
    print(c, "r2 max err", err)
    assert err <= R2_TOL


@pytest.mark.parametrize("c", ao.CASES)
def test_break_indices(golden, fitted, c):
    g, (e, _, out, status) = golden[c], fitted[c]
    keep = g["margin"] >= MARGIN
    print(c, "cells left out", int((~keep).sum()), "of", len(keep))
    assert (~keep).mean() <= MAX_EXCLUDED
    assert (e["status"] == 0).all() and (status == 0).all() and np.isfinite(out).all()
    assert np.array_equal(e["break_index"][:, keep], g["index"][:, keep])
    assert np.array_equal(e["breaks"][:, keep], g["breaks"][:, keep])


@pytest.mark.parametrize("c", ao.CASES)
def test_predictions_and_beta(golden, fitted, c):
    g, (e, _, out, _) = golden[c], fitted[c]
    keep = g["margin"] >= MARGIN
    print(c, "pred err / std", np.abs(out - g["pred"])[:, keep].max() / np.std(g["pred"][:, keep]))
    assert_close(out[:, keep], g["pred"][:, keep], rtol=RTOL, what=f"{c} pred")
    # (duplicate breaks make the design rank deficient: the stored beta is gelsd's minimum-norm solution)
    err = np.abs(e["beta"] - g["beta"])[:, keep].max(axis=0)
    bound = RTOL * g["cond"][keep] * np.abs(g["beta"][:, keep]).max(axis=0)
    print(c, "beta err / bound", (err / bound).max())
    assert (err <= bound).all()
    # ssr = sum e^2 - c.g in e = y - y[0]: both terms are of the size of the total sum of squares (a few times it when y[0] lies
    # off the mean) and carry T roundings of 1.1e-16 each plus the error of the hat-basis solve (condition below 1e3), so the
    # difference is good to about 1e-12 of the total sum of squares; 1e-10 of it is asked
    ssr_err = np.abs(e["ssr"] - g["ssr"])[keep]
    tss = np.sum((g["y"] - g["y"].mean(axis=0)) ** 2, axis=0)[keep]
    print(c, "ssr err / total sum of squares", (ssr_err / tss).max())
    assert (ssr_err <= 1e-10 * tss).all()


def test_duplicate_breaks_are_covered(golden):
    dup = [(np.diff(golden[c]["index"], axis=0) == 0).any(axis=0).sum() for c in ("gauss200", "gauss365")]
    assert min(dup) > 0  # the wrap of the mask (index < 10) picks an index twice


def test_state_round_trip_is_bit_identical(ctx, golden):
    g = golden["query101"]
    st = ctx.arrm_fit(g["X"], g["y"], g["mb"])
    e = st.export()
    out, status = ctx.arrm_predict(st, g["Xq"])
    st2 = ctx.arrm_import(e)
    e2 = st2.export()
    out2, status2 = ctx.arrm_predict(st2, g["Xq"])
    assert np.array_equal(out, out2) and np.array_equal(status, status2)
    for k in ("breaks", "break_index", "beta", "ssr", "status"):
        assert np.array_equal(e[k], e2[k]), k
    assert e2["T"] == len(g["X"])
    dX, dy, dq = ctx.to_device(g["X"]), ctx.to_device(g["y"]), ctx.to_device(g["Xq"])
    st3, r2_dev = ctx.arrm_fit(dX, dy, g["mb"], with_r2=True)  # the resident entry with its r2 diagnostic
    out3, _ = ctx.arrm_predict(st3, dq)
    assert np.array_equal(out3.to_host(), out)
    _, r2_host = ctx.arrm_fit(g["X"], g["y"], g["mb"], with_r2=True)
    assert np.array_equal(r2_dev.to_host(), r2_host, equal_nan=True) and np.array_equal(np.isnan(r2_host), np.isnan(g["r2"]))


def test_class_against_golden_and_pickle(golden):
    from sklearn.base import clone
    from sklearn.exceptions import NotFittedError

    from skdownscale_amd import PiecewiseLinearRegression, arrm_breakpoints

    g = golden["query101"]
    k = int(np.flatnonzero(g["margin"] >= MARGIN)[0])
    m = PiecewiseLinearRegression(fit_option="arrm", pwlf_kwargs={"disp_res": False, "degree": 1})
    with pytest.raises(NotFittedError):
        m.predict(g["Xq"][:, k:k + 1])
    assert clone(m).get_params() == m.get_params()
    m.fit(g["X"][:, k:k + 1], g["y"][:, k])
    assert np.array_equal(m.fit_breaks_, g["breaks"][:, k]) and np.array_equal(m.model_.fit_breaks, m.fit_breaks_)
    assert m.model_.n_segments == 5 and m.model_.n_parameters == 6 and m.X_.shape == (260, 1) and m.y_.shape == (260,)
    pred = m.predict(g["Xq"][:, k:k + 1])
    assert pred.shape == (101,)
    assert_close(pred, g["pred"][:, k], rtol=RTOL, what="class pred")
    assert_close(m.model_.predict(g["Xq"][:, k]), g["pred"][:, k], rtol=RTOL, what="model_ pred")
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m2.predict(g["Xq"][:, k:k + 1]), pred)
    assert np.array_equal(arrm_breakpoints(g["X"][:, k:k + 1], g["y"][:, k], 0.05, 7), g["breaks"][:, k])


def test_headline_length_against_the_oracle(ctx):
    """T = 14 600, the length of the benchmark workload: the r2 series of a cell takes 117 KB of LDS (the opt-in beyond 64 KB),
    a thread slides over 19 windows of 730 samples from one pivot, and the accumulate pass runs with 8 time slices.  Three cells
    against the NumPy restatement (about a second per cell)."""
    T, C = 14600, 3
    rng = np.random.default_rng(14600)
    X = 15.0 + 8.0 * rng.normal(size=(T, C))
    y = 13.0 + 0.9 * X + 0.05 * X * X + 3.0 * rng.normal(size=(T, C))
    Xq = np.concatenate([X.min(axis=0)[None] - 5.0, 15.0 + 8.0 * rng.normal(size=(300, C)), X.max(axis=0)[None] + 5.0])
    st, r2 = ctx.arrm_fit(X, y, 7, with_r2=True)
    e = st.export()
    out, status = ctx.arrm_predict(st, Xq)
    assert (e["status"] == 0).all() and (status == 0).all()
    for k in range(C):
        o = ao.breakpoints(X[:, k], y[:, k], 0.05, 7)
        assert np.array_equal(np.isnan(r2[:, k]), np.isnan(o["r2"]))
        print("T=14600 cell", k, "r2 max err", np.abs(r2[:, k] - o["r2"]).max(), "margin", o["margin"])
        assert np.abs(r2[:, k] - o["r2"]).max() <= R2_TOL
        if o["margin"] >= MARGIN:
            assert np.array_equal(e["break_index"][:, k], o["index"]) and np.array_equal(e["breaks"][:, k], o["breaks"])
        beta, ssr, cond = ao.fit_on_breaks(X[:, k], y[:, k], e["breaks"][:, k])  # (on the engine's breaks: the fit is checked either way)
        exp = ao.predict(Xq[:, k], e["breaks"][:, k], beta)
        print("T=14600 cell", k, "pred err / std", np.abs(out[:, k] - exp).max() / np.std(exp), "cond", cond)
        assert_close(out[:, k], exp, rtol=RTOL, what=f"T=14600 cell {k} pred")
        assert (np.abs(e["beta"][:, k] - beta) <= RTOL * cond * np.abs(beta).max()).all()
        assert abs(e["ssr"][k] - ssr) <= 1e-10 * np.sum((y[:, k] - y[:, k].mean()) ** 2)


def test_too_short_series(ctx):
    from skdownscale_amd import PiecewiseLinearRegression

    rng = np.random.default_rng(0)
    X, y = rng.normal(size=(49, 3)), rng.normal(size=(49, 3))
    with pytest.raises(ValueError, match="at least 50"):
        ctx.arrm_fit(X, y, 7)
    with pytest.raises(ValueError, match="at least 50 samples, got 49"):
        PiecewiseLinearRegression(fit_option="arrm").fit(X[:, :1], y[:, 0])
    with pytest.raises(ValueError, match="supported are 2 .. 16"):
        ctx.arrm_fit(rng.normal(size=(60, 2)), rng.normal(size=(60, 2)), 18)
    st = ctx.arrm_fit(rng.normal(size=(50, 2)), rng.normal(size=(50, 2)), 7)
    assert (st.export()["status"] == 0).all()


def test_pointwise_downscaler_mask_and_chunks(golden):
    from skdownscale_amd import GridArray, PiecewiseLinearRegression, PointWiseDownscaler

    g = golden["gauss365"]
    T, ny, nx = 365, 6, 11
    X, y, pred = (a[:, :ny * nx].reshape(T, ny, nx).copy() for a in (g["X"], g["y"], g["pred"]))
    X[:, 2, 3] = np.nan  # a masked cell (core.py:35-37)
    coords = {"time": pd.date_range("2001-01-01", periods=T), "lat": np.arange(ny), "lon": np.arange(nx)}
    Xg, yg = GridArray(X, ("time", "lat", "lon"), coords), GridArray(y, ("time", "lat", "lon"), coords)
    pw = PointWiseDownscaler(PiecewiseLinearRegression(fit_option="arrm"))
    pw.fit(Xg, yg)
    out = np.asarray(pw.predict(Xg).values)
    assert np.isnan(out[:, 2, 3]).all()
    live = np.ones((ny, nx), bool)
    live[2, 3] = False
    live &= (g["margin"][:ny * nx] >= MARGIN).reshape(ny, nx)
    assert_close(out[:, live], pred[:, live], rtol=RTOL, what="grid pred")
    breaks = np.asarray(pw.get_attr("fit_breaks_").values)
    assert breaks.shape == (6, ny, nx) and np.isnan(breaks[:, 2, 3]).all()
    assert np.array_equal(breaks[:, live], g["breaks"][:, :ny * nx].reshape(6, ny, nx)[:, live])
    with pytest.raises(TypeError, match=r"fit_with_breaks\(\) got an unexpected keyword argument 'atol'"):
        PointWiseDownscaler(PiecewiseLinearRegression(fit_option="arrm")).fit(Xg, yg, atol=1)
    from skdownscale_amd.core import LazyGridArray

    pc = PointWiseDownscaler(PiecewiseLinearRegression(fit_option="arrm"))
    pc.fit(Xg.chunk({"lat": 4, "lon": 5}), yg.chunk({"lat": 4, "lon": 5}))
    lazy = pc.predict(Xg.chunk({"lat": 4, "lon": 5}))
    assert isinstance(lazy, LazyGridArray)
    for sel, block in lazy.iter_blocks():  # block by block, then assembled
        assert np.array_equal(np.asarray(block.values), out[:, sel["lat"], sel["lon"]], equal_nan=True)
    outc = np.asarray(lazy.values)
    assert np.array_equal(np.isnan(outc), np.isnan(out)) and np.array_equal(outc[:, live], out[:, live])
