"""GPU parity of PiecewiseLinearRegression(fit_option='arrm') (csrc/sd_arrm.hip) where tests/test_gpu_arrm.py does not go: every
break count (max_breakpoints 2 .. 17, so the 128-thread form of arrm_accum_kernel with its LDS beyond 64 KB and the empty hinge
loops of B = 2), the shortest series (the wrap of the mask, a negative start of the lower loop, picks on the sentinels 1.0 / 2.0,
up to 14 redundant hinges in the null-space correction of arrm_solve_kernel, and the cells on which the reference raises),
half-to-even and odd window widths, the slice boundaries of the accumulate pass, the longest series whose r2 row fits the LDS, and
arrm_predict_kernel on hand-made states.

The expected numbers are the breakpoints recorded from the reference's arrm_breakpoints (tests/golden/g24_arrm_breaks*.npz) and the
NumPy restatement (tests/_arrm_oracle.py) of the fit on them.  The tolerances are those of tests/test_gpu_arrm.py, imported: r2
within R2_TOL, break indices and breaks equal on the cells whose ``margin_computed`` is at least MARGIN (at most MAX_EXCLUDED of the
cells of a case may fall below it), predictions within RTOL of the expected field's std, beta within RTOL * cond * max|beta|, ssr
within 1e-10 of the total sum of squares.

How far the oracle's float64 gelsd solve itself can be trusted at 15 hinges was measured on the CPU against a least-squares solve
in np.longdouble (``_arrm_oracle.predict_longdouble``): the oracle's predictions differ from it by at most 9.3e-14 of their std
over all g24 cases (cond up to 9.9e3), 1.2e-13 at T = 2048 / max_breakpoints 16 (cond 2.8e4) and 7.3e-12 at T = 19 456 /
max_breakpoints 16 (cond 9.2e5).  All are below RTOL / 10 = 1e-10, so RTOL is asserted everywhere as it stands.

A cell whose smallest upper pick is index 6 leaves the empty range r2[:0] to the lower picks; the reference's np.argmin raises
``ValueError: attempt to get argmin of an empty sequence`` there (``raises`` in the goldens).  The engine reports such a cell as
SD_CELL_EMPTY_RANGE with NaN breaks, beta, ssr and predictions and index -1, and fit / arrm_breakpoints / ArrmGridModel /
PointWiseDownscaler raise the reference's error."""
import numpy as np
import pandas as pd
import pytest

import _arrm_oracle as ao
from _cases import assert_close
from test_gpu_arrm import MARGIN, MAX_EXCLUDED, R2_TOL, RTOL

pytestmark = pytest.mark.gpu
EMPTY_RANGE = 5  # SD_CELL_EMPTY_RANGE
PITCH, C0 = 13, 5  # padding of the wider parents of the resident views, first cell of the view


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


@pytest.fixture(scope="module")
def golden():
    return {c: ao.breaks_case(c) for c in ao.CASES_BREAKS}


def resident(ctx, a):
    """a [T, C] on the device as a cells() view of a wider parent: the row pitch is not C"""
    parent = np.full((a.shape[0], a.shape[1] + PITCH), 7.0)
    parent[:, C0:C0 + a.shape[1]] = a
    return ctx.to_device(parent).cells(C0, C0 + a.shape[1])


@pytest.fixture(scope="module")
def fitted(ctx, golden):
    """every case fitted once from host buffers and once from resident fields: (export, r2, predictions on X, predict status) each"""
    res = {}
    for c, g in golden.items():
        st, r2 = ctx.arrm_fit(g["X"], g["y"], g["mb"], with_r2=True)
        out, status = ctx.arrm_predict(st, g["X"])
        host = (st.export(), r2, out, status)
        st.close()
        st, r2 = ctx.arrm_fit(resident(ctx, g["X"]), resident(ctx, g["y"]), g["mb"], with_r2=True)
        out, status = ctx.arrm_predict(st, resident(ctx, g["X"]))
        res[c] = (host, (st.export(), r2.to_host(), out.to_host(), status))
        st.close()
    return res


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("c", ao.CASES_BREAKS)
def test_golden_r2(golden, fitted, c):
    g, r2 = golden[c], fitted[c][0][1]
    live = ~g["raises"]
    exp = g["r2"][:, live]
    assert np.array_equal(np.isnan(r2[:, live]), np.isnan(exp)), f"{c}: NaN positions of r2 differ"
    err = np.abs(r2[:, live] - exp)[~np.isnan(exp)].max()
    print(c, "r2 max err", err)
    assert err <= R2_TOL


@pytest.mark.parametrize("c", ao.CASES_BREAKS)
def test_golden_breaks_and_raising_cells(golden, fitted, c):
    g, (e, _, out, status) = golden[c], fitted[c][0]
    B, raises = 2 * (g["mb"] // 2), g["raises"]
    assert e["breaks"].shape == (B, len(raises)) and e["T"] == len(g["X"])
    print(c, "raising cells", np.flatnonzero(raises), "engine status", e["status"])
    assert np.array_equal(e["status"], np.where(raises, EMPTY_RANGE, 0)) and np.array_equal(status, e["status"])
    assert np.isnan(e["breaks"][:, raises]).all() and np.isnan(e["beta"][:, raises]).all() and np.isnan(e["ssr"][raises]).all()
    assert (e["break_index"][:, raises] == -1).all() and np.isnan(out[:, raises]).all() and np.isfinite(out[:, ~raises]).all()
    keep = ~raises & ~(g["margin_computed"] < MARGIN)
    print(c, "cells left out by margin_computed", int((~raises & ~keep).sum()), "of", int((~raises).sum()))
    assert (~raises & ~keep).sum() <= MAX_EXCLUDED * (~raises).sum()
    assert np.array_equal(e["break_index"][:, keep], g["index"][:, keep])
    assert np.array_equal(e["breaks"][:, keep], g["breaks"][:, keep])


@pytest.mark.parametrize("c", ao.CASES_BREAKS)
def test_golden_predictions_beta_ssr(golden, fitted, c):
    g, (e, _, out, _) = golden[c], fitted[c][0]
    keep = ~g["raises"] & ~(g["margin_computed"] < MARGIN)
    print(c, "pred err / std", np.abs(out - g["pred"])[:, keep].max() / np.std(g["pred"][:, keep]))
    assert_close(out[:, keep], g["pred"][:, keep], rtol=RTOL, what=f"{c} pred")
    err = np.abs(e["beta"] - g["beta"])[:, keep].max(axis=0)
    bound = RTOL * g["cond"][keep] * np.abs(g["beta"][:, keep]).max(axis=0)
    print(c, "beta err / bound", (err / bound).max())
    assert (err <= bound).all()
    ssr_err = np.abs(e["ssr"] - g["ssr"])[keep]
    tss = np.sum((g["y"] - g["y"].mean(axis=0)) ** 2, axis=0)[keep]
    print(c, "ssr err / total sum of squares", (ssr_err / tss).max())
    assert (ssr_err <= 1e-10 * tss).all()


@pytest.mark.parametrize("c", ao.CASES_BREAKS)
def test_golden_resident_fields_are_bit_identical(fitted, c):
    (e, r2, out, status), (e_d, r2_d, out_d, status_d) = fitted[c]
    for k in ("breaks", "break_index", "beta", "ssr", "status"):
        assert same(e[k], e_d[k]), k
    assert same(r2, r2_d) and same(out, out_d) and same(status, status_d)


@pytest.mark.parametrize("c", ["mb2_300", "mb17_1000", "short50_mb16"])
def test_export_import_predict_is_bit_identical(ctx, golden, fitted, c):
    """B = 2, B = 16, and a state with SD_CELL_EMPTY_RANGE cells: the code survives export -> import"""
    g, (e, _, out, status) = golden[c], fitted[c][0]
    st = ctx.arrm_import(e)
    e2 = st.export()
    out2, status2 = ctx.arrm_predict(st, g["X"])
    st.close()
    assert same(out, out2) and same(status, status2) and e2["T"] == e["T"]
    for k in ("breaks", "break_index", "beta", "ssr", "status"):
        assert same(e[k], e2[k]), k


def test_raising_cell_raises_in_python(golden):
    from skdownscale_amd import ArrmGridModel, GridArray, PiecewiseLinearRegression, PointWiseDownscaler, arrm_breakpoints

    g = golden["short50_mb8"]  # (the reference raises on cells 6 and 7 of its 24)
    bad, good = int(np.flatnonzero(g["raises"])[0]), int(np.flatnonzero(~g["raises"] & ~(g["margin_computed"] < MARGIN))[0])
    X, y, mb = g["X"], g["y"], g["mb"]
    message = "^attempt to get argmin of an empty sequence$"
    with pytest.raises(ValueError, match=message):
        PiecewiseLinearRegression(n_segments=mb, fit_option="arrm").fit(X[:, bad:bad + 1], y[:, bad])
    with pytest.raises(ValueError, match=message):
        arrm_breakpoints(X[:, bad:bad + 1], y[:, bad], 0.05, mb)
    with pytest.raises(ValueError, match=message):
        ArrmGridModel(mb).fit(X, y)
    m = PiecewiseLinearRegression(n_segments=mb, fit_option="arrm").fit(X[:, good:good + 1], y[:, good])
    assert np.array_equal(m.fit_breaks_, g["breaks"][:, good])
    assert np.array_equal(arrm_breakpoints(X[:, good:good + 1], y[:, good], 0.05, mb), g["breaks"][:, good])
    T, ny, nx = X.shape[0], 4, 6
    coords = {"time": pd.date_range("2001-01-01", periods=T), "lat": np.arange(ny), "lon": np.arange(nx)}

    def grid(a):
        return GridArray(a.reshape(T, ny, nx).copy(), ("time", "lat", "lon"), coords)

    def downscaler():
        return PointWiseDownscaler(PiecewiseLinearRegression(n_segments=mb, fit_option="arrm"))

    with pytest.raises(ValueError, match=message):
        downscaler().fit(grid(X), grid(y))
    Xn = X.copy()
    Xn[25, bad - 2] = np.nan  # the reference's loop over the cells meets this one first
    with pytest.raises(ValueError, match="Input X contains NaN"):
        downscaler().fit(grid(Xn), grid(y))
    Xn[25, bad - 2], Xn[25, bad + 3] = X[25, bad - 2], np.nan  # ... and this one after the cell it fails on
    with pytest.raises(ValueError, match=message):
        downscaler().fit(grid(Xn), grid(y))
    Xm = X.copy()
    Xm[0, g["raises"]] = np.nan  # masked cells are skipped by the reference's loop: nothing raises
    pw = downscaler()
    pw.fit(grid(Xm), grid(y))
    out = np.asarray(pw.predict(grid(Xm)).values).reshape(T, -1)
    assert np.isnan(out[:, g["raises"]]).all() and np.isfinite(out[:, ~g["raises"]]).all()


def gaussian(seed, T, C):
    rng = np.random.default_rng(seed)
    X = 15.0 + 8.0 * rng.normal(size=(T, C))
    return X, 13.0 + 0.9 * X + 0.05 * X * X + 3.0 * rng.normal(size=(T, C))


def check_against_the_oracle(what, X, y, mb, e, r2, out, cells):
    """the cells ``cells`` of a fit (export e, r2, predictions out on X): r2 and, where margin_computed allows, the picks against
    ao.breakpoints; beta, ssr and the predictions against ao.fit_on_breaks on the engine's own breaks (the fit is checked whatever
    the picks are)"""
    worst = dict(r2=0.0, pred=0.0, beta=0.0, ssr=0.0, left_out=0)
    for k in cells:
        o = ao.breakpoints(X[:, k], y[:, k], 0.05, mb)
        assert np.array_equal(np.isnan(r2[:, k]), np.isnan(o["r2"])), (what, k)
        err = np.abs(r2[:, k] - o["r2"])[~np.isnan(o["r2"])].max()
        worst["r2"] = max(worst["r2"], err)
        assert err <= R2_TOL, (what, k, err)
        if o["margin_computed"] >= MARGIN:
            assert np.array_equal(e["break_index"][:, k], o["index"]) and np.array_equal(e["breaks"][:, k], o["breaks"]), (what, k)
        else:
            worst["left_out"] += 1
        beta, ssr, cond = ao.fit_on_breaks(X[:, k], y[:, k], e["breaks"][:, k])
        exp = ao.predict(X[:, k], e["breaks"][:, k], beta)
        worst["pred"] = max(worst["pred"], np.abs(out[:, k] - exp).max() / np.std(exp))
        worst["beta"] = max(worst["beta"], np.abs(e["beta"][:, k] - beta).max() / (RTOL * cond * np.abs(beta).max()))
        worst["ssr"] = max(worst["ssr"], abs(e["ssr"][k] - ssr) / np.sum((y[:, k] - y[:, k].mean()) ** 2))
        assert_close(out[:, k], exp, rtol=RTOL, what=f"{what} cell {k} pred")
        assert (np.abs(e["beta"][:, k] - beta) <= RTOL * cond * np.abs(beta).max()).all(), (what, k)
        assert abs(e["ssr"][k] - ssr) <= 1e-10 * np.sum((y[:, k] - y[:, k].mean()) ** 2), (what, k)
    print(what, "r2 max err %.3g, pred err / std %.3g, beta err / bound %.3g, ssr err / tss %.3g, cells left out %d of %d"
          % (worst["r2"], worst["pred"], worst["beta"], worst["ssr"], worst["left_out"], len(cells)))
    return worst


@pytest.mark.parametrize("mb", [7, 16])
@pytest.mark.parametrize("T", [255, 256, 257, 511, 512, 1023, 1024, 1025, 2047, 2048])
def test_accumulate_slices_and_cell_tiles(ctx, T, mb):
    """The time slices of arrm_accum_kernel change at T / 256 (256 threads, B <= 6) and T / 128 (128 threads above), up to 8: every
    T here sits on or next to a boundary of one of the two.  C = 67 is a full 64-cell tile and a ragged one; cell 1 is masked (its
    first X is NaN), cell 65 has an inf in y.  Six cells against the oracle (a Python loop): the first and the last, both sides of
    the tile edge, the neighbours of the planted cells; the others must be OK and finite."""
    C, MASKED, INF = 67, 1, 65
    X, y = gaussian(1000 * mb + T, T, C)
    X[0, MASKED] = np.nan
    y[T // 3, INF] = np.inf
    st, r2 = ctx.arrm_fit(X, y, mb, with_r2=True)
    e = st.export()
    out, status = ctx.arrm_predict(st, np.where(np.isnan(X), 0.0, X))
    st.close()
    expected = np.zeros(C, dtype=np.int32)
    expected[MASKED], expected[INF] = 1, 2
    assert np.array_equal(e["status"], expected) and np.array_equal(status, expected)
    ok = expected == 0
    assert np.isfinite(out[:, ok]).all() and np.isfinite(e["beta"][:, ok]).all() and np.isfinite(e["ssr"][ok]).all()
    assert np.isfinite(e["breaks"][:, ok]).all() and (e["break_index"][:, ok] >= 0).all() and (e["break_index"][:, ok] < T).all()
    assert (np.diff(e["break_index"][:, ok], axis=0) >= 0).all()
    assert np.isnan(out[:, ~ok]).all() and np.isnan(e["beta"][:, ~ok]).all() and (e["break_index"][:, ~ok] == -1).all()
    worst = check_against_the_oracle(f"T={T} mb={mb}", X, y, mb, e, r2, out, [0, 2, 63, 64, 66, 33])
    assert worst["left_out"] == 0  # (the oracle's margin_computed of these seeded cells is 2.5e-5 at the least: none is left out)


@pytest.mark.parametrize("mb", [7, 16])
def test_longest_series(ctx, mb):
    """T = 19 456: 8 T + 8192 bytes are the 160 KB of LDS exactly.  Two cells against the oracle (about a second each on the CPU);
    at max_breakpoints 16 the design's condition number is 9e5 and the oracle's own error 7.3e-12 of the std (module docstring)."""
    T, C = 19456, 2
    X, y = gaussian(19457, T, C)  # (a seed whose two cells have a margin_computed of 5e-6 and more at either break count)
    st, r2 = ctx.arrm_fit(X, y, mb, with_r2=True)
    e = st.export()
    out, status = ctx.arrm_predict(st, X)
    st.close()
    assert (e["status"] == 0).all() and (status == 0).all()
    assert check_against_the_oracle(f"T={T} mb={mb}", X, y, mb, e, r2, out, range(C))["left_out"] == 0


def test_one_sample_too_long_is_refused(ctx):
    T, C = 19457, 2
    X, y = gaussian(19457, T, C)
    with pytest.raises(NotImplementedError, match="the r2 series of 19457 samples does not fit in LDS"):
        ctx.arrm_fit(X, y, 7)
    with pytest.raises(NotImplementedError, match="the r2 series of 19457 samples does not fit in LDS"):
        ctx.arrm_fit(resident(ctx, X), resident(ctx, y), 16, with_r2=True)
    st = ctx.arrm_fit(X[:60], y[:60], 7)  # the context is as good as before
    assert (st.export()["status"] == 0).all()
    st.close()


def handmade_state(B, C, seed):
    """breaks [B, C] ascending with duplicates (b[2] == b[1] and, from B = 6 on, three equal ones) and, in every other cell, a
    first hinge at b[0] itself (pwlf's origin, the smallest x of a fit); beta of the order of one"""
    rng = np.random.default_rng(seed)
    breaks = np.sort(rng.normal(15.0, 8.0, size=(B, C)), axis=0)
    if B >= 4:
        breaks[2] = breaks[1]
    if B >= 6:
        breaks[5] = breaks[4] = breaks[3]
        breaks[1, ::2] = breaks[0, ::2]
        breaks[2, ::2] = breaks[0, ::2]
    beta = rng.normal(0.0, 1.0, size=(B, C))
    return dict(breaks=breaks, break_index=np.full((B, C), -1, dtype=np.int32), beta=beta, ssr=np.zeros(C), status=np.zeros(C, np.int32), T=0)


@pytest.mark.parametrize("Tq", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("C", [1, 64, 65])
@pytest.mark.parametrize("B", [2, 6, 16])
def test_predict_kernel(ctx, B, C, Tq):
    """arrm_predict_kernel on an imported state: 256 rows per workgroup (Tq on and next to the tile), 64 cells per workgroup, the
    hinge loop empty at B = 2.  The first query lies below the first break, the last above the last one, one query sits on a
    break; cell C // 2 gets a NaN, a +inf and a -inf query (as many as Tq has rows): those rows are NaN and the cell's status is
    2, nothing else changes.  The resident form writes into a cells() view of a wider field whose padding stays as it was."""
    e = handmade_state(B, C, 100 * B + C)
    rng = np.random.default_rng(Tq)
    Xq = rng.normal(15.0, 12.0, size=(Tq, C))
    Xq[0] = e["breaks"][0] - 5.0
    if Tq > 1:
        Xq[-1] = e["breaks"][-1] + 5.0
        Xq[Tq // 2] = e["breaks"][B // 2]
    bad_cell = C // 2
    bad_rows = sorted({Tq // 3, (2 * Tq) // 3, Tq - 1})
    clean = Xq.copy()
    for r, v in zip(bad_rows, (np.nan, np.inf, -np.inf)):
        Xq[r, bad_cell] = v
    exp = np.stack([ao.predict(clean[:, k], e["breaks"][:, k], e["beta"][:, k]) for k in range(C)], axis=1)
    exp[bad_rows, bad_cell] = np.nan
    exp_status = np.zeros(C, dtype=np.int32)
    exp_status[bad_cell] = 2
    st = ctx.arrm_import(e)
    out, status = ctx.arrm_predict(st, Xq)
    parent = ctx.to_device(np.full((Tq, C + PITCH), 7.0))
    out_d, status_d = ctx.arrm_predict(st, resident(ctx, Xq), out=parent.cells(C0, C0 + C))
    st.close()
    assert np.array_equal(status, exp_status) and np.array_equal(status_d, exp_status)
    assert np.array_equal(np.isnan(out), np.isnan(exp))
    if np.isfinite(exp).any():
        print(f"B={B} C={C} Tq={Tq} pred err / std", np.nanmax(np.abs(out - exp)) / np.nanstd(exp))
    assert_close(out, exp, rtol=RTOL, what="predict")
    whole = parent.to_host()
    assert same(whole[:, C0:C0 + C], out) and (whole[:, :C0] == 7.0).all() and (whole[:, C0 + C:] == 7.0).all()
    assert out_d.ld == C + PITCH
