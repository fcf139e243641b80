"""GPU: bcsd_fd_kernel on segments whose length is not a multiple of 20 (the RAG instantiation: February and December of a daily
series, and any length the launcher admits) against the register-tile kernel (SD_FX_NODMA) bit for bit, and against the oracle."""
import numpy as np
import pandas as pd
import pytest

import bcsd_oracle as bo
from _cases import assert_close, month_gid

pytestmark = pytest.mark.gpu

ENVS = (("dma", {}), ("regs", {"SD_FX_NODMA": "1"}))


def _run_variants(ctx, monkeypatch, full, c0, C, gid, G, gid_p=None):
    """bcsd_fit_predict of the cells c0 .. c0 + C of the resident fields under each switch: {name: (out, status, kernels)}"""
    gid_p = gid if gid_p is None else gid_p
    T, Ct = full["y"].shape
    dev = {k: ctx.to_device(v) for k, v in full.items()}
    res = {}
    for name, env in ENVS:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        big = ctx.to_device(np.full((T, Ct), -777.0))
        ctx.prof_reset()
        ctx.prof_enable(True)
        _, st = ctx.bcsd_fit_predict(0, dev["X"].cells(c0, c0 + C), dev["y"].cells(c0, c0 + C), gid, G, dev["Xp"].cells(c0, c0 + C), gid_p,
                                     out=big.cells(c0, c0 + C))
        ctx.prof_enable(False)
        res[name] = (big.to_host(), st, set(ctx.prof()))
        big.free()
        for k_ in env:
            monkeypatch.delenv(k_)
    for d in dev.values():
        d.free()
    return res


def _check(res, c0, C, what):
    ref, st_ref, kr = res["regs"]
    assert not any(k.startswith("bcsd_fd_kernel") for k in kr), kr
    got, st, kernels = res["dma"]
    assert "bcsd_fd_kernel_ragged" in kernels, kernels
    assert not any(k.startswith("bcsd_fx_kernel") for k in kernels), kernels
    assert np.array_equal(st, st_ref), what
    assert np.array_equal(got, ref, equal_nan=True), f"{what}: dma differs from the register-tile kernel"
    assert (np.delete(ref, np.s_[c0:c0 + C], axis=1) == -777.0).all()  # neighbours of the view untouched
    return ref, st_ref


# lengths with m % 20 = 1, 10, 16, 17, 19 (long and short lanes of data), next to whole-lane groups and one below full_min_len
LENS = [1101, 1130, 1136, 1137, 1139, 1230, 1240, 1200, 661, 679, 700]


@pytest.mark.parametrize("C,c0,Ct", [(8, 0, 8), (26, 0, 26), (22, 4, 30)])
@pytest.mark.parametrize("scatter", [False, True])
def test_ragged_segments_on_the_dma_kernel(dev_ctx, monkeypatch, C, c0, Ct, scatter):
    ctx = dev_ctx
    rng = np.random.default_rng(7 + C + 100 * scatter)
    G = len(LENS)
    T = sum(LENS)
    gid = np.repeat(np.arange(G), LENS).astype(np.int32)
    if scatter:
        gid = gid[rng.permutation(T)]  # members of a group anywhere in time
    full = {k: 15 + 8 * rng.standard_normal((T, Ct)) for k in ("X", "y", "Xp")}
    sl = slice(c0, c0 + C)
    X, y, Xp = (full[k][:, sl] for k in ("X", "y", "Xp"))
    if C > 8:
        X[0, 1] = np.nan                   # masked cell
        X[T - 1, 3] = np.inf               # non-finite x_hist
        y[T - 2, C - 3] = np.nan           # non-finite y_obs
        Xp[T - 1, C - 1] = -np.inf         # non-finite x_fut in the last cell (the ragged tile)
        last = np.flatnonzero(gid == 1)     # m = 1 130: a constant stretch at the end -> exactly tied shifted samples
        Xp[last[-30:], 5] = Xp[last[-30], 5]
        first = np.flatnonzero(gid == 4)    # m = 1 139
        Xp[first[:25], C - 2] = Xp[first[0], C - 2]
    res = _run_variants(ctx, monkeypatch, full, c0, C, gid, G)
    ref, st_ref = _check(res, c0, C, f"ragged C={C}")
    n = min(C, 6)
    exp, est = bo.pointwise_fit_predict(0, X[:, :n].copy(), y[:, :n].copy(), Xp[:, :n].copy(), gid, gid, G=G)
    assert np.array_equal(st_ref[:n], est)
    ok = est == 0
    assert_close(ref[:, sl][:, :n][:, ok], exp[:, ok], what="ragged DMA kernel vs oracle")


def test_ragged_months_of_a_daily_series(dev_ctx, monkeypatch):
    """40 years of daily data: February (1 130 samples) and December (1 230) take the RAG instantiation."""
    ctx = dev_ctx
    rng = np.random.default_rng(3)
    T, C = 14600, 16
    index = pd.date_range("1980-01-01", periods=T, freq="D")
    gid = month_gid(index)
    full = {k: 12 + 6 * rng.standard_normal((T, C)) for k in ("X", "y", "Xp")}
    for v in full.values():
        v[:, 8:] = np.round(v[:, 8:] * 64) / 64  # coarse values in the second tile: exact ties in most months (work list)
    res = _run_variants(ctx, monkeypatch, full, 0, C, gid, 12)
    ref, st_ref = _check(res, 0, C, "daily")
    exp, est = bo.pointwise_fit_predict(0, full["X"][:, :4], full["y"][:, :4], full["Xp"][:, :4], gid, gid)
    assert np.array_equal(st_ref[:4], est)
    assert_close(ref[:, :4], exp, what="daily series vs oracle")


def test_daily_fit_predict_launches_no_register_tile_kernel():
    """The default (production) build: a 40-year daily BcsdTemperature fit + predict runs on bcsd_fd_kernel alone."""
    from skdownscale_amd.engine import default_context

    ctx = default_context()
    T, C = 14600, 64
    index = pd.date_range("1980-01-01", periods=T, freq="D")
    gid = month_gid(index)
    rng = np.random.default_rng(5)
    X, y, Xp = (ctx.to_device(10 + 5 * rng.standard_normal((T, C))) for _ in range(3))
    ctx.prof_reset()
    ctx.prof_enable(True)
    out, st = ctx.bcsd_fit_predict(0, X, y, gid, 12, Xp, gid)
    ctx.prof_enable(False)
    kernels = ctx.prof()
    assert "bcsd_fd_kernel" in kernels and "bcsd_fd_kernel_ragged" in kernels, kernels
    assert not any(k.startswith("bcsd_fx_kernel") for k in kernels), kernels
    assert (st == 0).all()
    exp, _ = bo.pointwise_fit_predict(0, X.to_host()[:, :4], y.to_host()[:, :4], Xp.to_host()[:, :4], gid, gid)
    assert_close(out.to_host()[:, :4], exp, what="daily fit + predict vs oracle")
