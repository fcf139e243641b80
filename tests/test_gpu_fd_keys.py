"""GPU: bcsd_fd_kernel with the four-instruction key assembly, the pad keys written under the exec mask of the lanes past the data,
tag addresses taken straight from the keys and the finite tests made on the sums (sd_bcsd_fx.hip, formulas in sd_bcsd_plan.h), against
the register-tile kernel (SD_FX_NODMA, development library), byte for byte in output and status, and against the oracle.  A 40-year
daily calendar: the kernel takes segments of 641 .. 1 280 samples (whole-lane months of 1 200 / 1 240, ragged ones of 1 130 / 1 230)."""
import functools

import numpy as np
import pandas as pd
import pytest

import bcsd_oracle as bo
from _cases import assert_close, month_gid

pytestmark = pytest.mark.gpu

T = 14600
CT = 32  # cells of the shared fields
ENVS = (("dma", {}), ("regs", {"SD_FX_NODMA": "1"}))


@functools.lru_cache(maxsize=None)
def _gid():
    return month_gid(pd.date_range("1980-01-01", periods=T, freq="D"))


@functools.lru_cache(maxsize=None)
def _fields():
    rng = np.random.default_rng(53)
    full = {k: 14 + 7 * rng.standard_normal((T, CT)) for k in ("X", "y", "Xp")}
    for v in full.values():
        v.setflags(write=False)
    return full


@functools.lru_cache(maxsize=None)
def _oracle(c0, n):
    f = _fields()
    return bo.pointwise_fit_predict(0, f["X"][:, c0:c0 + n].copy(), f["y"][:, c0:c0 + n].copy(), f["Xp"][:, c0:c0 + n].copy(), _gid(), _gid())


def _run(ctx, monkeypatch, full, c0, C):
    """bcsd_fit_predict of the cells c0 .. c0 + C of `full` on either kernel: {name: (out [T, Ct], status, kernel names)}"""
    Ct = full["y"].shape[1]
    dev = {k: ctx.to_device(np.ascontiguousarray(v)) for k, v in full.items()}
    res = {}
    for name, env in ENVS:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        big = ctx.to_device(np.full((T, Ct), -777.0))
        ctx.prof_reset()
        ctx.prof_enable(True)
        _, st = ctx.bcsd_fit_predict(0, dev["X"].cells(c0, c0 + C), dev["y"].cells(c0, c0 + C), _gid(), 12, dev["Xp"].cells(c0, c0 + C), _gid(),
                                     out=big.cells(c0, c0 + C))
        ctx.prof_enable(False)
        res[name] = (big.to_host(), st, set(ctx.prof()))
        big.free()
        for k_ in env:
            monkeypatch.delenv(k_)
    for d in dev.values():
        d.free()
    return res


def _same_as_register_tiles(res, c0, C, what):
    (got, st, kernels), (ref, st_ref, kr) = res["dma"], res["regs"]
    assert not any(k.startswith("bcsd_fd_kernel") for k in kr), kr
    assert "bcsd_fd_kernel" in kernels and "bcsd_fd_kernel_ragged" in kernels, kernels
    assert not any(k.startswith("bcsd_fx_kernel") for k in kernels), kernels
    assert np.array_equal(st, st_ref), f"{what}: status differs from the register-tile kernel: {st} / {st_ref}"
    assert got.tobytes() == ref.tobytes(), f"{what}: output differs from the register-tile kernel"
    assert (np.delete(got, np.s_[c0:c0 + C], axis=1) == -777.0).all()  # neighbours of the view untouched
    return got, st


# one tile; three tiles; a last tile shifted back over its predecessor; a cell view with a larger even leading dimension
@pytest.mark.parametrize("C,c0,Ct", [(8, 0, 8), (24, 0, 24), (22, 0, 22), (24, 4, 32)])
def test_against_register_tiles_and_oracle(dev_ctx, monkeypatch, C, c0, Ct):
    full = {k: v[:, :Ct] for k, v in _fields().items()}
    got, st = _same_as_register_tiles(_run(dev_ctx, monkeypatch, full, c0, C), c0, C, f"C={C} c0={c0} ld={Ct}")
    exp, est = _oracle(c0, 4)
    assert np.array_equal(st[:4], est)
    assert_close(got[:, c0:c0 + 4], exp, what=f"C={C} c0={c0} ld={Ct} vs oracle")


def _nan_y_obs(f, gid):
    f["y"][7777, 9] = np.nan


def _inf_x_hist(f, gid):
    f["X"][T - 3, 9] = -np.inf


def _masked(f, gid):
    f["X"][0, 9] = np.nan  # the mask is read off the first time step


def _all_equal_x_fut(f, gid):
    f["Xp"][:, 9] = 3.25  # every shifted sample of a month equal: every key ties


def _tied_x_fut(f, gid):
    rows = np.flatnonzero(gid == 6)[100:130]  # a constant stretch inside one July: equal windows, exactly tied shifted samples
    f["Xp"][rows, 9] = f["Xp"][rows[0], 9]


@pytest.mark.parametrize("spoil,clean", [(_nan_y_obs, False), (_inf_x_hist, False), (_masked, False), (_all_equal_x_fut, True), (_tied_x_fut, True)])
def test_rare_paths(dev_ctx, monkeypatch, spoil, clean):
    """cell 9 (second tile): a NaN among the observations and an infinity in x_hist (the sums are non-finite: the per-value tests set
    the status), a masked cell, ties of every key and of a stretch of x_fut (the item goes to the work list)"""
    C, gid = 24, _gid()
    full = {k: v[:, :C].copy() for k, v in _fields().items()}
    spoil(full, gid)
    got, st = _same_as_register_tiles(_run(dev_ctx, monkeypatch, full, 0, C), 0, C, spoil.__name__)
    exp, est = bo.pointwise_fit_predict(0, full["X"][:, 8:10].copy(), full["y"][:, 8:10].copy(), full["Xp"][:, 8:10].copy(), gid, gid)
    assert np.array_equal(st[8:10], est), (st[8:10], est)
    assert est[0] == 0 and (est[1] == 0) == clean, est
    ok = est == 0
    assert_close(got[:, 8:10][:, ok], exp[:, ok], what=f"{spoil.__name__} vs oracle")
    assert np.isnan(got[:, 8:10][:, ~ok]).all()


def test_finite_observations_whose_sum_overflows(dev_ctx, monkeypatch):
    """+-1e308 among the observations of cell 9: a lane's sum and the climatology sum overflow, the per-value tests find nothing -- the
    status stays clean, and the result is the register-tile kernel's, which tests every value"""
    C, gid = 24, _gid()
    full = {k: v[:, :C].copy() for k, v in _fields().items()}
    july, feb = np.flatnonzero(gid == 6), np.flatnonzero(gid == 1)  # a whole-lane month and a ragged one
    for rows in (july, feb):
        full["y"][rows[40:43], 9] = 1e308  # three neighbours of one lane: 3e308 overflows
        full["y"][rows[700:702], 9] = -1e308
    with np.errstate(over="ignore"):
        assert np.isinf(full["y"][july[40:60], 9].sum()) and np.isfinite(full["y"][:, 9]).all()
    got, st = _same_as_register_tiles(_run(dev_ctx, monkeypatch, full, 0, C), 0, C, "overflowing sum")
    assert (st == 0).all(), st
    # the other cells of the tile are the oracle's
    exp, est = bo.pointwise_fit_predict(0, full["X"][:, 10:12].copy(), full["y"][:, 10:12].copy(), full["Xp"][:, 10:12].copy(), gid, gid)
    assert (est == 0).all()
    assert_close(got[:, 10:12], exp, what="neighbours of the overflowing cell vs oracle")
