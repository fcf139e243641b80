"""GPU: bcsd_fd_kernel with its request rows read from the row tables cached with the group tables (sd_bcsd_plan.h:
build_row_tables), against the same call deriving the rows in the kernel (SD_FD_NOTAB, development library) and against the
register-tile kernel (SD_FX_NODMA), byte for byte in output and status, and against the oracle.  A 40-year daily calendar: the
only way to whole-lane months (1 200 / 1 240 samples) next to the ragged ones (1 130 / 1 230)."""
import functools

import numpy as np
import pandas as pd
import pytest

import bcsd_oracle as bo
from _cases import assert_close, month_gid

pytestmark = pytest.mark.gpu

T = 14600
CT = 32  # cells of the resident fields the cases take their cells from
ENVS = (("tab", {}), ("notab", {"SD_FD_NOTAB": "1"}), ("regs", {"SD_FX_NODMA": "1"}))


@functools.lru_cache(maxsize=None)
def _gid(start):
    return month_gid(pd.date_range(start, periods=T, freq="D"))


@functools.lru_cache(maxsize=None)
def _fields():
    rng = np.random.default_rng(41)
    full = {k: 14 + 7 * rng.standard_normal((T, CT)) for k in ("X", "y", "Xp")}
    for v in full.values():
        v.setflags(write=False)
    return full


@functools.lru_cache(maxsize=None)
def _oracle(start, c0, n):
    """the oracle on the cells c0 .. c0 + n of the shared fields (computed once per calendar and first cell)"""
    f = _fields()
    return bo.pointwise_fit_predict(0, f["X"][:, c0:c0 + n].copy(), f["y"][:, c0:c0 + n].copy(), f["Xp"][:, c0:c0 + n].copy(), _gid(start),
                                    _gid(start))


def _run(ctx, monkeypatch, full, c0, C, gid, envs=ENVS):
    """bcsd_fit_predict of the cells c0 .. c0 + C of `full` under each switch: {name: (out [T, Ct], status, kernel names)}"""
    Ct = full["y"].shape[1]
    dev = {k: ctx.to_device(np.ascontiguousarray(v)) for k, v in full.items()}
    res = {}
    for name, env in envs:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        big = ctx.to_device(np.full((T, Ct), -777.0))
        ctx.prof_reset()
        ctx.prof_enable(True)
        _, st = ctx.bcsd_fit_predict(0, dev["X"].cells(c0, c0 + C), dev["y"].cells(c0, c0 + C), gid, 12, dev["Xp"].cells(c0, c0 + C), gid,
                                     out=big.cells(c0, c0 + C))
        ctx.prof_enable(False)
        res[name] = (big.to_host(), st, set(ctx.prof()))
        big.free()
        for k_ in env:
            monkeypatch.delenv(k_)
    for d in dev.values():
        d.free()
    return res


def _same_on_every_path(res, c0, C, what):
    ref, st_ref, kr = res["regs"]
    assert not any(k.startswith("bcsd_fd_kernel") for k in kr), kr
    for name in ("tab", "notab"):
        got, st, kernels = res[name]
        assert "bcsd_fd_kernel" in kernels and "bcsd_fd_kernel_ragged" in kernels, (name, kernels)
        assert not any(k.startswith("bcsd_fx_kernel") for k in kernels), (name, kernels)
        assert np.array_equal(st, st_ref), f"{what}: status of {name} differs from the register-tile kernel"
        assert got.tobytes() == ref.tobytes(), f"{what}: {name} differs from the register-tile kernel"
    assert (np.delete(ref, np.s_[c0:c0 + C], axis=1) == -777.0).all()  # neighbours of the view untouched
    return ref, st_ref


# one tile; three tiles; a last tile shifted back over its predecessor (the late y rows follow the column, not the wave); a cell view
# with a larger even leading dimension
@pytest.mark.parametrize("C,c0,Ct", [(8, 0, 8), (24, 0, 24), (22, 0, 22), (24, 4, 32)])
def test_tables_against_derived_rows_and_register_tiles(dev_ctx, monkeypatch, C, c0, Ct):
    start = "1980-01-01"
    full = {k: v[:, :Ct] for k, v in _fields().items()}
    res = _run(dev_ctx, monkeypatch, full, c0, C, _gid(start))
    ref, st_ref = _same_on_every_path(res, c0, C, f"C={C} c0={c0} ld={Ct}")
    exp, est = _oracle(start, c0, 4)
    assert np.array_equal(st_ref[:4], est)
    assert_close(ref[:, c0:c0 + 4], exp, what=f"C={C} c0={c0} ld={Ct} vs oracle")


def _masked(f, gid):
    f["X"][0, 9] = np.nan  # the mask is read off the first time step


def _nan_x_hist(f, gid):
    f["X"][T - 3, 9] = np.nan


def _inf_y_obs(f, gid):
    f["y"][4321, 9] = np.inf


def _tied_x_fut(f, gid):
    rows = np.flatnonzero(gid == 6)[100:130]  # a constant stretch inside one July: equal windows, exactly tied shifted samples
    f["Xp"][rows, 9] = f["Xp"][rows[0], 9]


@pytest.mark.parametrize("spoil,code", [(_masked, None), (_nan_x_hist, None), (_inf_y_obs, None), (_tied_x_fut, 0)])
def test_rare_paths(dev_ctx, monkeypatch, spoil, code):
    """a masked cell, a non-finite x_hist, a non-finite y_obs, a tie in x_fut (the item goes to the work list): cell 9, second tile"""
    start, C = "1980-01-01", 24
    gid = _gid(start)
    full = {k: v[:, :C].copy() for k, v in _fields().items()}
    spoil(full, gid)
    res = _run(dev_ctx, monkeypatch, full, 0, C, gid)
    ref, st_ref = _same_on_every_path(res, 0, C, spoil.__name__)
    exp, est = bo.pointwise_fit_predict(0, full["X"][:, 8:10].copy(), full["y"][:, 8:10].copy(), full["Xp"][:, 8:10].copy(), gid, gid)
    assert np.array_equal(st_ref[8:10], est), (st_ref[8:10], est)
    assert est[0] == 0 and (est[1] == 0 if code == 0 else est[1] != 0), est
    ok = est == 0
    assert_close(ref[:, 8:10][:, ok], exp[:, ok], what=f"{spoil.__name__} vs oracle")
    assert np.isnan(ref[:, 8:10][:, ~ok]).all()


def test_cached_tables_follow_their_calendar(dev_ctx, monkeypatch):
    """a second calendar (one year on: other month lengths, other rows), then the first again; then enough other group tables to
    evict both, and the first once more (tables rebuilt): every call equals the one that derives its rows in the kernel"""
    ctx, C = dev_ctx, 16
    full = {k: v[:, :C] for k, v in _fields().items()}
    envs = ENVS[:2]

    def call(start):
        res = _run(ctx, monkeypatch, full, 0, C, _gid(start), envs)
        (got, st, kernels), (ref, st_ref, _) = res["tab"], res["notab"]
        assert "bcsd_fd_kernel" in kernels and "bcsd_fd_kernel_ragged" in kernels, kernels
        assert np.array_equal(st, st_ref) and got.tobytes() == ref.tobytes(), f"calendar from {start}: tables differ from derived rows"
        return got

    a, b = "1980-01-01", "1981-01-01"
    assert not np.array_equal(_gid(a), _gid(b))
    first = call(a)
    second = call(b)
    assert first.tobytes() != second.tobytes()
    assert call(a).tobytes() == first.tobytes()
    small = {k: ctx.to_device(np.ascontiguousarray(v[:400, :8])) for k, v in full.items()}
    for i in range(10):  # more group tables than the cache holds
        g = ((np.arange(400) + i) // 34 % 12).astype(np.int32)
        ctx.bcsd_fit_predict(0, small["X"], small["y"], g, 12, small["Xp"], g)
    for d in small.values():
        d.free()
    assert call(a).tobytes() == first.tobytes()
    assert call(b).tobytes() == second.tobytes()
    exp, est = _oracle(a, 0, 4)
    assert (est == 0).all()
    assert_close(first[:, :4], exp, what="first calendar vs oracle")
