"""GPU: the y side of bcsd_fd_kernel -- every cell's second-level keys in five whole chunks of the tile, the late chunks of y
requested by the wave whose cell they cover, the vote on the fix-up of u read behind the barrier of the y tile.

A 40-year daily calendar (T = 14 600: months of 1 240, 1 200, 1 130 and 1 230 samples, both instantiations) on 8, 10 and 26 cells;
10 and 26 cells end in a tile fetched shifted back over its predecessor, where a wave's column is not its number.  Against the
oracle (1e-6 relative, the tolerance of the fused path in test_gpu_bcsd.py) with the status codes, and bit for bit against the
register-tile kernel on the development library."""
import numpy as np
import pandas as pd
import pytest

import bcsd_oracle as bo
from _cases import assert_close, month_gid

pytestmark = pytest.mark.gpu

T = 14600
CELLS = (8, 10, 26)
GID = month_gid(pd.date_range("1980-01-01", periods=T, freq="D"))
Y_TIES, BAD_XP, BAD_Y, MASKED = 2, 3, 4, 5  # cells of the first tile; the tied x_fut cell is the grid's last one


def _continuous(C):
    rng = np.random.default_rng(900 + C)
    return tuple(15 + 8 * rng.standard_normal((T, C)) for _ in range(3))


def _special(C):
    """Cells 0, 1, 6 and C - 2 stay clean: the first and the last tile hold live, continuous cells next to the others."""
    X, y, Xp = _continuous(C)
    # constant stretches of x_fut: where nine or more constant days lie inside one month the rolling mean equals the sample and
    # the shifted samples tie exactly -- in May (1 240 samples, whole lanes), December (1 230) and February (1 130)
    Xp[125:150, C - 1] = Xp[125, C - 1]
    Xp[4000:4024, C - 1] = Xp[4000, C - 1]
    Xp[770:795, C - 1] = Xp[770, C - 1]
    y[:, Y_TIES] = np.round(y[:, Y_TIES] * 2) / 2  # tied observations in every month
    Xp[9000, BAD_XP] = -np.inf
    y[5000, BAD_Y] = np.nan
    X[0, MASKED] = np.nan
    return X, y, Xp


def _tied_months(xp):
    """months in which the shifted samples u = x_fut - (rolling mean - x_climo) of a cell hold exact duplicates: the
    position tags cannot rank them, the second-level keys compare equal and the item goes to the work list"""
    tied = set()
    for g in range(12):
        seg = xp[GID == g]
        u = seg - bo.rolling_mean_centered(seg)
        if len(np.unique(u)) < len(u):
            tied.add(g)
    return tied


_cache = {}


def _case(name, C, ra):
    """inputs, expected field and status of a case (computed once)"""
    key = (name, C)
    if key not in _cache:
        X, y, Xp = (_continuous if name == "continuous" else _special)(C)
        _cache[key] = {"in": (X, y, Xp)}
    e = _cache[key]
    if ra not in e:
        e[ra] = bo.pointwise_fit_predict(bo.TAS, *e["in"], GID, GID, return_anoms=ra)
        for a in e[ra]:
            a.setflags(write=False)
    return e["in"], e[ra][0], e[ra][1]


def _engine(ctx, inputs, ra):
    X, y, Xp = (ctx.to_device(v) for v in inputs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    out, st = ctx.bcsd_fit_predict(0, X, y, GID, 12, Xp, GID, ra)
    ctx.prof_enable(False)
    kernels = set(ctx.prof())
    print("kernels:", sorted(kernels))
    assert "bcsd_fd_kernel" in kernels and "bcsd_fd_kernel_ragged" in kernels, kernels
    assert not any(k.startswith("bcsd_fx_kernel") for k in kernels), kernels
    got = out.to_host()
    for d in (X, y, Xp, out):
        d.free()
    return got, st


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


def _check(got, st, exp, est, what):
    assert np.array_equal(st, est), (what, st, est)
    ok = est == 0
    assert np.isnan(got[:, ~ok]).all(), what
    err = np.abs(got[:, ok] - exp[:, ok])
    print(f"{what}: max abs error {np.nanmax(err):.3e} (std of the field {np.std(exp[:, ok]):.3e})")
    assert_close(got[:, ok], exp[:, ok], what=what)


@pytest.mark.parametrize("ra", [True, False])
@pytest.mark.parametrize("C", CELLS)
def test_continuous_data_stays_on_the_fast_path(ctx, C, ra):
    inputs, exp, est = _case("continuous", C, ra)
    assert (est == 0).all()
    assert not any(_tied_months(inputs[2][:, c]) for c in range(C))  # nothing for the work list
    got, st = _engine(ctx, inputs, ra)
    _check(got, st, exp, est, f"continuous C={C} return_anoms={ra}")


@pytest.mark.parametrize("ra", [True, False])
@pytest.mark.parametrize("C", CELLS)
def test_ties_bad_and_masked_cells_next_to_live_ones(ctx, C, ra):
    """Exact ties in x_fut in the last cell: its (tile, month) items are handed back behind the barrier of the y tile, after
    the late requests went out; the other cells of the tile come back right from RANK / APPLY, the other months from the
    kernel itself.  Tied observations are interchangeable and stay on the fast path.  The non-finite and the masked cell
    carry their status and NaN.  The next call on the same context is clean again."""
    inputs, exp, est = _case("special", C, ra)
    want = np.zeros(C, dtype=est.dtype)
    want[[BAD_XP, BAD_Y]] = bo.STATUS_NONFINITE
    want[MASKED] = bo.STATUS_MASKED
    assert np.array_equal(est, want)
    # the hand-back is in the data: May of the whole-lane launch, February and December of the ragged one, last cell only.
    # (The profiler names cannot show it: RANK / APPLY are launched over the work list whether it is empty or not.)
    assert _tied_months(inputs[2][:, C - 1]) == {1, 4, 11}
    assert not any(_tied_months(inputs[2][:, c]) for c in range(C - 1) if c != BAD_XP)
    got, st = _engine(ctx, inputs, ra)
    _check(got, st, exp, est, f"special C={C} return_anoms={ra}")
    inputs, exp, est = _case("continuous", C, ra)
    got, st = _engine(ctx, inputs, ra)
    _check(got, st, exp, est, f"continuous after special C={C} return_anoms={ra}")


@pytest.mark.parametrize("C", CELLS)
def test_bit_identical_to_the_register_tile_kernel(dev_ctx, monkeypatch, C):
    """Same arithmetic in the same order as bcsd_fx_kernel (SD_FX_NODMA, development library)."""
    inputs, exp, est = _case("continuous", C, True)
    got, st = _engine(dev_ctx, inputs, True)
    monkeypatch.setenv("SD_FX_NODMA", "1")
    X, y, Xp = (dev_ctx.to_device(v) for v in inputs)
    dev_ctx.prof_reset()
    dev_ctx.prof_enable(True)
    out, st_ref = dev_ctx.bcsd_fit_predict(0, X, y, GID, 12, Xp, GID, True)
    dev_ctx.prof_enable(False)
    monkeypatch.delenv("SD_FX_NODMA")
    kernels = set(dev_ctx.prof())
    assert not any(k.startswith("bcsd_fd_kernel") for k in kernels), kernels
    ref = out.to_host()
    for d in (X, y, Xp, out):
        d.free()
    assert np.array_equal(st, st_ref) and np.array_equal(st, est)
    assert np.array_equal(got, ref), f"C={C}: the DMA kernel differs from the register-tile kernel"
    assert_close(ref, exp, what=f"register-tile kernel vs oracle C={C}")
