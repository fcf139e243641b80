"""GPU: the kernels that run sdws::wave_sort with the merge levels 4 .. 6 in the half-batch issue order (csrc/sd_wsort.h),
against the oracle: the keys, the comparators and their order per register are those of the stage-by-stage form, so every
result must stay what it was.

BcsdTemperature fit + predict through the C ABI on 16 and 24 cells (24 is no multiple of the 8-cell tiles times two: the last
tile is fetched shifted back) with three daily calendars from 1980-01-01:
  22 years (T = 8 036)  months of 660 samples (33 lanes of 20: level 6 on its smallest input), 682 and 622 (ragged);
  40 years (T = 14 600) 1 240 / 1 200 (whole lanes) and 1 130 / 1 230 (ragged);
  15 years (T = 5 479)  every month below 641 samples: the register-tile kernel's wave_sort;
and three data sets: Gaussian; one cell whose x_fut is constant (all its keys tie: the item is handed back); cells in which
half the observations repeat their neighbour and x_fut has constant stretches (duplicates in both sorts).  The reference
is computed once for 24 cells; the 16-cell runs compare with its first columns (the model is pointwise).  Plus one PureAnalog
F = 1 case (16 cells x 2 000 steps): analog_sort2_kernel shares the header."""
import numpy as np
import pandas as pd
import pytest

import analog_oracle as ao
import bcsd_oracle as bo
from _cases import assert_close, month_gid
from skdownscale_amd import synth

pytestmark = pytest.mark.gpu

YEARS = {22: 8036, 40: 14600, 15: 5479}
CELLS = (16, 24)
CONST, DUP = 5, (9, 22)  # special cells; 22 lies in the shifted last tile of the 24-cell grid


def _gid(T):
    return month_gid(pd.date_range("1980-01-01", periods=T, freq="D"))


def _data(name, T):
    rng = np.random.default_rng(4100 + T)
    X, y, Xp = (15 + 8 * rng.standard_normal((T, 24)) for _ in range(3))
    if name == "constant":
        Xp[:, CONST] = 17.25
    if name == "duplicates":
        for c in DUP:
            y[1::2, c] = y[0:T - 1:2, c][: len(y[1::2, c])]
            # exact ties among the shifted samples u = x_fut - (rolling mean - x_climo): constant stretches inside one month, as in
            # test_gpu_bcsd_fd_late.py.  (x_fut constant over blocks everywhere would leave u = x_climo up to the rounding of the
            # rolling mean: ranks that depend on the last bit, in the oracle as in the engine.)
            for a in (125, 770, 4000):
                Xp[a:a + 24, c] = Xp[a, c]
    return X, y, Xp


_cache = {}


def _case(name, years):
    """inputs, group ids, expected field and status for 24 cells (computed once, read-only)"""
    key = (name, years)
    if key not in _cache:
        T = YEARS[years]
        gid = _gid(T)
        inputs = _data(name, T)
        exp, est = bo.pointwise_fit_predict(bo.TAS, *inputs, gid, gid, return_anoms=True)
        for a in inputs + (exp, est):
            a.setflags(write=False)
        _cache[key] = (inputs, gid, exp, est)
    return _cache[key]


def _engine(ctx, inputs, gid, C):
    X, y, Xp = (ctx.to_device(np.ascontiguousarray(v[:, :C])) for v in inputs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    out, st = ctx.bcsd_fit_predict(0, X, y, gid, 12, Xp, gid, True)
    ctx.prof_enable(False)
    print("kernels:", sorted(ctx.prof()))
    got = out.to_host()
    for d in (X, y, Xp, out):
        d.free()
    return got, st


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


def test_calendars_have_the_month_lengths_the_levels_need():
    m = {years: np.bincount(_gid(T), minlength=12) for years, T in YEARS.items()}
    assert m[22][3] == 660 and m[22][0] == 682 and m[22][1] == 622  # 660 = 33 lanes of 20 keys
    assert set(m[40]) == {1240, 1200, 1130, 1230}
    assert m[15].max() < 641


@pytest.mark.parametrize("C", CELLS)
@pytest.mark.parametrize("years", sorted(YEARS))
@pytest.mark.parametrize("name", ["gaussian", "constant", "duplicates"])
def test_bcsd_against_the_oracle(ctx, name, years, C):
    inputs, gid, exp, est = _case(name, years)
    got, st = _engine(ctx, inputs, gid, C)
    what = f"{name}, {years} years, C={C}"
    assert np.array_equal(st, est[:C]), (what, st, est[:C])
    ok = est[:C] == 0
    assert np.isnan(got[:, ~ok]).all(), what
    print(f"{what}: max abs error {np.nanmax(np.abs(got[:, ok] - exp[:, :C][:, ok])):.3e}")
    assert_close(got[:, ok], exp[:, :C][:, ok], what=what)


@pytest.mark.parametrize("years", sorted(YEARS))
def test_bit_identical_to_the_register_tile_kernel(dev_ctx, monkeypatch, years):
    """SD_FX_NODMA (development library): the same sorts inside bcsd_fx_kernel; where the plan chooses that kernel anyway the
    two runs are the same launch."""
    inputs, gid, exp, est = _case("duplicates", years)
    got, st = _engine(dev_ctx, inputs, gid, 24)
    monkeypatch.setenv("SD_FX_NODMA", "1")
    ref, st_ref = _engine(dev_ctx, inputs, gid, 24)
    monkeypatch.delenv("SD_FX_NODMA")
    assert np.array_equal(st, st_ref) and np.array_equal(st, est)
    assert np.array_equal(got, ref, equal_nan=True), f"{years} years: the DMA kernel differs from the register-tile kernel"


def test_pure_analog_one_feature(ctx):
    X, y, Xq = synth.analog_fields(7, 2000, np.arange(16), 16, n_query=300)
    exp = ao.pointwise_analog(X, y, Xq, 30, ao.KIND_MEAN)
    state = ctx.analog_fit(X, y)
    got, st = ctx.analog_predict(state, Xq, 30, 3)
    one, ost = ctx.analog_fit_predict(X, y, Xq, 30, 3)
    assert np.array_equal(st, ost)
    assert np.array_equal(one, got), "fit_predict differs from fit -> predict"
    assert_close(got, exp, what="PureAnalog F=1, 16 cells x 2000 steps")
