"""GPU: the kernels that run sdws::wave_sort<20> on the searched networks (csrc/sd_wsort_nets20.h: a sorter and a bitonic
merger built around 3-sorters), against the oracle.  A network that sorts hands the fix-up the same sorted keys, so every result
must stay what it was.

BcsdTemperature fit + predict through the C ABI on 16 and 24 cells (24 is no multiple of the 8-cell tiles times two: the last
tile is fetched shifted back) with two daily calendars from 1980-01-01:
  22 years (T = 8 036)  months of 660 samples (33 data lanes of 20: level 6 on its smallest input), 682 and 622 (ragged):
                        the launch plan gives these to the register-tile kernel bcsd_fx_kernel<20>;
  40 years (T = 14 600) 1 240 / 1 200 (whole lanes) and 1 130 / 1 230 (ragged): the LDS-DMA kernel bcsd_fd_kernel<20>;
and two data sets: Gaussian; and one with a cell whose x_fut is constant (all its keys tie: the item is handed back) beside
cells in which half the observations repeat their neighbour and x_fut has constant stretches (duplicates in both sorts).
The reference is computed once for 24 cells; the 16-cell runs compare with its first columns (the model is pointwise).
Plus one BcsdPrecipitation case, 16 cells x 40 years: the K = 20 rank kernels with the wet-day sorts of 12 keys per lane
(bcsd_fxc_kernel<20, 12>) share the header.  Tolerance: tests/_cases.py assert_close, as everywhere against this oracle."""
import numpy as np
import pandas as pd
import pytest

import bcsd_oracle as bo
from _cases import assert_close, month_gid
from skdownscale_amd import synth

pytestmark = pytest.mark.gpu

YEARS = {22: 8036, 40: 14600}
CELLS = (16, 24)
CONST, DUP = 5, (9, 22)  # special cells; 22 lies in the shifted last tile of the 24-cell grid


def _gid(T):
    return month_gid(pd.date_range("1980-01-01", periods=T, freq="D"))


def _data(name, T):
    rng = np.random.default_rng(5200 + T)
    X, y, Xp = (15 + 8 * rng.standard_normal((T, 24)) for _ in range(3))
    if name == "ties":
        Xp[:, CONST] = 17.25
        for c in DUP:
            y[1::2, c] = y[0:T - 1:2, c][: len(y[1::2, c])]
            # exact ties among the shifted samples u = x_fut - (rolling mean - x_climo): constant stretches inside one month
            # (x_fut constant over blocks everywhere would leave ranks that depend on the last bit of the rolling mean)
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


def _engine(ctx, kind, inputs, gid, C):
    X, y, Xp = (ctx.to_device(np.ascontiguousarray(v[:, :C])) for v in inputs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    out, st = ctx.bcsd_fit_predict(kind, X, y, gid, 12, Xp, gid, True)
    ctx.prof_enable(False)
    kernels = set(ctx.prof())
    print("kernels:", sorted(kernels))
    got = out.to_host()
    for d in (X, y, Xp, out):
        d.free()
    return got, st, kernels


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import default_context

    return default_context()


def test_calendars_have_the_month_lengths_the_levels_need():
    m = {years: np.bincount(_gid(T), minlength=12) for years, T in YEARS.items()}
    assert m[22][3] == 660 and m[22][0] == 682 and m[22][1] == 622  # 660 = 33 lanes of 20 keys
    assert set(m[40]) == {1240, 1200, 1130, 1230}


@pytest.mark.parametrize("C", CELLS)
@pytest.mark.parametrize("years", sorted(YEARS))
@pytest.mark.parametrize("name", ["gaussian", "ties"])
def test_bcsd_temperature_against_the_oracle(ctx, name, years, C):
    inputs, gid, exp, est = _case(name, years)
    got, st, kernels = _engine(ctx, 0, inputs, gid, C)
    what = f"{name}, {years} years, C={C}"
    # the fused K = 20 kernels ran: the LDS-DMA kernel for the 40-year months, the register-tile kernel for the 22-year ones
    want = "bcsd_fd_kernel" if years == 40 else "bcsd_fx_kernel"
    assert want in kernels and want + ("_ragged" if years == 40 else "_full") in kernels, (what, kernels)
    assert np.array_equal(st, est[:C]), (what, st, est[:C])
    ok = est[:C] == 0
    assert np.isnan(got[:, ~ok]).all(), what
    print(f"{what}: max abs error {np.nanmax(np.abs(got[:, ok] - exp[:, :C][:, ok])):.3e}")
    assert_close(got[:, ok], exp[:, :C][:, ok], what=what)


def test_bcsd_precipitation_against_the_oracle(ctx):
    T, C = YEARS[40], 16
    gid = _gid(T)
    cells = np.arange(C)
    X, y, Xp = (synth.fill(synth.PRECIP, 91, stream, np.arange(T), cells, C, amp=40.0 + stream, p_dry=0.6) for stream in (10, 11, 12))
    exp, est = bo.pointwise_fit_predict(bo.PR, X, y, Xp, gid, gid, return_anoms=True)
    got, st, kernels = _engine(ctx, 1, (X, y, Xp), gid, C)
    assert any(k.startswith(("bcsd_fxc_kernel", "bcsd_fxp_kernel")) for k in kernels), kernels
    assert np.array_equal(st, est), (st, est)
    ok = est == 0
    assert ok.any() and np.isnan(got[:, ~ok]).all()
    print(f"precipitation, 40 years, C={C}: max abs error {np.nanmax(np.abs(got[:, ok] - exp[:, ok])):.3e}")
    assert_close(got[:, ok], exp[:, ok], what="precipitation, 40 years, C=16")
