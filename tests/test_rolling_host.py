"""CPU, no engine: the host side of GridArray.rolling (skdownscale_amd/rolling.py) -- the window arithmetic, the lazy surface, the
refusals and their messages, the halo block cutter of timesource.walk -- and the NumPy oracle (tests/_rolling_oracle.py) against
what pandas made of the golden cases (tests/golden/g27_rolling.npz, written by tests/golden/make_golden_rolling.py with pandas 2.3.3).

Tolerance (measured, tests/_rolling_oracle.py: pandas' online update carries rounding from earlier windows, so no bound follows from a
window alone): 8 x the largest difference measured on the golden file, in units of max|x| of the field (max|x|^2 for var and for
std^2).  The NaN patterns must match exactly."""
import os

import numpy as np
import pandas as pd
import pytest

import _rolling_oracle as ro

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g27_rolling.npz"))
    return {k: g[k] for k in g.files}


def test_the_golden_cases_are_what_the_issue_describes(golden):
    tas, pr = golden["tas"], golden["pr"]
    assert tas.shape == pr.shape == (400, 6) and golden["tas32"].dtype == np.float32 and golden["tas366"].shape == (366, 6)
    assert 0.03 < np.isnan(tas[:, :5]).mean() < 0.07 and np.isnan(tas[150:190, 5]).all()  # a run of NaN longer than every window
    assert 0.5 < (pr == 0.0).mean() < 0.7  # zero-inflated
    cases = ro.golden_cases(golden)
    have = {(f, w, op, c, mp) for _, f, w, op, c, mp, _, _ in cases}
    for call in (("tas", 9, "mean", True, 1), ("tas", 31, "mean", True, None), ("tas", 31, "std", True, None)):  # the reference's own
        assert call in have
    assert {w for _, _, w, *_ in cases} >= {1, 2, 5, 9, 30, 31} and {c for _, _, _, _, c, *_ in cases} == {False, True}
    assert {op for _, _, _, op, *_ in cases} == set(ro.OPS) and {mp for *_, mp, _, _ in cases} >= {None, 0, 1, 3}
    assert {dd for *_, dd, _ in cases} == {0, 1} and sum(wr for *_, wr in cases) >= 4
    assert golden["tas.w31.sum.c.mp0.ddof1"][170, 5] == 0.0 and np.isnan(golden["tas.w31.mean.t.mp0.ddof1"][185, 5])


def test_oracle_against_pandas_golden_and_live(golden):
    worst = dict.fromkeys(ro.OPS, 0.0)
    for key, f, w, op, center, mp, ddof, wrap in ro.golden_cases(golden):
        got = ro.rolling(golden[f], w, op, center, mp, ddof, wrap)
        worst[op] = max(worst[op], ro.check(got, golden[key], golden[f], op, f"{key} vs golden"))
        if not wrap:  # the pandas that is installed
            r = pd.DataFrame(golden[f].astype(np.float64)).rolling(w, center=center, min_periods=mp)
            live = (getattr(r, op)(ddof=ddof) if op in ("var", "std") else getattr(r, op)()).to_numpy()
            ro.check(got, live, golden[f], op, f"{key} vs pandas {pd.__version__}")
    print({op: f"{v:.2e} of the scale (measured {ro.MEASURED[op]:.1e}, allowed {ro.TOLERANCE[op]:.2e})" for op, v in worst.items()})
    assert all(ro.TOLERANCE[op] == 8 * ro.MEASURED[op] for op in ro.OPS)


def test_the_fast_oracle_has_the_bits_of_the_definition(golden):
    for f, T in (("tas", 400), ("pr", 150), ("tas32", 150)):
        x = golden[f][:T]
        for w, back, wrap in ((1, 0, False), (2, 1, False), (9, 4, False), (9, 8, True), (31, 15, False), (31, 30, False), (T, T // 2, False),
                              (T, 0, True), (331 if T == 400 else 120, 100, False)):
            for a, b in zip(ro.moments(x, w, back, wrap), ro.moments_by_rows(x, w, back, wrap)):
                assert np.array_equal(a, b) and not np.signbit(a[a == 0]).any(), (f, w, back, wrap)


def test_wrap_is_the_padded_series():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(37, 3))
    x[rng.random(x.shape) < 0.1] = np.nan
    for w in (1, 2, 9, 31, 37):
        for center in (False, True):
            back = ro.back_of(w, center)
            padded = np.concatenate([x[37 - back:], x, x[:w - 1 - back]])
            for op in ro.OPS:
                want = ro.rolling(padded, w, op, min_periods=1, back=back)[back:back + 37]
                assert np.array_equal(ro.rolling(x, w, op, center, 1, wrap=True), want, equal_nan=True), (w, center, op)


def test_window_and_label_arithmetic():
    from skdownscale_amd import GridArray
    from skdownscale_amd.rolling import window_back

    assert [window_back(w, False) for w in (1, 2, 9, 30)] == [0, 1, 8, 29] and [window_back(w, True) for w in (1, 2, 9, 30)] == [0, 1, 4, 15]
    # pandas puts the extra step of an even centred window before the label
    x = np.arange(10.0)[:, None]
    for w in (2, 4, 5):
        want = pd.DataFrame(x).rolling(w, center=True, min_periods=1).sum().to_numpy()
        assert np.array_equal(ro.rolling(x, w, "sum", True, 1), want)
    time = pd.date_range("2001-01-01", periods=20, freq="D")
    a = GridArray(np.arange(60.0).reshape(20, 3), ("time", "cell"), dict(time=time, cell=np.arange(3)), name="tas")
    for lazy in (a.rolling(time=9, center=True, min_periods=1).mean(), a.rolling({"time": 9}, center=True, min_periods=1).mean()):
        assert not lazy.computed and lazy.dims == a.dims and lazy.shape == a.shape and lazy.sizes == a.sizes and lazy.name == "tas"
        assert lazy.coords["time"] is a.coords["time"] and lazy.dtype == np.float64 and lazy.window == 9 and lazy.source is a
    r = a.rolling(time=5)
    assert (r.dim, r.window) == ("time", 5) and r.var()._ddof == 1 and r.std(ddof=0)._ddof == 0 and r.sum()._op == "sum"
    assert r.mean()._min_periods == 5 and a.rolling(time=5, min_periods=0).mean()._min_periods == 0
    part = r.mean().isel(cell=slice(1, 3))
    assert not part.computed and part.shape == (20, 2) and part.source.shape == (20, 2)
    chunked = r.mean().chunk({"cell": 2})
    assert chunked.chunksizes["cell"] == (2, 1) and chunked.unchunked().chunksizes is None and not chunked.computed


def test_refusals_and_their_messages():
    from skdownscale_amd import GridArray, GridRolling, RolledGridArray

    a = GridArray(np.zeros((20, 3)), ("time", "cell"), dict(time=np.arange(20)))
    with pytest.raises(ValueError, match="min_periods 10 must be <= window 9"):  # pandas' words
        a.rolling(time=9, min_periods=10)
    with pytest.raises(ValueError, match="min_periods 10 must be <= window 9"):
        pd.Series(np.zeros(20)).rolling(9, min_periods=10)
    with pytest.raises(ValueError, match="min_periods must be >= 0"):
        a.rolling(time=9, min_periods=-1)
    for w in (0, -3, 2.5):
        with pytest.raises(ValueError, match="window must be an integer 1 or greater"):
            a.rolling(time=w)
    with pytest.raises(ValueError, match="exactly one dim=window"):
        a.rolling()
    with pytest.raises(ValueError, match="exactly one dim=window"):
        a.rolling(time=3, cell=2)
    with pytest.raises(ValueError, match="dim 'day' is not a dim"):
        a.rolling(day=3)
    with pytest.raises(ValueError, match="rolling needs"):
        a.rolling("time")
    with pytest.raises(ValueError, match="wrap=True: the window of 21 steps is longer than the 20 steps"):
        a.rolling(time=21, wrap=True)
    assert isinstance(a.rolling(time=21), GridRolling)  # clipped: fine
    with pytest.raises(ValueError, match="ddof must be an integer >= 0"):
        a.rolling(time=3).var(ddof=-1)
    with pytest.raises(NotImplementedError, match="only mean, sum, var and std"):
        RolledGridArray(a, "time", 3, "max")
    r = a.rolling(time=3)
    for name in ("max", "min", "median", "count", "quantile", "apply", "construct"):
        with pytest.raises(NotImplementedError, match=rf"rolling\(...\)\.{name}\(\): only mean\(\), sum\(\), var\(\) and std\(\)"):
            getattr(r, name)()
    with pytest.raises(AttributeError):
        r.no_such_thing


@pytest.mark.parametrize("halo", [(0, 0), (8, 0), (4, 4), (15, 14), (0, 30), (30, 0)])
@pytest.mark.parametrize("T", [1, 37, 120, 400])
def test_halo_blocks_cover_every_row_once_and_hold_every_window(T, halo):
    from skdownscale_amd.timesource import _halo_blocks, _time_blocks

    before, after = halo
    for max_rows in (1, before + after, before + after + 1, before + after + 7, 64, T - 1, T, T + 5):
        if max_rows < 1:
            continue
        blocks = _halo_blocks(T, max_rows, halo)
        if max_rows < T and max_rows <= before + after:
            assert blocks is None  # no room for a row beside its halo
            continue
        assert [r0 for r0, *_ in blocks] == [0] + [r1 for _, r1, *_ in blocks[:-1]] and blocks[-1][1] == T  # every row once, in order
        for r0, r1, b0, b1 in blocks:
            assert 0 <= b0 <= r0 < r1 <= b1 <= T and b1 - b0 <= max(max_rows, 1)
            # every window of the run, clipped to the array, lies inside the block
            assert b0 <= max(0, r0 - before) and min(T, r1 + after) <= b1
        if halo == (0, 0):
            assert [(r0, r1) for r0, r1, _, _ in blocks] == _time_blocks(T, min(T, max_rows))
    assert _halo_blocks(T, T, halo) == [(0, T, 0, T)]
