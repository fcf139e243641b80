"""CPU: the calendar of a disaggregation (skdownscale_amd.disagg.time_map) against an independent pandas formulation, the oracle
(tests/_disagg_oracle.py) against a per-month pandas restatement, and the closed loop on the oracle: pandas' resampler applied to the
daily output gives the monthly target back within the derived bound (_disagg_oracle.bound)."""
import numpy as np
import pandas as pd
import pytest

import _disagg_oracle as do
from skdownscale_amd import time_map
from skdownscale_amd.disagg import disagg_op


_eligible = {}


def eligible_years(daily, month):
    """years whose calendar month is held day by day, exactly once: boolean masks on .year / .month and days_in_month"""
    key = (daily[0], daily[-1], len(daily), month)
    if key not in _eligible:
        _eligible[key] = _eligible_years(daily, month)
    return _eligible[key]


def _eligible_years(daily, month):
    years = []
    for y in sorted(set(daily.year)):
        days = daily[(daily.year == y) & (daily.month == month)]
        if len(days) == pd.Timestamp(year=y, month=month, day=1).days_in_month and len(set(days.normalize())) == len(days):
            years.append(y)
    return years


def independent_map(monthly, daily, years):
    times, rows, offsets = [], [], [0]
    for label, y in zip(monthly, years):
        src = np.flatnonzero((daily.year == y) & (daily.month == label.month))
        assert y in eligible_years(daily, label.month)
        n = label.days_in_month
        rows += [src[min(d, len(src) - 1)] for d in range(n)]
        times += list(pd.date_range(pd.Timestamp(year=label.year, month=label.month, day=1), periods=n, freq="D"))
        offsets.append(offsets[-1] + n)
    return pd.DatetimeIndex(times), np.array(rows, dtype=np.int64), np.array(offsets, dtype=np.int64)


def assert_map(got, want):
    assert got[0].equals(want[0]) and isinstance(got[0], pd.DatetimeIndex)
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1])
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2])


DAILY = pd.date_range("2001-01-01", "2008-12-31", freq="D")  # leap years 2004 and 2008


def test_leap_months_on_short_sources_and_the_reverse():
    monthly = pd.DatetimeIndex(["2004-02-01", "2005-02-01", "2008-02-01"])
    years = np.array([2001, 2004, 2008])
    out_time, src_row, offsets = got = time_map(monthly, DAILY, years)
    assert_map(got, independent_map(monthly, DAILY, years))
    assert list(np.diff(offsets)) == [29, 28, 29]
    feb01, feb04 = DAILY.get_loc("2001-02-01"), DAILY.get_loc("2004-02-01")
    assert list(src_row[:29]) == list(range(feb01, feb01 + 28)) + [feb01 + 27]  # the last day is repeated
    assert list(src_row[29:57]) == list(range(feb04, feb04 + 28))                # the 29th is dropped
    assert out_time[28] == pd.Timestamp("2004-02-29") and out_time[29] == pd.Timestamp("2005-02-01")


def test_gaps_between_months_and_month_end_labels():
    monthly = pd.DatetimeIndex(["2001-01-01", "2001-03-01", "2002-07-01"])
    years = [2003, 2001, 2008]
    assert_map(time_map(monthly, DAILY, np.array(years)), independent_map(monthly, DAILY, years))
    ms, me = pd.date_range("2002-11-01", periods=6, freq="MS"), pd.date_range("2002-11-30", periods=6, freq="ME")
    for kw in (dict(years="same"), dict(seed=4)):
        a, b = time_map(ms, DAILY, **kw), time_map(me + pd.Timedelta(hours=6), DAILY, **kw)  # the day and hour of a label are ignored
        assert_map(a, b)
    assert time_map(ms, DAILY, "same")[0].equals(pd.date_range("2002-11-01", "2003-04-30", freq="D"))


def test_same_year_on_overlapping_periods_is_the_identity():
    daily = pd.date_range("2003-01-01", "2004-12-31", freq="D")
    out_time, src_row, offsets = time_map(pd.date_range("2003-01-01", periods=24, freq="MS"), daily, "same")
    assert np.array_equal(src_row, np.arange(len(daily))) and out_time.equals(daily) and offsets[-1] == len(daily)
    # inside a longer record
    out_time, src_row, _ = time_map(pd.date_range("2003-01-01", periods=24, freq="MS"), DAILY, "same")
    assert np.array_equal(src_row, DAILY.get_loc("2003-01-01") + np.arange(len(daily))) and out_time.equals(daily)


def test_seeded_draws_are_reproducible_and_eligible():
    # March 2002 lacks a day, May 2003 holds a day twice (two hours), January 2009 is cut short
    daily = pd.date_range("2001-01-01", "2009-01-15", freq="D")
    daily = daily.delete(daily.get_loc("2002-03-17"))
    daily = daily.insert(daily.get_loc("2003-05-11"), pd.Timestamp("2003-05-10 12:00"))
    assert 2002 not in eligible_years(daily, 3) and 2003 not in eligible_years(daily, 5) and 2009 not in eligible_years(daily, 1)
    monthly = pd.date_range("2030-01-01", periods=240, freq="MS")
    for seed in (0, 3):
        rng = np.random.default_rng(seed)
        years = [int(rng.choice(eligible_years(daily, label.month))) for label in monthly]  # one draw per month, in order
        got = time_map(monthly, daily, seed=seed)
        assert_map(got, independent_map(monthly, daily, years))
        assert_map(got, time_map(monthly, daily, None, seed))
        src_time = daily[got[1]]
        assert (src_time.month == got[0].month).all()
        assert not ((src_time.year == 2002) & (src_time.month == 3)).any() and not ((src_time.year == 2003) & (src_time.month == 5)).any()
        assert not (src_time.year == 2009).any() and len(set(src_time.year)) == 8
    assert not np.array_equal(time_map(monthly, daily, seed=0)[1], time_map(monthly, daily, seed=3)[1])
    assert np.array_equal(time_map(monthly, daily)[1], time_map(monthly, daily, seed=0)[1])  # the default seed


def test_refusals():
    monthly = pd.date_range("2003-01-01", periods=3, freq="MS")
    with pytest.raises(ValueError, match="the monthly time coordinate must be a DatetimeIndex"):
        time_map(np.arange(3), DAILY)
    with pytest.raises(ValueError, match="the daily time coordinate must be a DatetimeIndex"):
        time_map(monthly, np.arange(len(DAILY)))
    with pytest.raises(ValueError, match="the daily time coordinate must be a DatetimeIndex"):
        time_map(monthly, pd.period_range("2001-01-01", periods=400, freq="D"))
    with pytest.raises(ValueError, match=r"daily time coordinate is not strictly increasing at position 5 \(2001-01-05"):
        time_map(monthly, DAILY[:5].append(DAILY[4:]))
    with pytest.raises(ValueError, match="not strictly increasing at position 1"):
        time_map(monthly, DAILY[::-1])
    with pytest.raises(ValueError, match=r"strictly increasing \(year, month\): position 1 \(2003-01-31"):
        time_map(pd.DatetimeIndex(["2003-01-01", "2003-01-31"]), DAILY)
    with pytest.raises(ValueError, match=r"strictly increasing \(year, month\): position 2"):
        time_map(pd.DatetimeIndex(["2003-01-01", "2003-03-01", "2003-02-01"]), DAILY)
    with pytest.raises(ValueError, match="do not hold every day of 2009-02 exactly once: it cannot be borrowed for 2003-02"):
        time_map(monthly, DAILY, np.array([2001, 2009, 2001]))
    with pytest.raises(ValueError, match="do not hold every day of 2010-01 exactly once: it cannot be borrowed for 2010-01"):
        time_map(pd.date_range("2010-01-01", periods=2, freq="MS"), DAILY, "same")
    with pytest.raises(ValueError, match="hold no complete month to borrow for 2003-02"):
        time_map(monthly, DAILY[:40])
    with pytest.raises(ValueError, match="expected None, 'same' or one year per month"):
        time_map(monthly, DAILY, "random")
    with pytest.raises(ValueError, match="expected 3 integer years"):
        time_map(monthly, DAILY, np.array([2001, 2002]))
    with pytest.raises(ValueError, match="expected 3 integer years"):
        time_map(monthly, DAILY, np.array([2001.0, 2002.0, 2003.0]))
    with pytest.raises(ValueError, match="nothing to disaggregate"):
        time_map(monthly[:0], DAILY)
    # kind / stat
    assert disagg_op("shift") == disagg_op("shift", "mean") == "shift" and disagg_op("scale", "mean") == "scale_mean" and disagg_op("scale", "sum") == "scale_sum"
    with pytest.raises(ValueError, match="kind='scale' needs stat='mean' or stat='sum'"):
        disagg_op("scale")
    with pytest.raises(ValueError, match="kind='scale' needs stat='mean' or stat='sum'"):
        disagg_op("scale", "max")
    with pytest.raises(ValueError, match="kind='shift' matches the monthly mean"):
        disagg_op("shift", "sum")
    with pytest.raises(ValueError, match="expected 'shift' or 'scale'"):
        disagg_op("ratio")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    """6 years x 5 cells: temperatures and zero-inflated precipitation with a NaN day, a NaN cell, a dry month and an all-NaN month"""
    rng = np.random.default_rng(7)
    daily = pd.date_range("2001-01-01", "2006-12-31", freq="D")
    monthly = pd.date_range("2041-01-01", periods=72, freq="MS")
    out_time, src_row, offsets = time_map(monthly, daily, seed=11)
    T = len(daily)
    tas = 285.0 + 10.0 * np.sin(2 * np.pi * np.arange(T) / 365.25)[:, None] + 3.0 * rng.normal(size=(T, 5))
    pr = np.where(rng.random((T, 5)) < 0.6, 0.0, rng.gamma(0.7, 6.0, size=(T, 5)))
    first = int(src_row[offsets[3]])  # the source month of output month 3
    for x in (tas, pr):
        x[first + 4, 1] = np.nan                             # a NaN day
        x[:, 4] = np.nan                                     # a NaN cell
        x[first:first + 31, 2] = np.nan                      # an all-NaN source month (as long as output month 3 at least)
    second = int(src_row[offsets[5]])
    pr[second:second + 31, 0] = 0.0                          # a dry source month
    months = pd.DataFrame(index=monthly)
    t_tas = 288.0 + 8.0 * np.sin(2 * np.pi * (months.index.month.to_numpy() - 4) / 12)[:, None] + rng.normal(size=(72, 5))
    t_pr = rng.gamma(2.0, 1.5, size=(72, 5))
    t_pr[7, 3] = 0.0
    t_tas[9, 0] = t_pr[9, 0] = np.nan                        # a NaN target
    return dict(daily=daily, monthly=monthly, out_time=out_time, src_row=src_row, offsets=offsets, tas=tas, pr=pr, t_tas=t_tas, t_pr=t_pr,
                dry=(5, 0), all_nan=(3, 2), nan_target=(9, 0))


def fields(case, op):
    return (case["t_tas"], case["tas"]) if op == "shift" else (case["t_pr"] * (30.0 if op == "scale_sum" else 1.0), case["pr"])


@pytest.mark.parametrize("op", do.OPS)
def test_oracle_against_a_per_month_pandas_restatement(case, op):
    target, obs = fields(case, op)
    src_row, offsets = case["src_row"], case["offsets"]
    got = do.disaggregate(target, obs, src_row, offsets, op)
    frame = pd.DataFrame(obs)
    u, worst = 2.0 ** -53, 0.0
    for m in range(72):
        x = frame.iloc[src_row[offsets[m]:offsets[m + 1]]].reset_index(drop=True)
        tgt, n = target[m], x.notna().sum().to_numpy()
        with np.errstate(all="ignore"):
            if op == "shift":
                want = (x + (tgt - x.mean())).to_numpy()
            else:
                stat = x.mean() if op == "scale_mean" else x.sum()
                want = (x * (tgt / stat)).to_numpy()
                dry = (stat == 0).to_numpy()  # every non-NaN day gets the same share
                share = tgt if op == "scale_mean" else tgt / n
                want[:, dry] = np.where(x.notna().to_numpy(), share, np.nan)[:, dry]
            want[:, n == 0] = np.nan
            block = got[offsets[m]:offsets[m + 1]]
            assert np.array_equal(np.isnan(block), np.isnan(want)), (op, m)
            # pandas' mean / sum add in another order: the statistic moves by at most 2 n u sum|x| (/ n), the rest is one rounding each
            Sx = x.abs().sum().to_numpy()
            if op == "shift":
                tol = 2 * u * (n + 2) * Sx / np.maximum(n, 1) + 2 * np.spacing(np.abs(want))
            else:
                tol = np.abs(want) * (2 * u * (n + 2) * np.where(Sx > 0, Sx / np.abs(x.sum().to_numpy()), 0.0) + 4 * u) + 5e-324
            err = np.nan_to_num(np.abs(block - want), nan=0.0)
            worst = max(worst, float(np.max(np.nan_to_num(err / tol, nan=0.0))))
            assert (err <= np.nan_to_num(tol, nan=0.0)).all(), (op, m, worst)
    print(f"{op}: oracle against pandas, max |diff| / tol = {worst:.3f}")
    m, c = case["dry"]
    if op != "shift":
        dry = got[offsets[m]:offsets[m + 1], c]
        n = offsets[m + 1] - offsets[m]
        assert (dry == (target[m, c] if op == "scale_mean" else target[m, c] / n)).all()
    m, c = case["all_nan"]
    assert np.isnan(got[offsets[m]:offsets[m + 1], c]).all() and np.isnan(got[:, 4]).all()
    m, c = case["nan_target"]
    assert np.isnan(got[offsets[m]:offsets[m + 1], c]).all() and np.isfinite(got[offsets[m]:offsets[m + 1], 3]).all()


@pytest.mark.parametrize("op", do.OPS)
@pytest.mark.parametrize("with_climo", [False, True], ids=["plain", "climo"])
def test_the_closed_loop_returns_the_target(case, op, with_climo):
    target, obs = fields(case, op)
    src_row, offsets = case["src_row"], case["offsets"]
    climo = group = None
    if with_climo:  # the target as an anomaly on a monthly climatology
        group = (case["monthly"].month.to_numpy() - 1).astype(np.int32)
        with np.errstate(invalid="ignore"):
            climo = np.stack([np.nanmean(target[group == g], axis=0) for g in range(12)])
            target = target - climo[group] if op == "shift" else target / climo[group]
    out = do.disaggregate(target, obs, src_row, offsets, op, climo, group)
    back = pd.DataFrame(out, index=case["out_time"]).resample("MS")
    back = (back.sum(min_count=1) if op == "scale_sum" else back.mean()).to_numpy()
    want = do.resolve_target(target, op, climo, group)
    nothing = np.isnan(out).reshape(-1, 5)
    assert back.shape == want.shape == (72, 5)
    bound = do.bound(out, target, obs, src_row, offsets, op, climo, group)
    _, cnt = do.statistic(obs, src_row, offsets)
    defined = (cnt > 0) & ~np.isnan(want)
    assert np.array_equal(np.isnan(back), ~defined) and nothing[:, 4].all()
    err = np.abs(back - want)[defined]
    ratio = float((err / bound[defined]).max())
    rel = float((err / np.maximum(np.abs(want[defined]), 1e-300)).max())
    print(f"{op} {'climo' if with_climo else 'plain'}: largest err / bound = {ratio:.4f} (largest |err| = {err.max():.3e}, relative {rel:.3e})")
    assert (err <= bound[defined]).all(), ratio
