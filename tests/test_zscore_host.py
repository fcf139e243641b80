"""ZScoreRegressor on the host: the day-window plan (scikit-downscale_amd/csrc/sd_zscore_plan.h, compiled with g++) against the
NumPy oracle's construction, the errors raised before the engine is reached, and the oracle pinned to the reference's own
expectations (test/test_pointwise_models.py:236-299 of the reference)."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _zscore_oracle as zo  # noqa: E402

REF_TIME = pd.date_range(start="2018-01-01", end="2020-01-01")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("zplan") / "zscore_plan_check"
    src = os.path.join(ROOT, "tests", "zscore_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(day_idx, year, D, w):
        line = " ".join(map(str, [len(day_idx), D, w] + list(day_idx) + list(year)))
        out = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end"
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return {"error": int(code), "message": msg}
        L, n, K = map(int, lines[0].split()[1:])
        labels = [int(v) for v in lines[1].split()[1:]]
        wins = [[int(v) for v in ln.split()[1:]] for ln in lines[2:-1]]
        return {"L": L, "n": n, "K": K, "labels": labels, "win": wins}

    return run


def grid_of(index):
    doy = np.asarray(index.dayofyear)
    days, day_idx = np.unique(doy, return_inverse=True)
    return days, day_idx.ravel(), np.asarray(index.year)


CALENDARS = {
    "ref_2018_2020": REF_TIME,
    "daily_40y_leap": pd.date_range("1980-01-01", periods=40 * 365 + 10, freq="D"),
    "monthly_480": pd.date_range(periods=480, start="1950", freq="MS"),
    "days_100": pd.date_range("2001-03-01", periods=100, freq="D"),
}


@pytest.mark.parametrize("cal", sorted(CALENDARS))
@pytest.mark.parametrize("w", [1, 2, 30, 31, 61])
def test_plan_matches_oracle_windows(plan, cal, w):
    index = CALENDARS[cal]
    days, day_idx, year = grid_of(index)
    p = plan(day_idx, year, len(days), w)
    lab, mean, std = zo.fit_stats(np.arange(len(index), dtype=float) * 0.37 + np.sin(np.arange(len(index))), index, w)
    if len(lab) == 0:
        assert p["error"] == 3  # no kept window: refused as unsupported
        return
    assert p["K"] == len(lab)
    assert np.array_equal(days[p["labels"]], lab)
    # every kept window's day multiset gives the oracle's statistics
    vals = np.arange(len(index), dtype=float) * 0.37 + np.sin(np.arange(len(index)))
    for k, win in enumerate(p["win"]):
        assert len(win) == w
        s = np.concatenate([vals[day_idx == d] for d in win])
        np.testing.assert_allclose([s.mean(), s.std()], [mean[k], std[k]], rtol=1e-12, atol=1e-12)


def test_plan_headline_counts(plan):
    for index, K, first, last in ((REF_TIME, 364, 1, 364), (CALENDARS["daily_40y_leap"], 365, 1, 365)):
        days, day_idx, year = grid_of(index)
        p = plan(day_idx, year, len(days), 31)
        assert p["K"] == K and days[p["labels"][0]] == first and days[p["labels"][-1]] == last
    days, day_idx, year = grid_of(CALENDARS["monthly_480"])
    p = plan(day_idx, year, len(days), 31)
    assert p["K"] == 21
    assert list(days[p["labels"]][:4]) == [1, 32, 60, 61] and list(days[p["labels"]][-2:]) == [306, 335]


def test_plan_window_wider_than_the_day_grid_counts_days_twice(plan):
    index = pd.date_range("2000-01-01", periods=24, freq="MS")  # 13 distinct days of year (leap 2000)
    days, day_idx, year = grid_of(index)
    p = plan(day_idx, year, len(days), 31)
    assert len(days) < 31 and p["K"] > 0
    assert any(len(set(wn)) < len(wn) for wn in p["win"])
    lab, mean, std = zo.fit_stats(np.arange(24.0) ** 1.5, index, 31)
    assert np.array_equal(days[p["labels"]], lab)
    vals = np.arange(24.0) ** 1.5
    for k, wn in enumerate(p["win"]):
        s = np.concatenate([vals[day_idx == d] for d in wn])
        np.testing.assert_allclose([s.mean(), s.std()], [mean[k], std[k]], rtol=1e-12)


def test_plan_duplicate_day_is_refused(plan):
    index = pd.date_range("2001-01-01", periods=200, freq="12h")
    days, day_idx, year = grid_of(index)
    p = plan(day_idx, year, len(days), 31)
    assert p["error"] == 1 and "at most one sample per day" in p["message"]
    with pytest.raises(ValueError):
        zo.fit_stats(np.zeros(200), index, 31)


def test_plan_bad_width(plan):
    days, day_idx, year = grid_of(REF_TIME)
    assert plan(day_idx, year, len(days), 0) == {"error": 1, "message": "window_width must be positive, got 0"}


# ---- errors raised before the engine is reached ----
def test_window_width_must_be_positive():
    from skdownscale_amd import ZScoreRegressor

    with pytest.raises(ValueError, match="window_width must be positive, got 0"):
        ZScoreRegressor(window_width=0)


def test_two_features():
    from skdownscale_amd import ZScoreRegressor

    X = pd.DataFrame({"a": np.arange(50.0), "b": np.arange(50.0)}, index=REF_TIME[:50])
    y = pd.DataFrame({"a": np.arange(50.0)}, index=REF_TIME[:50])
    with pytest.raises(ValueError, match="Zscore only supports 1 feature, found 2"):
        ZScoreRegressor().fit(X, y)


def test_single_sample():
    from skdownscale_amd import ZScoreRegressor

    X = pd.DataFrame({"a": [1.0]}, index=REF_TIME[:1])
    with pytest.raises(TypeError, match="X.squeeze\\(\\) must be a pd.Series"):
        ZScoreRegressor().fit(X, X)


def test_non_datetime_index():
    from skdownscale_amd import ZScoreRegressor

    X = pd.DataFrame({"a": np.arange(50.0)})
    with pytest.raises(AttributeError, match=".dt accessor"):
        ZScoreRegressor().fit(X, X)


def test_predict_before_fit():
    from sklearn.exceptions import NotFittedError

    from skdownscale_amd import ZScoreRegressor

    with pytest.raises(NotFittedError):
        ZScoreRegressor().predict(pd.DataFrame({"a": np.arange(50.0)}, index=REF_TIME[:50]))


def test_exported_and_batched():
    import skdownscale_amd
    from skdownscale_amd.core import PointWiseDownscaler

    assert "ZScoreRegressor" in skdownscale_amd.__all__
    assert PointWiseDownscaler(skdownscale_amd.ZScoreRegressor())._batched() == "zscore"


# ---- the oracle against the reference's own expectations ----
def test_oracle_scale_anchor():
    X = np.linspace(0, 1, len(REF_TIME))
    f = zo.fit(X, 2 * X, REF_TIME)
    assert list(f["scale"].index) == list(range(1, 365))
    np.testing.assert_allclose(f["scale"], 2.0)


def test_oracle_shift_anchor():
    f = zo.fit(np.zeros(len(REF_TIME)), np.ones(len(REF_TIME)), REF_TIME)
    assert list(f["shift"].index) == list(range(1, 365))
    np.testing.assert_allclose(f["shift"], 1.0)


def test_oracle_identity_anchor():
    X = np.linspace(0, 1, len(REF_TIME))
    days = pd.Index(np.arange(1, 365), name="day")
    out, _ = zo.predict(X, REF_TIME, pd.Series(np.zeros(364), index=days), pd.Series(np.ones(364), index=days))
    exp = X.copy()
    exp[:15] = np.nan
    exp[-15:] = np.nan
    np.testing.assert_allclose(out.values, exp)


def test_oracle_expansion_past_the_fit_fails():
    days = pd.Index(np.arange(1, 100), name="day")
    with pytest.raises(IndexError):
        zo.predict(np.arange(400.0), pd.date_range("2001-01-01", periods=400), pd.Series(np.zeros(99), index=days),
                   pd.Series(np.ones(99), index=days))
