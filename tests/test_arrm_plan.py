"""The ARRM launch plan (scikit-downscale_amd/csrc/sd_arrm_plan.h, compiled with g++) against the reference's window geometry as
Python states it (arrm.py:47-67, 87-91): start, width, the half-to-even slot of every window and which of two windows that share
a slot is written last; the refusals; and the launch sizes against the LDS of the device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _arrm_oracle as ao  # noqa: E402

LDS = 160 * 1024
CUS = 256


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("aplan") / "arrm_plan_check"
    src = os.path.join(ROOT, "tests", "arrm_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(T, C=1000, mb=7, ld=None, lds=LDS, cus=CUS):
        line = " ".join(map(str, [T, C, C if ld is None else ld, mb, lds, cus]))
        out = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end"
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return {"error": int(code), "message": msg}
        rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines[:-1]}
        half, B, start, width, nacc, slices = rows["plan"]
        return dict(half=half, B=B, start=start, width=width, nacc=nacc, slices=slices, select=rows["select"], accum=rows["accum"],
                    predict=rows["predict"], upper=rows["upper"], lower=rows["lower"])

    return run


@pytest.mark.parametrize("T", [50, 51, 190, 200, 210, 290, 310, 365, 500, 501, 530, 600, 1200, 14600, 19456])
def test_geometry_matches_python(plan, T):
    p = plan(T)
    q = ao.plotting_positions(T)
    start = int(abs(q - 0.4).argmin())
    width = max(round(0.05 * T), 10)
    assert (p["start"], p["width"]) == (start, width) and start >= width
    # the upper loop in the reference's order: the last writer of every slot
    last = {}
    for right in range(start, T + 1):
        left = right - width
        last[round((left + right) / 2)] = left
    assert p["upper"] == [m for m, _ in sorted(last.items(), key=lambda kv: kv[1])]
    # the lower loop runs downwards: the smallest left of a slot is written last
    stop = start + 4
    final = {}
    for left in range(stop, -1, -1):
        final[round((2 * left + width) / 2)] = left
    assert p["lower"] == [1 if final[round((2 * left + width) / 2)] == left else 0 for left in range(stop + 1)]
    if width % 2:
        assert len(set(p["upper"])) == len(p["upper"]) and all(m % 2 == 0 for m in p["upper"])


@pytest.mark.parametrize("mb,half", [(2, 1), (3, 1), (4, 2), (7, 3), (16, 8), (17, 8)])
def test_breaks_of_max_breakpoints(plan, mb, half):
    p = plan(600, mb=mb)
    assert (p["half"], p["B"], p["nacc"]) == (half, 2 * half, 5 * (2 * half - 1) + 1)


def test_refusals(plan):
    assert plan(49) == {"error": 1, "message": "sd_arrm_fit: T = 49 samples, at least 50 are needed (the first window would start before the series)"}
    assert plan(600, mb=1)["error"] == 1 and plan(600, mb=18)["error"] == 1 and plan(600, mb=-3)["error"] == 1
    assert plan(600, C=10, ld=9)["error"] == 1 and plan(600, C=0)["error"] == 1
    assert plan(20000)["error"] == 3  # the r2 series of a cell must fit in LDS


@pytest.mark.parametrize("T,C,mb", [(50, 1, 2), (600, 67, 7), (14600, 100000, 7), (14600, 100000, 16), (19456, 5, 16)])
def test_launch_sizes(plan, T, C, mb):
    p = plan(T, C, mb)
    gx, block, lds = p["select"]
    assert lds == 8 * T and lds + 8192 <= LDS and block == 512 and 1 <= gx <= min(C, 4 * CUS)
    agx, agy, ablock, alds = p["accum"]
    assert agx == -(-C // 64) and agy == p["slices"] and 1 <= agy <= 8 and ablock in (128, 256)
    assert alds == 8 * (p["nacc"] - 1) * ablock + 8 * 16 * 64 and alds <= LDS
    assert T // (agy * ablock // 64) >= min(64, T // (ablock // 64))  # a slice is not shorter than 64 steps where T allows
    # the slice count is a function of T alone: a chunk of a grid adds a cell's sums in the same order as the whole grid
    assert plan(T, 3, mb)["slices"] == p["slices"]


SLICE_T = [50, 127, 128, 255, 256, 257, 1023, 1024, 2047, 2048, 19456]


@pytest.mark.parametrize("mb", range(2, 18))
def test_every_break_count(plan, mb):
    """max_breakpoints 2 .. 17: B, the sums per (cell, slice), the accumulate workgroup (every thread keeps 5 (B - 1) doubles in
    LDS: 256 threads while that is at most 64 KB, which is B <= 6, else 128) with its LDS bytes, and the slice count (64 steps per
    thread at least, 8 slices at most), restated here from those rules and not from the header"""
    B = 2 * (mb // 2)
    block = 256 if B <= 6 else 128
    assert (8 * 5 * (B - 1) * 256 <= 64 * 1024) == (block == 256)
    lds = 8 * 5 * (B - 1) * block + 8 * 16 * 64  # the sums, and the knots of 64 cells
    for T in SLICE_T:
        p = plan(T, 67, mb)
        assert (p["half"], p["B"], p["nacc"]) == (mb // 2, B, 5 * (B - 1) + 1)
        rows_per_step = block // 64  # time steps a workgroup takes at once
        slices = min(8, max(1, T // (64 * rows_per_step)))
        assert p["slices"] == slices and p["accum"] == [2, slices, block, lds], (T, p["accum"])
        assert lds <= LDS
    if B == 16:
        assert lds == 84992 and lds > 64 * 1024


@pytest.mark.parametrize("mb,B", [(2, 2), (3, 2), (16, 16), (17, 16)])
@pytest.mark.parametrize("T,C", [(50, 1), (255, 64), (256, 65), (257, 129), (1025, 67)])
def test_predict_launch(plan, mb, B, T, C):
    """256 rows and 64 cells per workgroup, breaks and beta of the 64 cells in LDS"""
    assert plan(T, C, mb)["predict"] == [-(-C // 64), -(-T // 256), 256, 2 * 8 * B * 64]
