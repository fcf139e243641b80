"""The issue order of the register wave sort's merge levels 4 .. 6 (csrc/sd_wsort.h, LevelSched), checked on the host: the op
lists the kernels execute are compiled into a small C++ program (tests/wsort_sched_check.cpp) that runs them on a model of the
64 lanes for K = 12, 20 and 24 and lanes_used = 1, 2, 3, 33, 62, 64: the dataflow of the lists (every fetch after the last write
of the register it reads and before the next one, every med3 on the fetch of its own stage), every 0-1 input of the merge
levels, and random 32-bit keys with duplicates and pads, all against the stage-by-stage form."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sched_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wsort_sched")
    exe = tmp / "wsort_sched_check"
    src = os.path.join(ROOT, "tests", "wsort_sched_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    # sd_wsort.h includes <hip/hip_runtime.h> for its device half: a stub directory keeps the host compile self-contained
    stub = tmp / "hip"
    stub.mkdir()
    (stub / "hip_runtime.h").write_text("#pragma once\n")
    res = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{tmp}", f"-I{inc}", src, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(exe)


@pytest.mark.parametrize("K", [12, 20, 24])
def test_level_schedule(sched_check, K):
    run = subprocess.run([sched_check, str(K)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    # the shipped chaining and the A/B one (first fetches of a level under the merger of the level before)
    assert run.stdout.count(": ok") == 2 and f"K={K}:" in run.stdout and f"K={K}, first fetches" in run.stdout, run.stdout
