"""The route policies of the register wave sort's cross-lane stages (scikit-downscale_amd/csrc/sd_wsort.h: via_lds(policy, L, x) --
which stages of the merge levels 4 .. 6 fetch their partner through the LDS pipe instead of a DPP move), checked on the host: the op
lists of every policy at K = 20 are compiled into a small C++ program (tests/wsort_route_check.cpp) that runs them on a model of the
64 lanes: sorted and equal to the stage-by-stage form on random keys, runs of equal keys and reversed input; per register the same
comparator sequence as policy 0; every med3 fed through the LDS pipe behind a counted wait of at most kMaxLgkm."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wsort_route")
    exe = tmp / "wsort_route_check"
    src = os.path.join(ROOT, "tests", "wsort_route_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    # sd_wsort.h includes <hip/hip_runtime.h> for its device half: a stub directory keeps the host compile self-contained
    stub = tmp / "hip"
    stub.mkdir()
    (stub / "hip_runtime.h").write_text("#pragma once\n")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{tmp}", f"-I{inc}", src, "-o", str(exe)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return run.returncode, run.stdout + run.stderr


@pytest.mark.parametrize("policy", [0, 1, 2, 3])
def test_policy(report, policy):
    rc, out = report
    line = [ln for ln in out.splitlines() if ln.startswith(f"policy {policy}:")]
    assert len(line) == 1 and line[0].endswith(": ok"), out
    # 15 stages of K = 20 keys in the levels 4 .. 6; a policy step moves three of them off the vector pipe
    m = re.search(r"(\d+) requests to the LDS pipe, (\d+) DPP moves, \d+ counted waits \(at most (\d+) outstanding\)", line[0])
    assert m and (int(m.group(1)), int(m.group(2))) == (120 + 60 * policy, 180 - 60 * policy) and int(m.group(3)) <= 15, line[0]


def test_all_policies_pass(report):
    rc, out = report
    assert rc == 0 and out.count(": ok") == 4, out
