"""The build-or-destroy guard of the fitted states (scikit-downscale_amd/csrc/sd_state_guard.h, compiled with g++ alone under the
address and undefined-behaviour sanitizers): a failing body costs exactly one destroy, leaves *out NULL and hands its code back; a
body that succeeds costs none and *out is the state."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def guard(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sguard") / "state_guard_check"
    src = os.path.join(ROOT, "tests", "state_guard_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(codes):
        out = subprocess.run([str(exe)], input="".join(f"{c}\n" for c in codes), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]  # (a leak or a double free of the state fails here)
        return out.stdout.splitlines()

    return run


@pytest.mark.parametrize("code", [1, 2, 3, 4, -7])
def test_failing_body_destroys_once(guard, code):
    assert guard([code]) == [f"rc {code} destroys 1 out null"]


def test_body_that_succeeds_hands_the_state_over(guard):
    assert guard([0]) == ["rc 0 destroys 0 out state"]


def test_calls_do_not_share_anything(guard):
    assert guard([0, 2, 0]) == ["rc 0 destroys 0 out state", "rc 2 destroys 1 out null", "rc 0 destroys 0 out state"]
