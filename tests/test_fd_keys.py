"""The integer formulas of bcsd_fd_kernel's sort keys, pad keys and tag addresses (scikit-downscale_amd/csrc/sd_bcsd_plan.h, namespace
sdfx::tmj), checked on the host: the header is compiled with g++ into a small driver (tests/fd_keys_check.cpp) that evaluates the
forms the kernel uses (key_u2: four instructions per key; key_off: chunk and slot straight from the key; pad_key) and the forms they
replaced, bit for bit, and both against the layout restated there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("spread", "near_integers_and_halves", "nonfinite", "tag_addresses", "pad_keys")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fd_keys") / "fd_keys_check"
    src = os.path.join(ROOT, "tests", "fd_keys_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert got[-1] == "end", got
    return got[:-1]


@pytest.mark.parametrize("name", CHECKS)
def test_formulas(lines, name):
    """spread: ~10^5 values of t over [1, kQD - 1] and the exact ends, every tag; near_integers_and_halves: within one ulp (of t and
    of t + 2^21) of an integer and of a half; nonfinite: NaN and the infinities; tag_addresses: every tag, and the tags of every
    lane for 57, 60, 62 and 64 lanes of data; pad_keys: every lane past the data"""
    assert f"ok {name}" in lines, lines


def test_every_check_ran(lines):
    assert sorted(lines) == sorted(f"ok {n}" for n in CHECKS), lines
