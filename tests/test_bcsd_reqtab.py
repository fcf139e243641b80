"""The request row tables of the LDS-DMA kernel (scikit-downscale_amd/csrc/sd_bcsd_plan.h: tmj::build_row_tables), checked on the host:
the header is compiled with g++ into a small driver (tests/bcsd_reqtab_check.cpp) that builds P and W for a segment length and
compares them with the chunk layout restated there (lane l owns rows 20 l .. 20 l + 19, tails in the chunks behind the lanes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# months of a 40-year daily series (1 200, 1 240 whole lanes; 1 130, 1 230 ragged), the shortest lengths the kernel takes, the longest
LENGTHS = (1200, 1240, 1130, 1230, 660, 1280)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("reqtab") / "bcsd_reqtab_check"
    src = os.path.join(ROOT, "tests", "bcsd_reqtab_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(lengths):
        text = "".join(f"{m} {11 + i}\n" for i, m in enumerate(lengths))
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        return lines[:-1]

    return run


def test_tables_equal_the_chunk_layout(check):
    """P and W of the builder equal the restated layout; every row of the segment sits in exactly one slot, every other slot holds
    row m - 1; W is the stated permutation of P; entries are in range for a random order table."""
    assert check(LENGTHS) == [f"ok {m}" for m in LENGTHS]


def test_lengths_between_the_months(check):
    """every remainder m % 20 (the ragged last lane reaches its tail slots from 17 on), and every count of data lanes"""
    lengths = list(range(1121, 1141)) + list(range(641, 1281, 20))
    assert check(lengths) == [f"ok {m}" for m in lengths]


def test_a_length_the_kernel_does_not_take_is_refused(check):
    assert check([640, 1281]) == ["FAIL 640: length outside the kernel's range", "FAIL 1281: length outside the kernel's range"]
