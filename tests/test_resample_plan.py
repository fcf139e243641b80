"""The resampling launch plan (scikit-downscale_amd/csrc/sd_resample_plan.h), checked on the host: the header is compiled with g++
into a small driver (tests/resample_plan_check.cpp) that prints plans, checks offsets tables and walks the grid of a plan the way
resample_kernel decodes it."""
import os
import subprocess

import pytest

from _bins_offsets import BAD_OFFSETS, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, SUM = 0, 1
INVALID = 1
GROUP, PER_WAVE, BATCH = 8, 2, 8  # bins of a workgroup, bins of a wave, rows in flight


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "resample_plan_check"
    src = os.path.join(ROOT, "tests", "resample_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(what="plan", op=MEAN, f32=False, T=14600, C=100_000, ld=None, M=480, ld_out=None, src_aligned=True, out_aligned=True, offsets=None):
        ld = C if ld is None else ld
        ld_out = C if ld_out is None else ld_out
        line = f"{what} {op} {int(f32)} {T} {C} {ld} {M} {ld_out} {int(src_aligned)} {int(out_aligned)}"
        if offsets is not None:
            line = line.replace("plan", "offsets", 1) + " " + " ".join(str(int(o)) for o in offsets)
        out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        first = lines[0]
        if first.startswith("error "):
            _, code, msg = first.split(" ", 2)
            return {"error": int(code), "message": msg}
        return {k: int(v) for k, v in (w.split("=") for w in first.split()[1:])}

    return run


def test_plan_of_the_benchmark_shape(plan):
    p = plan()
    assert p == dict(cols=2, block=256, ctiles=782, bin_groups=60, blocks=782 * 60, bins_per_group=GROUP, bins_per_wave=PER_WAVE, batch=BATCH)
    assert plan(op=SUM) == p
    assert plan(f32=True) == dict(p, cols=4, ctiles=391, blocks=391 * 60)


@pytest.mark.parametrize("f32,C,ld,ld_out,src_aligned,out_aligned,cols", [
    # float64: two cells per lane need C and both leading dimensions even and both pointers on 16 bytes
    (False, 100, None, None, True, True, 2), (False, 101, None, None, True, True, 1), (False, 100, 101, None, True, True, 1),
    (False, 100, 102, None, True, True, 2), (False, 100, None, 101, True, True, 1), (False, 100, None, 104, True, True, 2),
    (False, 100, None, None, False, True, 1), (False, 100, None, None, True, False, 1), (False, 1, None, None, True, True, 1),
    (False, 2, None, None, True, True, 2),
    # float32: four where everything divides by four, else two, else one
    (True, 100, None, None, True, True, 4), (True, 102, None, None, True, True, 2), (True, 100, 102, None, True, True, 2),
    (True, 100, None, 102, True, True, 2), (True, 100, 104, 108, True, True, 4), (True, 101, None, None, True, True, 1),
    (True, 100, 101, None, True, True, 1), (True, 100, None, None, False, True, 1), (True, 100, None, None, True, False, 1),
    (True, 4, None, None, True, True, 4)])
def test_cells_per_lane_follow_alignment_and_evenness(plan, f32, C, ld, ld_out, src_aligned, out_aligned, cols):
    p = plan(f32=f32, C=C, ld=ld, ld_out=ld_out, src_aligned=src_aligned, out_aligned=out_aligned)
    assert p["cols"] == cols and p["ctiles"] == -(-C // (64 * cols)) and p["blocks"] == p["ctiles"] * 60


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 127, 128, 129, 130, 256, 257, 260, 516])
@pytest.mark.parametrize("M", [1, PER_WAVE, PER_WAVE + 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 3])
def test_the_grid_covers_every_cell_and_bin_once(plan, f32, C, M):
    c = plan("cover", f32=f32, T=100, C=C, M=M)
    assert c == dict(cells_min=1, cells_max=1, bins_min=1, bins_max=1, outside=0)
    p = plan(f32=f32, T=100, C=C, M=M)
    assert p["bin_groups"] == -(-M // GROUP) and p["ctiles"] == -(-C // (64 * p["cols"]))


def test_refusals_and_their_messages(plan):
    def err(**kw):
        p = plan(**kw)
        return p["error"], p["message"]

    assert err(op=2) == (INVALID, "sd_resample: unknown op code 2") and err(op=-1)[1].endswith("code -1")
    for bad in (dict(T=0), dict(C=0), dict(M=0), dict(T=-1), dict(C=-5), dict(M=-1)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_resample: bad sizes (T="), bad
    assert err(T=0, M=0) == (INVALID, "sd_resample: bad sizes (T=0, C=100000, M=0)")
    assert err(ld=99_999) == (INVALID, "sd_resample: ld = 99999 is less than the 100000 cells of a row")
    assert err(ld_out=99_999) == (INVALID, "sd_resample: ld_out = 99999 is less than the 100000 cells of a row")
    assert "error" not in plan(ld=100_000, ld_out=100_000)
    # the order: op, sizes, ld, ld_out
    assert err(op=5, T=0, ld=1, ld_out=1)[1].startswith("sd_resample: unknown op")
    assert err(T=0, ld=1, ld_out=1)[1].startswith("sd_resample: bad sizes")
    assert err(ld=1, ld_out=1)[1].startswith("sd_resample: ld = 1")


def test_offsets_tables(plan):
    def check(offsets, T=10, M=None, **kw):
        return plan(T=T, C=4, M=len(offsets) - 1 if M is None else M, offsets=offsets, **kw)

    assert "error" not in check([0, 10]) and "error" not in check([0, 0, 3, 3, 10, 10])  # empty first, middle and last bins
    assert check([1, 10]) == dict(error=INVALID, message="sd_resample: offsets[0] = 1, expected 0")
    assert check([0, 9]) == dict(error=INVALID, message="sd_resample: offsets[M] = 9, expected T = 10")
    assert check([0, 11]) == dict(error=INVALID, message="sd_resample: offsets[M] = 11, expected T = 10")
    assert check([0, 5, 4, 10]) == dict(error=INVALID, message="sd_resample: offsets decrease at bin 1 (4 after 5)")
    assert check([0, 12, 10])["message"] == "sd_resample: offsets decrease at bin 1 (10 after 12)"  # (never past T on the way)
    assert check([0, -1, 10])["message"] == "sd_resample: offsets decrease at bin 0 (-1 after 0)"
    # a refusal of the plan comes first and the table is not read
    assert check([0, 10], op=7)["message"] == "sd_resample: unknown op code 7"


@pytest.mark.parametrize("offsets,words", BAD_OFFSETS)
def test_offsets_refusals_in_the_words_shared_with_disagg(plan, offsets, words):
    got = plan(T=ROWS, C=4, M=len(offsets) - 1, offsets=offsets)
    assert got == dict(error=INVALID, message=words.format(who="sd_resample", rows="T"))


def test_the_limit_of_two_to_the_31(plan):
    big = dict(error=INVALID, message="sd_resample: grid too large")
    most = (1 << 31) - 1
    # one cell tile: bin_groups < 2^31
    assert plan(T=1, C=1, M=most * GROUP)["blocks"] == most and plan(T=1, C=1, M=most * GROUP + 1) == big
    # 782 cell tiles
    groups = most // 782
    assert plan(M=groups * GROUP)["blocks"] == groups * 782 and plan(M=groups * GROUP + 1) == big
    assert plan(T=1 << 40, C=1 << 30, M=1) == dict(error=INVALID, message="sd_resample: field too large")
    assert plan(T=1, C=1 << 30, M=1 << 40)["message"] == "sd_resample: field too large"
