"""The disaggregation launch plan (scikit-downscale_amd/csrc/sd_disagg_plan.h), checked on the host: the header is compiled with g++
into a small driver (tests/disagg_plan_check.cpp) that prints plans, checks the tables of a call and walks the grid of a plan the way
disagg_kernel decodes it."""
import os
import subprocess

import numpy as np
import pytest

from _bins_offsets import BAD_OFFSETS, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT, SCALE_MEAN, SCALE_SUM = 0, 1, 2
INVALID = 1
GROUP, PER_WAVE, BATCH = 8, 2, 8  # bins of a workgroup, bins of a wave, rows in flight


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "disagg_plan_check"
    src = os.path.join(ROOT, "tests", "disagg_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(what="plan", op=SHIFT, f32=False, To=14610, C=100_000, Tout=14600, M=480, ld_t=None, ld_obs=None, ld_out=None, climo=False, group=None,
            G=12, ld_c=None, aligned=(True, True, True, True), src_row=None, offsets=None, groups=None):
        ld = [C if v is None else v for v in (ld_t, ld_obs, ld_out, ld_c)]
        group = climo if group is None else group
        words = [what, op, int(f32), To, C, Tout, M, ld[0], ld[1], ld[2], int(climo), int(group), G, ld[3], *(int(a) for a in aligned)]
        for tab in (src_row, offsets, groups):
            if tab is not None:
                words += [int(v) for v in tab]
        out = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=120)
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
    assert plan(op=SCALE_MEAN) == p and plan(op=SCALE_SUM) == p and plan(climo=True) == p
    assert plan(f32=True) == dict(p, cols=4, ctiles=391, blocks=391 * 60)


ALL = (True, True, True, True)


@pytest.mark.parametrize("f32,C,lds,climo,aligned,cols", [
    # float64: two cells per lane need C and every leading dimension even and every pointer on 16 bytes
    (False, 100, {}, False, ALL, 2), (False, 101, {}, False, ALL, 1), (False, 1, {}, False, ALL, 1), (False, 2, {}, False, ALL, 2),
    (False, 100, dict(ld_t=101), False, ALL, 1), (False, 100, dict(ld_obs=101), False, ALL, 1), (False, 100, dict(ld_out=101), False, ALL, 1),
    (False, 100, dict(ld_t=102, ld_obs=104, ld_out=106), False, ALL, 2),
    (False, 100, {}, False, (False, True, True, True), 1), (False, 100, {}, False, (True, False, True, True), 1),
    (False, 100, {}, False, (True, True, False, True), 1),
    # the climatology counts only when there is one
    (False, 100, dict(ld_c=101), False, ALL, 2), (False, 100, dict(ld_c=101), True, ALL, 1), (False, 100, dict(ld_c=102), True, ALL, 2),
    (False, 100, {}, False, (True, True, True, False), 2), (False, 100, {}, True, (True, True, True, False), 1),
    # float32 observations: four where everything divides by four, else two, else one
    (True, 100, {}, False, ALL, 4), (True, 102, {}, False, ALL, 2), (True, 101, {}, False, ALL, 1), (True, 4, {}, False, ALL, 4),
    (True, 100, dict(ld_t=102), False, ALL, 2), (True, 100, dict(ld_obs=102), False, ALL, 2), (True, 100, dict(ld_out=102), False, ALL, 2),
    (True, 100, dict(ld_t=104, ld_obs=108, ld_out=112), False, ALL, 4), (True, 100, dict(ld_obs=101), False, ALL, 1),
    (True, 100, dict(ld_c=102), True, ALL, 2), (True, 100, dict(ld_c=104), True, ALL, 4),
    (True, 100, {}, False, (True, False, True, True), 1), (True, 100, {}, True, (True, True, True, False), 1)])
def test_cells_per_lane_follow_alignment_and_evenness(plan, f32, C, lds, climo, aligned, cols):
    p = plan(f32=f32, C=C, climo=climo, aligned=aligned, **lds)
    assert p["cols"] == cols and p["ctiles"] == -(-C // (64 * cols)) and p["blocks"] == p["ctiles"] * 60


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 129, 130, 257, 260, 516])
@pytest.mark.parametrize("lengths", [[31], [1], [28, 29, 30, 31, 1, 8, 9, 16, 7], [3] * GROUP, [2, 0] * GROUP + [5]],
                         ids=["M=1", "one row", "M=group+1", "M=group", "M=2*group+1 with empty bins"])
def test_the_grid_writes_every_row_and_cell_once(plan, f32, C, lengths):
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    Tout, M = int(offsets[-1]), len(lengths)
    c = plan("cover", f32=f32, To=40, C=C, Tout=Tout, M=M, offsets=offsets)
    assert c == dict(written_min=1, written_max=1, outside=0)
    p = plan(f32=f32, To=40, C=C, Tout=Tout, M=M)
    assert p["bin_groups"] == -(-M // GROUP) and p["ctiles"] == -(-C // (64 * p["cols"]))


def test_refusals_and_their_messages(plan):
    def err(**kw):
        p = plan(**kw)
        return p["error"], p["message"]

    assert err(op=3) == (INVALID, "sd_disagg: unknown op code 3") and err(op=-1)[1].endswith("code -1")
    for bad in (dict(To=0), dict(C=0), dict(Tout=0), dict(M=0), dict(To=-1), dict(C=-5), dict(Tout=-2), dict(M=-1)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_disagg: bad sizes (To="), bad
    assert err(Tout=0, M=0) == (INVALID, "sd_disagg: bad sizes (To=14610, C=100000, Tout=0, M=0)")
    assert err(climo=True, group=False) == (INVALID, "sd_disagg: climo without group")
    assert err(climo=False, group=True) == (INVALID, "sd_disagg: group without climo")
    assert err(climo=True, G=0) == (INVALID, "sd_disagg: bad sizes (G=0)") and "error" not in plan(G=0)
    for name in ("ld_t", "ld_obs", "ld_out"):
        assert err(**{name: 99_999}) == (INVALID, f"sd_disagg: {name} = 99999 is less than the 100000 cells of a row")
    assert err(climo=True, ld_c=99_999) == (INVALID, "sd_disagg: ld_c = 99999 is less than the 100000 cells of a row")
    assert "error" not in plan(ld_c=5)  # (not read without a climatology)
    # the order: op, sizes, climo / group, leading dimensions
    assert err(op=5, To=0, climo=True, group=False, ld_t=1)[1].startswith("sd_disagg: unknown op")
    assert err(To=0, climo=True, group=False, ld_t=1)[1].startswith("sd_disagg: bad sizes")
    assert err(climo=True, group=False, ld_t=1)[1].startswith("sd_disagg: climo without group")
    assert err(ld_t=1, ld_obs=1)[1].startswith("sd_disagg: ld_t = 1")


def test_tables(plan):
    def check(src_row, offsets, To=10, groups=None, G=3, **kw):
        return plan("tables", To=To, C=4, Tout=len(src_row), M=len(offsets) - 1, src_row=src_row, offsets=offsets, climo=groups is not None,
                    groups=groups, G=G, **kw)

    rows = [3, 4, 5, 5, 9, 0]
    assert "error" not in check(rows, [0, 6]) and "error" not in check(rows, [0, 0, 4, 4, 6, 6])  # empty first, middle and last bins
    assert "error" not in check(rows, [0, 4, 6], groups=[2, 0])
    assert check(rows, [1, 6]) == dict(error=INVALID, message="sd_disagg: offsets[0] = 1, expected 0")
    assert check(rows, [0, 5]) == dict(error=INVALID, message="sd_disagg: offsets[M] = 5, expected Tout = 6")
    assert check(rows, [0, 7]) == dict(error=INVALID, message="sd_disagg: offsets[M] = 7, expected Tout = 6")
    assert check(rows, [0, 5, 4, 6]) == dict(error=INVALID, message="sd_disagg: offsets decrease at bin 1 (4 after 5)")
    assert check(rows, [0, 8, 6])["message"] == "sd_disagg: offsets decrease at bin 1 (6 after 8)"  # (never past Tout on the way)
    assert check(rows, [0, -1, 6])["message"] == "sd_disagg: offsets decrease at bin 0 (-1 after 0)"
    assert check([3, 10, 5], [0, 3]) == dict(error=INVALID, message="sd_disagg: src_row[1] = 10 lies outside the 10 rows of obs")
    assert check([3, 4, -1], [0, 3]) == dict(error=INVALID, message="sd_disagg: src_row[2] = -1 lies outside the 10 rows of obs")
    assert "error" not in check([9, 0, 9], [0, 3])
    assert check(rows, [0, 4, 6], groups=[0, 3]) == dict(error=INVALID, message="sd_disagg: group[1] = 3 lies outside the 3 rows of climo")
    assert check(rows, [0, 4, 6], groups=[-1, 0]) == dict(error=INVALID, message="sd_disagg: group[0] = -1 lies outside the 3 rows of climo")
    # a refusal of the plan comes first and the tables are not read; offsets come before src_row, src_row before group
    assert check(rows, [0, 6], op=7)["message"] == "sd_disagg: unknown op code 7"
    assert check([3, 10, 5], [0, 2])["message"].startswith("sd_disagg: offsets[M]")
    assert check([3, 10, 5], [0, 3], groups=[9])["message"].startswith("sd_disagg: src_row[1]")


@pytest.mark.parametrize("offsets,words", BAD_OFFSETS)
def test_offsets_refusals_in_the_words_shared_with_resample(plan, offsets, words):
    got = plan("tables", To=ROWS, C=4, Tout=ROWS, M=len(offsets) - 1, src_row=[0] * ROWS, offsets=offsets)
    assert got == dict(error=INVALID, message=words.format(who="sd_disagg", rows="Tout"))


def test_the_limit_of_two_to_the_31(plan):
    big = dict(error=INVALID, message="sd_disagg: grid too large")
    most = (1 << 31) - 1
    # one cell tile: bin_groups < 2^31
    assert plan(To=1, C=1, Tout=1, M=most * GROUP)["blocks"] == most and plan(To=1, C=1, Tout=1, M=most * GROUP + 1) == big
    # 782 cell tiles
    groups = most // 782
    assert plan(M=groups * GROUP)["blocks"] == groups * 782 and plan(M=groups * GROUP + 1) == big
    too_large = dict(error=INVALID, message="sd_disagg: field too large")
    assert plan(To=1 << 40, C=1 << 30, Tout=1, M=1) == too_large and plan(To=1, C=1 << 30, Tout=1 << 40, M=1) == too_large
    assert plan(To=1, C=1 << 30, Tout=1, M=1 << 40) == too_large and plan(To=1, C=1 << 30, Tout=1, M=1, climo=True, G=1 << 40) == too_large
