"""The paired skill launch plan (scikit-downscale_amd/csrc/sd_skill_plan.h), checked on the host: the header is compiled with g++ into a
small driver (tests/skill_plan_check.cpp) that prints plans, checks offsets tables and walks the grid of a plan the way skill_kernel
decodes it."""
import os
import subprocess

import pytest

from _bins_offsets import BAD_OFFSETS, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, BIAS, RATIO, MAE, RMSE, CORR, STD_RATIO = range(7)
INVALID = 1
GROUP, PER_WAVE, BATCH = 8, 2, 8  # bins of a workgroup, bins of a wave, rows in flight


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "skill_plan_check"
    src = os.path.join(ROOT, "tests", "skill_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(what="plan", a_f32=False, b_f32=False, T=14600, C=100_000, ld_a=None, ld_b=None, M=40, stats=(BIAS,), nstat=None, ld_out=None,
            stride_out=None, a_aligned=True, b_aligned=True, out_aligned=True, offsets=None):
        ld_a = C if ld_a is None else ld_a
        ld_b = C if ld_b is None else ld_b
        ld_out = C if ld_out is None else ld_out
        stride_out = M * ld_out if stride_out is None else stride_out
        nstat = len(stats) if nstat is None else nstat
        codes = (list(stats) + [0] * 7)[:7]
        line = (f"{what} {int(a_f32)} {int(b_f32)} {T} {C} {ld_a} {ld_b} {M} {nstat} {' '.join(str(s) for s in codes)} {ld_out} {stride_out} "
                f"{int(a_aligned)} {int(b_aligned)} {int(out_aligned)}")
        if offsets is not None:
            assert len(offsets) == M + 1
            line = line.replace("plan", "tables", 1) + " " + " ".join(str(int(v)) for v in offsets)
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


def test_plan_of_the_benchmark_shapes(plan):
    p = plan()  # forty years of daily steps against as many, yearly bins, float64 against float64
    assert p == dict(cols=2, block=256, ctiles=782, bin_groups=5, blocks=782 * 5, bins_per_group=GROUP, bins_per_wave=PER_WAVE, batch=BATCH)
    assert plan(stats=(BIAS, RMSE, CORR)) == p and plan(stats=tuple(range(7))) == p and plan(stats=(CORR, CORR)) == p  # (a code may repeat)
    assert plan(M=1) == dict(p, bin_groups=1, blocks=782)  # the whole axis
    assert plan(a_f32=True) == p and plan(b_f32=True) == p  # one float32 source: still two cells per lane
    assert plan(a_f32=True, b_f32=True) == dict(p, cols=4, ctiles=391, blocks=391 * 5)


@pytest.mark.parametrize("a_f32,b_f32,kw,cols", [
    # float64 on either side: two cells per lane need C, every leading dimension and the stride even and every pointer on 16 bytes
    (False, False, dict(), 2), (False, False, dict(C=101), 1), (False, False, dict(ld_a=101), 1), (False, False, dict(ld_b=101), 1),
    (False, False, dict(ld_a=102, ld_b=106), 2), (False, False, dict(ld_out=101), 1), (False, False, dict(ld_out=104), 2),
    (False, False, dict(stride_out=40 * 100 + 1), 1), (False, False, dict(stride_out=40 * 100 + 2), 2),
    (False, False, dict(a_aligned=False), 1), (False, False, dict(b_aligned=False), 1), (False, False, dict(out_aligned=False), 1),
    (True, False, dict(), 2), (False, True, dict(), 2), (True, False, dict(ld_a=104, ld_b=104, ld_out=104), 2), (True, False, dict(ld_b=101), 1),
    (False, True, dict(ld_a=101), 1), (True, False, dict(a_aligned=False), 1), (False, True, dict(b_aligned=False), 1), (True, False, dict(C=4), 2),
    # float32 on both sides: four where everything divides by four, else two, else one
    (True, True, dict(), 4), (True, True, dict(C=102), 2), (True, True, dict(ld_a=102), 2), (True, True, dict(ld_b=102), 2),
    (True, True, dict(ld_out=102), 2), (True, True, dict(ld_a=104, ld_b=112, ld_out=108), 4), (True, True, dict(stride_out=40 * 100 + 2), 2),
    (True, True, dict(stride_out=40 * 100 + 4), 4), (True, True, dict(stride_out=40 * 100 + 3), 1), (True, True, dict(ld_b=101), 1),
    (True, True, dict(C=101), 1), (True, True, dict(a_aligned=False), 1), (True, True, dict(b_aligned=False), 1),
    (True, True, dict(out_aligned=False), 1), (True, True, dict(C=4), 4)])
def test_cells_per_lane_follow_dtypes_alignment_and_evenness(plan, a_f32, b_f32, kw, cols):
    kw = dict(dict(C=100, T=1000), **kw)
    p = plan(a_f32=a_f32, b_f32=b_f32, **kw)
    assert p["cols"] == cols and p["ctiles"] == -(-kw["C"] // (64 * cols)) and p["blocks"] == p["ctiles"] * 5


@pytest.mark.parametrize("f32", [(False, False), (True, False), (True, True)], ids=["f64-f64", "f32-f64", "f32-f32"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 127, 128, 129, 130, 256, 257, 260, 516])
@pytest.mark.parametrize("M", [1, PER_WAVE, PER_WAVE + 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 3])
def test_the_grid_covers_every_bin_and_cell_once(plan, f32, C, M):
    a_f32, b_f32 = f32
    c = plan("cover", a_f32=a_f32, b_f32=b_f32, T=100, C=C, M=M)
    assert c == dict(min=1, max=1, outside=0)
    p = plan(a_f32=a_f32, b_f32=b_f32, T=100, C=C, M=M)
    assert p["bin_groups"] == -(-M // GROUP) and p["ctiles"] == -(-C // (64 * p["cols"]))
    assert p["cols"] == (4 if all(f32) and C % 4 == 0 else 2 if C % 2 == 0 else 1)


def test_refusals_and_their_messages(plan):
    def err(**kw):
        p = plan(**kw)
        return p["error"], p["message"]

    assert err(stats=(BIAS, 7)) == (INVALID, "sd_skill: unknown statistic code 7 (stats[1])")
    assert err(stats=(-1,)) == (INVALID, "sd_skill: unknown statistic code -1 (stats[0])")
    assert err(stats=(), nstat=0) == (INVALID, "sd_skill: nstat = 0, expected 1 to 7 statistics")
    assert err(stats=(BIAS,) * 7, nstat=8) == (INVALID, "sd_skill: nstat = 8, expected 1 to 7 statistics") and err(nstat=-2)[1].startswith("sd_skill: nstat = -2")
    for bad in (dict(T=0), dict(C=0), dict(M=0), dict(T=-1), dict(C=-5), dict(M=-1)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_skill: bad sizes (T="), bad
    assert err(T=0, M=0) == (INVALID, "sd_skill: bad sizes (T=0, C=100000, M=0)")
    assert err(T=1 << 31, C=1, M=1) == (INVALID, "sd_skill: T = 2147483648 steps, the counts are int32 (T < 2^31)")
    assert "error" not in plan(T=(1 << 31) - 1, C=1, M=1)
    assert err(ld_a=99_999) == (INVALID, "sd_skill: ld_a = 99999 is less than the 100000 cells of a row")
    assert err(ld_b=99_999) == (INVALID, "sd_skill: ld_b = 99999 is less than the 100000 cells of a row")
    assert err(ld_out=99_999) == (INVALID, "sd_skill: ld_out = 99999 is less than the 100000 cells of a row")
    assert err(stride_out=40 * 100_000 - 1) == (INVALID, "sd_skill: stride_out = 3999999 is less than the 4000000 elements of one statistic (M * ld_out)")
    assert err(ld_out=100_002, stride_out=40 * 100_000)[1].startswith("sd_skill: stride_out = 4000000 is less than the 4000080 elements")
    assert "error" not in plan(stride_out=40 * 100_000 + 6, stats=(BIAS, CORR))
    assert err(T=1 << 30, C=1 << 30, ld_a=1 << 40, M=1) == (INVALID, "sd_skill: field too large")
    assert err(T=1 << 30, C=1 << 30, ld_b=1 << 40, M=1) == (INVALID, "sd_skill: field too large")
    assert err(T=1, C=1 << 30, M=1 << 40, stride_out=1 << 30)[1] == "sd_skill: field too large"
    assert err(T=1, C=1, M=1, stride_out=1 << 60, stats=(BIAS,) * 7)[1] == "sd_skill: field too large"
    # the order: statistic codes, nstat, sizes, T, ld_a, ld_b, ld_out, stride_out, too large, offsets
    everything = dict(stats=(9,), nstat=9, T=0, ld_a=1, ld_b=1, ld_out=1, stride_out=1)
    order = ["unknown statistic", "nstat = 9", "bad sizes (T=0", "ld_a = 1", "ld_b = 1", "ld_out = 1", "stride_out = 1"]
    fixes = [dict(stats=(BIAS,)), dict(nstat=1), dict(T=14600), dict(ld_a=100_000), dict(ld_b=100_000), dict(ld_out=100_000),
             dict(stride_out=40 * 100_000)]
    for words, fix in zip(order, fixes):
        assert err(**everything)[1].startswith("sd_skill: " + words), (words, err(**everything))
        everything.update(fix)
    assert "error" not in plan(**everything)
    # T >= 2^31 comes behind the sizes and before the leading dimensions; too large before the table of bins
    assert err(T=1 << 31, C=4, M=1, ld_a=1)[1].startswith("sd_skill: T = 2147483648 steps")
    assert err(T=10, C=4, M=1, ld_a=1 << 61, offsets=[1, 10])[1] == "sd_skill: field too large"


def test_offsets_tables(plan):
    def check(offsets, T=10, **kw):
        return plan(T=T, C=4, M=len(offsets) - 1, offsets=offsets, **kw)

    assert "error" not in check([0, 10]) and "error" not in check([0, 0, 3, 3, 10, 10])  # empty first, middle and last bins
    assert check([0, 5, 4, 10]) == dict(error=INVALID, message="sd_skill: offsets decrease at bin 1 (4 after 5)")
    assert check([0, 11]) == dict(error=INVALID, message="sd_skill: offsets[M] = 11, expected T = 10")
    assert check([0, -1, 10])["message"] == "sd_skill: offsets decrease at bin 0 (-1 after 0)"
    # a refusal of the sizes and codes comes before the table
    assert check([1, 10], stats=(8,))["message"] == "sd_skill: unknown statistic code 8 (stats[0])"
    assert check([1, 10], ld_b=3)["message"].startswith("sd_skill: ld_b = 3")


@pytest.mark.parametrize("offsets,words", BAD_OFFSETS)
def test_offsets_refusals_in_the_words_shared_with_resample(plan, offsets, words):
    got = plan(T=ROWS, C=4, M=len(offsets) - 1, offsets=offsets)
    assert got == dict(error=INVALID, message=words.format(who="sd_skill", rows="T"))


def test_the_limit_of_two_to_the_31(plan):
    big = dict(error=INVALID, message="sd_skill: grid too large")
    most = (1 << 31) - 1
    # one bin group, one cell per lane (an unaligned source): ctiles < 2^31
    assert plan(T=1, C=most * 64, M=1, b_aligned=False)["blocks"] == most and plan(T=1, C=most * 64 + 1, M=1, b_aligned=False) == big
    # 782 cell tiles by runs of bins
    groups = most // 782
    assert plan(T=1, M=groups * GROUP)["blocks"] == groups * 782 and plan(T=1, M=groups * GROUP + 1) == big
