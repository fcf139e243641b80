"""The threshold / spell launch plan (scikit-downscale_amd/csrc/sd_spells_plan.h), checked on the host: the header is compiled with g++
into a small driver (tests/spells_plan_check.cpp) that prints plans, checks group ids and offsets tables and walks the grid of a plan
the way spells_kernel decodes it."""
import os
import subprocess

import pytest

from _bins_offsets import BAD_OFFSETS, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT, GE, LT, LE = 0, 1, 2, 3
VALID, COUNT, FRACTION, LONGEST, DAYS, SPELLS = range(6)
INVALID = 1
GROUP, PER_WAVE, BATCH = 8, 2, 8  # bins of a workgroup, bins of a wave, rows in flight


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "spells_plan_check"
    src = os.path.join(ROOT, "tests", "spells_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(what="plan", op=GT, f32=False, T=14600, C=100_000, ld=None, table=False, G=1, ld_t=None, has_group=None, M=40, min_length=1,
            stats=(COUNT,), nstat=None, ld_out=None, stride_out=None, src_aligned=True, table_aligned=True, out_aligned=True, group=None,
            offsets=None):
        ld = C if ld is None else ld
        ld_t = C if ld_t is None else ld_t
        ld_out = C if ld_out is None else ld_out
        stride_out = M * ld_out if stride_out is None else stride_out
        has_group = (table and G > 1) if has_group is None else has_group
        nstat = len(stats) if nstat is None else nstat
        codes = (list(stats) + [0] * 6)[:6]
        line = (f"{what} {op} {int(f32)} {T} {C} {ld} {int(table)} {G} {ld_t} {int(has_group)} {M} {min_length} {nstat} "
                f"{' '.join(str(s) for s in codes)} {ld_out} {stride_out} {int(src_aligned)} {int(table_aligned)} {int(out_aligned)}")
        if offsets is not None:
            ids = [] if not has_group else (group if group is not None else [r % G for r in range(T)])
            assert len(ids) == (T if has_group else 0) and len(offsets) == M + 1
            line = line.replace("plan", "tables", 1) + " " + " ".join(str(int(v)) for v in list(ids) + list(offsets))
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
    p = plan()  # forty years of daily steps, yearly bins, one statistic of a scalar threshold
    assert p == dict(cols=2, block=256, ctiles=782, bin_groups=5, blocks=782 * 5, bins_per_group=GROUP, bins_per_wave=PER_WAVE, batch=BATCH)
    for op in (GE, LT, LE):
        assert plan(op=op) == p
    assert plan(table=True, G=366, stats=(COUNT, FRACTION, DAYS), min_length=6) == p  # the day-of-year table, three statistics
    assert plan(table=True, G=1) == p  # a per-cell threshold
    assert plan(f32=True) == dict(p, cols=4, ctiles=391, blocks=391 * 5)
    assert plan(stats=(VALID, COUNT, FRACTION, LONGEST, DAYS, SPELLS)) == p and plan(stats=(COUNT, COUNT)) == p  # (a code may repeat)
    assert plan(min_length=1 << 40) == p  # never reached, not refused


@pytest.mark.parametrize("f32,kw,cols", [
    # float64: two cells per lane need C, every leading dimension and the stride even and every pointer on 16 bytes
    (False, dict(), 2), (False, dict(C=101), 1), (False, dict(ld=101), 1), (False, dict(ld=102), 2), (False, dict(ld_out=101), 1),
    (False, dict(ld_out=104), 2), (False, dict(stride_out=40 * 100 + 1), 1), (False, dict(stride_out=40 * 100 + 2), 2),
    (False, dict(src_aligned=False), 1), (False, dict(out_aligned=False), 1),
    # the table counts only where there is one
    (False, dict(table_aligned=False, ld_t=101), 2), (False, dict(table=True, table_aligned=False), 1), (False, dict(table=True, ld_t=101), 1),
    (False, dict(table=True, ld_t=102), 2), (False, dict(table=True, G=5, ld_t=101), 1), (False, dict(table=True, G=5, ld_t=106), 2),
    # float32: four where everything divides by four, else two, else one
    (True, dict(), 4), (True, dict(C=102), 2), (True, dict(ld=102), 2), (True, dict(ld_out=102), 2), (True, dict(ld=104, ld_out=108), 4),
    (True, dict(stride_out=40 * 100 + 2), 2), (True, dict(stride_out=40 * 100 + 4), 4), (True, dict(stride_out=40 * 100 + 3), 1),
    (True, dict(table=True, ld_t=102), 2), (True, dict(table=True, ld_t=104), 4), (True, dict(table=True, ld_t=101), 1),
    (True, dict(table=True, table_aligned=False), 1), (True, dict(C=101), 1), (True, dict(src_aligned=False), 1), (True, dict(C=4), 4)])
def test_cells_per_lane_follow_alignment_and_evenness(plan, f32, kw, cols):
    kw = dict(dict(C=100, T=1000), **kw)
    p = plan(f32=f32, **kw)
    assert p["cols"] == cols and p["ctiles"] == -(-kw["C"] // (64 * cols)) and p["blocks"] == p["ctiles"] * 5


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

    assert err(op=4) == (INVALID, "sd_spells: unknown op code 4") and err(op=-1)[1].endswith("code -1")
    assert err(stats=(COUNT, 6)) == (INVALID, "sd_spells: unknown statistic code 6 (stats[1])")
    assert err(stats=(-1,)) == (INVALID, "sd_spells: unknown statistic code -1 (stats[0])")
    assert err(stats=(), nstat=0) == (INVALID, "sd_spells: nstat = 0, expected 1 to 6 statistics")
    assert err(stats=(COUNT,) * 6, nstat=7) == (INVALID, "sd_spells: nstat = 7, expected 1 to 6 statistics") and err(nstat=-2)[1].startswith("sd_spells: nstat = -2")
    assert err(min_length=0) == (INVALID, "sd_spells: min_length = 0, expected at least 1") and err(min_length=-4)[0] == INVALID
    for bad in (dict(T=0), dict(C=0), dict(M=0), dict(T=-1), dict(C=-5), dict(M=-1)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_spells: bad sizes (T="), bad
    assert err(T=0, M=0) == (INVALID, "sd_spells: bad sizes (T=0, C=100000, M=0)")
    assert err(T=1 << 31, C=1, M=1) == (INVALID, "sd_spells: T = 2147483648 steps, the counts are int32 (T < 2^31)")
    assert "error" not in plan(T=(1 << 31) - 1, C=1, M=1)
    assert err(ld=99_999) == (INVALID, "sd_spells: ld = 99999 is less than the 100000 cells of a row")
    assert err(table=True, ld_t=99_999) == (INVALID, "sd_spells: ld_t = 99999 is less than the 100000 cells of a row")
    assert "error" not in plan(ld_t=1)  # no table: not read
    assert err(ld_out=99_999) == (INVALID, "sd_spells: ld_out = 99999 is less than the 100000 cells of a row")
    assert err(stride_out=40 * 100_000 - 1) == (INVALID, "sd_spells: stride_out = 3999999 is less than the 4000000 elements of one statistic (M * ld_out)")
    assert err(ld_out=100_002, stride_out=40 * 100_000)[1].startswith("sd_spells: stride_out = 4000000 is less than the 4000080 elements")
    assert "error" not in plan(stride_out=40 * 100_000 + 6, stats=(COUNT, DAYS))
    assert err(T=1 << 30, C=1 << 30, ld=1 << 40, M=1) == (INVALID, "sd_spells: field too large")
    assert err(T=1, C=1 << 30, M=1 << 40, stride_out=1 << 30)[1] == "sd_spells: field too large"
    assert err(T=1, C=1, M=1, stride_out=1 << 60, stats=(COUNT,) * 6)[1] == "sd_spells: field too large"
    assert err(table=True, G=0) == (INVALID, "sd_spells: bad sizes (G=0)") and err(table=True, G=-3)[1] == "sd_spells: bad sizes (G=-3)"
    assert "error" not in plan(G=0)  # no table: not read
    assert err(T=1, C=1, M=1, table=True, G=1 << 62, has_group=False)[1] == "sd_spells: field too large"
    assert err(table=True, G=2, has_group=False) == (INVALID, "sd_spells: a table of 2 rows needs group ids (group is NULL)")
    assert "error" not in plan(T=100, table=True, G=1, has_group=True)  # (ids of one group: all zero)
    # the order: op, statistic codes, nstat, min_length, sizes, T, ld, ld_t, ld_out, stride_out, too large, G, NULL group, ids, offsets, grid
    everything = dict(op=9, stats=(7,), nstat=9, min_length=0, T=0, ld=1, table=True, ld_t=1, ld_out=1, stride_out=1, G=0)
    order = ["unknown op", "unknown statistic", "nstat = 9", "min_length = 0", "bad sizes (T=0", "ld = 1", "ld_t = 1", "ld_out = 1", "stride_out = 1",
             "bad sizes (G=0)"]
    fixes = [dict(op=GT), dict(stats=(COUNT,)), dict(nstat=1), dict(min_length=1), dict(T=14600), dict(ld=100_000), dict(ld_t=100_000),
             dict(ld_out=100_000), dict(stride_out=40 * 100_000), dict(G=1)]
    for words, fix in zip(order, fixes):
        assert err(**everything)[1].startswith("sd_spells: " + words), (words, err(**everything))
        everything.update(fix)
    assert "error" not in plan(**everything)


def test_group_ids_and_offsets_tables(plan):
    def check(offsets, T=10, group=None, G=1, **kw):
        return plan(T=T, C=4, M=len(offsets) - 1, offsets=offsets, table=group is not None, has_group=group is not None, group=group, G=G, **kw)

    assert "error" not in check([0, 10]) and "error" not in check([0, 0, 3, 3, 10, 10])  # empty first, middle and last bins
    assert "error" not in check([0, 4, 10], group=[0, 1, 2, 2, 1, 0, 0, 0, 2, 2], G=3)
    assert check([0, 10], group=[0, 1, 2, 3, 1, 0, 0, 0, 2, 2], G=3) == dict(error=INVALID, message="sd_spells: group[3] = 3 lies outside the 3 groups")
    assert check([0, 10], group=[-1] + [0] * 9, G=3)["message"] == "sd_spells: group[0] = -1 lies outside the 3 groups"
    assert check([0, 5, 4, 10]) == dict(error=INVALID, message="sd_spells: offsets decrease at bin 1 (4 after 5)")
    assert check([0, 11]) == dict(error=INVALID, message="sd_spells: offsets[M] = 11, expected T = 10")
    assert check([0, -1, 10])["message"] == "sd_spells: offsets decrease at bin 0 (-1 after 0)"
    # the ids come before the offsets, and a refusal of the sizes and codes before either
    assert check([1, 10], group=[5] * 10, G=3)["message"].startswith("sd_spells: group[0] = 5")
    assert check([1, 10], group=[5] * 10, G=3, op=7)["message"] == "sd_spells: unknown op code 7"
    assert check([1, 10], group=[5] * 10, G=3, min_length=0)["message"].startswith("sd_spells: min_length = 0")


@pytest.mark.parametrize("offsets,words", BAD_OFFSETS)
def test_offsets_refusals_in_the_words_shared_with_resample(plan, offsets, words):
    got = plan(T=ROWS, C=4, M=len(offsets) - 1, offsets=offsets)
    assert got == dict(error=INVALID, message=words.format(who="sd_spells", rows="T"))


def test_the_limit_of_two_to_the_31(plan):
    big = dict(error=INVALID, message="sd_spells: grid too large")
    most = (1 << 31) - 1
    # one bin group, one cell per lane (an unaligned source): ctiles < 2^31
    assert plan(T=1, C=most * 64, M=1, src_aligned=False)["blocks"] == most and plan(T=1, C=most * 64 + 1, M=1, src_aligned=False) == big
    # 782 cell tiles by runs of bins
    groups = most // 782
    assert plan(T=1, M=groups * GROUP)["blocks"] == groups * 782 and plan(T=1, M=groups * GROUP + 1) == big
