"""The grouped launch plans of compare(...).groupby(...) (skill_groups_plan in scikit-downscale_amd/csrc/sd_skill_plan.h and
twosample_groups_plan in sd_twosample_plan.h), checked on the host: the headers are compiled with g++ into a small driver
(tests/skill_groups_plan_check.cpp) that prints plans and the row tables and walks the grid of a plan the way skill_groups_kernel decodes
it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, BIAS, RATIO, MAE, RMSE, CORR, STD_RATIO = range(7)
KS, PERKINS, NA, NB = range(4)
INVALID, UNSUPPORTED = 1, 3
FEW, PER_WAVE, WAVES = 16, 2, 4  # kFewGroups, kBinsPerWave, waves of a workgroup


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "skill_groups_plan_check"
    src = os.path.join(ROOT, "tests", "skill_groups_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


def _ask(exe, line):
    out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "end", lines
    first = lines[0]
    if first.startswith("error "):
        _, code, msg = first.split(" ", 2)
        return {"error": int(code), "message": msg}
    got = {"plan": first}
    for l in lines[1:-1]:
        name, *values = l.split()
        got[name] = [int(v) for v in values]
    return got


@pytest.fixture(scope="module")
def skill(exe):
    def run(what="skill", a_f32=False, b_f32=False, T=14600, C=100_000, ld_a=None, ld_b=None, G=12, stats=(BIAS,), nstat=None, ld_out=None,
            stride_out=None, a_aligned=True, b_aligned=True, out_aligned=True, ids=None):
        ld_a = C if ld_a is None else ld_a
        ld_b = C if ld_b is None else ld_b
        ld_out = C if ld_out is None else ld_out
        stride_out = G * ld_out if stride_out is None else stride_out
        nstat = len(stats) if nstat is None else nstat
        codes = (list(stats) + [0] * 7)[:7]
        ids = [] if ids is None else list(ids)
        got = _ask(exe, f"{what} {int(a_f32)} {int(b_f32)} {T} {C} {ld_a} {ld_b} {G} {nstat} {' '.join(str(s) for s in codes)} {ld_out} "
                        f"{stride_out} {int(a_aligned)} {int(b_aligned)} {int(out_aligned)} {len(ids)} {' '.join(str(int(v)) for v in ids)}")
        if "plan" in got:
            got.update({k: int(v) for k, v in (w.split("=") for w in got.pop("plan").split()[1:])})
        return got

    return run


@pytest.fixture(scope="module")
def twosample(exe):
    def run(a_f32=False, b_f32=False, T=2000, C=100, ld_a=None, ld_b=None, G=12, stats=(KS,), nstat=None, width=1.0, origin=0.0, ld_out=None,
            stride_out=None, a_aligned=True, b_aligned=True, lds_max=160 * 1024, cu_count=256, ids=None, sizes=None):
        if sizes is not None:
            T, G = sum(sizes), len(sizes)
        ld_a = C if ld_a is None else ld_a
        ld_b = C if ld_b is None else ld_b
        ld_out = C if ld_out is None else ld_out
        stride_out = G * ld_out if stride_out is None else stride_out
        nstat = len(stats) if nstat is None else nstat
        codes = (list(stats) + [0] * 4)[:4]
        tail = [] if ids is None else list(ids)
        tail = [len(tail)] + tail if sizes is None else [len(sizes)] + list(sizes)
        got = _ask(exe, f"{'twosample' if sizes is None else 'sizes'} {int(a_f32)} {int(b_f32)} {T} {C} {ld_a} {ld_b} {G} {nstat} "
                        f"{' '.join(str(s) for s in codes)} {width!r} {origin!r} {ld_out} {stride_out} {int(a_aligned)} {int(b_aligned)} {lds_max} "
                        f"{cu_count} {' '.join(str(int(v)) for v in tail)}")
        if "plan" in got:
            words = got.pop("plan").split()
            got["path"] = words[1]
            got.update({k: int(v) for k, v in (w.split("=") for w in words[3:])})
        return got

    return run


# ---- the paired plan ----
def test_geometry_is_that_of_the_groupby_reduction(skill):
    p = skill()  # forty years of daily steps by calendar month: one group per wave, three workgroups per tile of cells
    assert p == dict(cols=2, block=256, ctiles=782, bin_groups=3, blocks=782 * 3, bins_per_wave=1, few_groups=FEW)
    assert skill(G=4)["blocks"] == 782 and skill(G=4)["bins_per_wave"] == 1  # the seasons: one workgroup, four waves at work
    assert skill(G=366) == dict(p, bin_groups=46, blocks=782 * 46, bins_per_wave=PER_WAVE)  # day of year: kBinsPerGroup groups per workgroup
    assert skill(a_f32=True, b_f32=True)["cols"] == 4 and skill(a_f32=True)["cols"] == 2 and skill(C=101)["cols"] == 1
    assert skill(out_aligned=False)["cols"] == 1 and skill(stride_out=12 * 100_000 + 1)["cols"] == 1


def test_the_few_groups_edge(skill):
    at, past = skill(C=128, G=FEW), skill(C=128, G=FEW + 1)
    assert (at["bins_per_wave"], at["bin_groups"], at["blocks"]) == (1, 4, 4)  # 16 waves of one group
    assert (past["bins_per_wave"], past["bin_groups"], past["blocks"]) == (PER_WAVE, 3, 3)  # 8 groups per workgroup
    assert skill(C=128, G=1)["blocks"] == 1 and skill(C=128, G=2 * WAVES * PER_WAVE + 1)["bin_groups"] == 3


@pytest.mark.parametrize("f32", [(False, False), (True, False), (True, True)], ids=["f64-f64", "f32-f64", "f32-f32"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130, 256, 260])
@pytest.mark.parametrize("G", [1, 3, 4, 5, FEW, FEW + 1, 2 * WAVES * PER_WAVE + 1])
def test_the_grid_covers_every_group_and_cell_once(skill, f32, C, G):
    assert {k: v for k, v in skill("cover", a_f32=f32[0], b_f32=f32[1], T=100, C=C, G=G).items()} == dict(min=1, max=1, outside=0)


def test_tables_for_ids_in_any_order_a_missing_id_and_one_group(skill):
    ids = [2, 0, 2, 1, 0, 2, 2, 0, 1, 0]
    got = skill(T=10, C=4, G=3, ids=ids)
    assert got["rows"] == [1, 4, 7, 9, 3, 8, 0, 2, 5, 6] and got["offsets"] == [0, 4, 6, 10]  # ascending inside a group
    got = skill(T=6, C=4, G=5, ids=[4, 1, 4, 4, 1, 3])  # ids 0 and 2 never occur: empty bins first and in the middle
    assert got["rows"] == [1, 4, 5, 0, 2, 3] and got["offsets"] == [0, 0, 2, 2, 3, 6]
    got = skill(T=4, C=4, G=3, ids=[0, 0, 1, 0])  # ... and last
    assert got["rows"] == [0, 1, 3, 2] and got["offsets"] == [0, 3, 4, 4]
    got = skill(T=5, C=4, G=1, ids=[0] * 5)
    assert got["rows"] == [0, 1, 2, 3, 4] and got["offsets"] == [0, 5] and got["blocks"] == 1
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 7, 200)
    got = skill(T=200, C=4, G=7, ids=ids)
    assert got["rows"] == list(np.argsort(ids, kind="stable")) and got["offsets"] == [0] + list(np.cumsum(np.bincount(ids, minlength=7)))


def test_skill_refusals_in_their_order(skill):
    def err(**kw):
        p = skill(**kw)
        return p["error"], p["message"]

    who = "sd_skill_groups: "
    assert err(stats=(BIAS, 7)) == (INVALID, who + "unknown statistic code 7 (stats[1])")
    assert err(stats=(), nstat=0) == (INVALID, who + "nstat = 0, expected 1 to 7 statistics")
    assert err(T=0) == (INVALID, who + "bad sizes (T=0, C=100000)") and err(C=-1) == (INVALID, who + "bad sizes (T=14600, C=-1)")
    assert err(T=1 << 31, C=1) == (INVALID, who + "T = 2147483648 steps, the counts are int32 (T < 2^31)")
    assert err(ld_a=99_999) == (INVALID, who + "ld_a = 99999 is less than the 100000 cells of a row")
    assert err(ld_b=99_999) == (INVALID, who + "ld_b = 99999 is less than the 100000 cells of a row")
    assert err(ld_out=99_999) == (INVALID, who + "ld_out = 99999 is less than the 100000 cells of a row")
    assert err(stride_out=12 * 100_000 - 1) == (INVALID, who + "stride_out = 1199999 is less than the 1200000 elements of one statistic (G * ld_out)")
    assert err(T=1 << 30, C=1 << 30, ld_a=1 << 40) == (INVALID, who + "field too large")
    assert err(G=0) == (INVALID, who + "bad sizes (G=0)") and err(G=-3, stride_out=0) == (INVALID, who + "bad sizes (G=-3)")
    assert err(T=4, C=4, G=3, ids=[0, 1, 3, 0]) == (INVALID, who + "group[2] = 3 lies outside the 3 groups")
    assert err(T=4, C=4, G=3, ids=[0, -1, 3, 0]) == (INVALID, who + "group[1] = -1 lies outside the 3 groups")
    # the order: codes, nstat, sizes, T, ld_a, ld_b, ld_out, stride_out, G, the ids
    everything = dict(stats=(9,), nstat=9, T=0, C=4, ld_a=1, ld_b=1, ld_out=1, stride_out=1, G=3, ids=[0, 5, 1, 2])
    order = ["unknown statistic", "nstat = 9", "bad sizes (T=0", "ld_a = 1", "ld_b = 1", "ld_out = 1", "stride_out = 1", "group[1] = 5"]
    fixes = [dict(stats=(BIAS,)), dict(nstat=1), dict(T=4), dict(ld_a=4), dict(ld_b=4), dict(ld_out=4), dict(stride_out=12), dict(ids=[0, 2, 1, 2])]
    for words, fix in zip(order, fixes):
        assert err(**everything)[1].startswith(who + words), (words, err(**everything))
        everything.update(fix)
    assert "error" not in skill(**everything)
    # G <= 0 comes behind everything that depends on codes and sizes and before the ids; a table that cannot be made is never read
    assert err(G=0, ld_b=1)[1].startswith(who + "ld_b = 1") and err(G=0, T=4, C=4, ids=[9, 9, 9, 9])[1] == who + "bad sizes (G=0)"
    assert err(T=1 << 31, C=1, G=1)[1].startswith(who + "T = 2147483648")
    most = (1 << 31) - 1
    assert skill(T=1, C=most * 64, G=1, b_aligned=False)["blocks"] == most
    assert err(T=1, C=most * 64 + 1, G=1, b_aligned=False) == (INVALID, who + "grid too large")


# ---- the two-sample plan ----
@pytest.mark.parametrize("longest,path,K", [(320, "segment", 5), (321, "segment", 7), (448, "segment", 7), (449, "segment", 13),
                                            (832, "segment", 13), (833, "segment", 19), (1216, "segment", 19), (1217, "series", 13),
                                            (19456, "series", 19)])
def test_the_longest_group_chooses_the_path(twosample, longest, path, K):
    p = twosample(sizes=[3, longest, 0, 40], C=17)  # interleaved ids: no group but the tail of the longest is a run of rows
    assert (p["path"], p["n_max"], p["K"]) == (path, longest, K)
    if path == "series":
        chunk = 64 * K
        per = [-(-n // chunk) for n in (3, longest, 0, 40)]
        assert p["chunks"] == sum(per) and p["run_slots"] == sum(per) * chunk and p["select_blocks"] == min(4 * 17, 4 * 256)
    else:
        assert p["blocks"] == 8 * 4  # three tiles of 8 cells, rounded to 8, by four groups


def test_a_group_beyond_the_workgroup_merge_is_unsupported(twosample):
    who = "sd_twosample_groups: "
    assert twosample(sizes=[19457, 2]) == dict(error=UNSUPPORTED, message=who + "a group of 19457 samples exceeds the workgroup merge (19456)")
    assert "error" not in twosample(sizes=[19456, 19456, 1])
    # ... behind the ids, before the LDS and the 32-bit row addressing
    assert twosample(T=4, G=2, ids=[0, 2, 1, 0], lds_max=1024)["message"] == who + "group[1] = 2 lies outside the 2 groups"
    assert twosample(sizes=[19457, 2], lds_max=1024, ld_a=1 << 29)["error"] == UNSUPPORTED
    assert twosample(sizes=[5, 2], lds_max=1024) == dict(
        error=UNSUPPORTED, message=who + "two tiles of 320-row segments (41920 bytes) do not fit the LDS (1024)")
    assert twosample(sizes=[5, 2], ld_a=1 << 29)["message"] == who + "rows of 536870912 and 100 elements exceed the 32-bit row addressing"


def test_twosample_refusals_in_their_order_and_the_tables(twosample):
    def err(**kw):
        p = twosample(**kw)
        return p["error"], p["message"]

    who = "sd_twosample_groups: "
    assert err(stats=(KS, 4)) == (INVALID, who + "unknown statistic code 4 (stats[1])")
    assert err(stats=(), nstat=0) == (INVALID, who + "nstat = 0, expected 1 to 4 statistics")
    assert err(stats=(PERKINS,), width=0.0) == (INVALID, who + "width = 0, expected a positive finite bin width")
    assert "error" not in twosample(stats=(KS,), width=0.0)  # read only where Perkins is asked for
    assert err(T=0) == (INVALID, who + "bad sizes (T=0, C=100)")
    assert err(ld_b=99) == (INVALID, who + "ld_b = 99 is less than the 100 cells of a row")
    assert err(stride_out=1199) == (INVALID, who + "stride_out = 1199 is less than the 1200 elements of one statistic (G * ld_out)")
    assert err(G=0) == (INVALID, who + "bad sizes (G=0)")
    assert err(G=0, ld_a=1)[1].startswith(who + "ld_a = 1") and err(G=-1, stride_out=0, T=3, ids=[7, 7, 7]) == (INVALID, who + "bad sizes (G=-1)")
    got = twosample(T=10, C=4, G=3, ids=[2, 0, 2, 1, 0, 2, 2, 0, 1, 0])
    assert got["rows"] == [1, 4, 7, 9, 3, 8, 0, 2, 5, 6] and got["offsets"] == [0, 4, 6, 10] and (got["path"], got["K"], got["n_max"]) == ("segment", 5, 4)
    got = twosample(T=3, C=4, G=4, ids=[3, 1, 3])
    assert got["offsets"] == [0, 0, 1, 1, 3] and got["rows"] == [1, 0, 2]
    assert twosample(T=3, C=4, G=1, ids=[0, 0, 0])["offsets"] == [0, 3]
