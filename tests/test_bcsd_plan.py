"""The BCSD launch plan (scikit-downscale_amd/csrc/sd_bcsd_plan.h), checked on the host: which kernels a call launches, in which
order, over which groups, with which widths, grids and LDS sizes.  The header is compiled with g++ into a small driver
(tests/bcsd_plan_check.cpp) that reads calls on stdin and prints their plans."""
import os
import subprocess

import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024  # MI355X
CU = 256
TAS, PR = 0, 1
FIT, PREDICT, FIT_PREDICT = 0, 1, 2
SWITCHES = ("path_v1", "no_fused", "no_rs_split", "no_dma", "no_full", "no_compact")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "bcsd_plan_check"
    src = os.path.join(ROOT, "tests", "bcsd_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(fit_len, predict_len=None, op=FIT_PREDICT, kind=TAS, detrend=False, C=100_000, ld=None, ld_p=None, ld_out=None, aligned=True,
            lds_max=LDS, **switches):
        assert set(switches) <= set(SWITCHES), switches
        ld, ld_p, ld_out = (C if v is None else v for v in (ld, ld_p, ld_out))
        if op != FIT and predict_len is None:
            predict_len = fit_len
        head = [op, kind, int(detrend), len(fit_len), C, ld, ld_p, ld_out, int(aligned), lds_max, CU] + [int(switches.get(s, False)) for s in SWITCHES]
        line = " ".join(map(str, head + list(fit_len) + (list(predict_len) if op != FIT else [])))
        out = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return {"error": int(code), "message": msg}
        launches = []
        for ln in lines[:-2]:
            f = ln.split()
            launches.append(dict(name=f[0], width=int(f[2]), ident=bool(int(f[3])), gmask=int(f[4]), rs=int(f[5]), slab_k=int(f[6]),
                                 list=int(f[7]), lds=int(f[8]), grid=(int(f[9]), int(f[10])), block=int(f[11])))
        p = [int(x) for x in lines[-2].split()[1:]]
        return {"launches": launches, "via_state": bool(p[0]), "rank_apply": bool(p[1]), "identity": bool(p[2]), "fused": bool(p[3]), "nmax": p[4]}

    return run


def month_lengths(T, start="1980-01-01", calendar=None):
    if calendar == "360_day":  # 30-day months
        return [T // 360 * 30 + min(max(T % 360 - 30 * m, 0), 30) for m in range(12)]
    idx = pd.date_range(start, periods=T, freq="D")
    return [int((idx.month == m + 1).sum()) for m in range(12)]


def mask(groups):
    return sum(1 << g for g in groups)


def tiled(C, gmask, G=12):
    return 8 * (((C + 7) // 8 + 7) // 8) * (bin(gmask).count("1") if gmask else G)


def names(p):
    return [(L["name"], L["width"], L["gmask"]) for L in p["launches"]]


MONTHS = month_lengths(14600)  # bench config 2 / 3: 40 years of daily steps from 1980-01-01
WHOLE = mask(g for g, n in enumerate(MONTHS) if n % 20 == 0)
RAGGED = mask([1, 11])  # February (1 130 samples) and December (1 230: the series ends on 2019-12-21)
NARROW = mask(g for g, n in enumerate(MONTHS) if n <= 64 * 19)  # the months the 19-wide register-sort kernels serve
WIDE = mask(range(12)) & ~NARROW


def fd_lds(n):  # [head: 88 doubles][tile: (ceil(n / 20) + 16) chunks of 1 032 B]
    return 88 * 8 + ((n + 19) // 20 + 16) * 1032


def test_headline_fit_predict_runs_both_sets_on_the_dma_kernel(plan):
    assert MONTHS[1] == 1130 and MONTHS[11] == 1230 and WHOLE == mask(range(12)) & ~RAGGED
    p = plan(MONTHS)
    assert names(p) == [("bcsd_fd_kernel", 20, WHOLE), ("bcsd_fd_kernel_ragged", 20, RAGGED), ("bcsd_rs_rank_kernel", 21, 0),
                        ("bcsd_rs_apply_kernel", 21, 0)]
    fd, rag, rank, apply = p["launches"]
    assert fd["lds"] == fd_lds(1240) and fd["rs"] == 16 * ((1240 + 19) // 20 + 16) and fd["grid"] == (tiled(100_000, WHOLE), 1)
    assert rag["lds"] == fd_lds(1230) and rag["grid"] == (tiled(100_000, RAGGED), 1) and fd["block"] == rag["block"] == 512
    assert rank["list"] == apply["list"] == 1 and rank["grid"] == apply["grid"] == (2 * CU, 1)
    assert not rank["ident"] and apply["ident"] and rank["slab_k"] == 21
    assert p["fused"] and p["identity"] and p["rank_apply"] and not p["via_state"] and p["nmax"] == 1240


@pytest.mark.parametrize("kw", [dict(C=99_999), dict(ld=100_001), dict(ld_out=100_001), dict(aligned=False), dict(C=6)])
def test_fields_the_dma_kernel_cannot_take_go_to_the_register_tile_kernel(plan, kw):
    p = plan(MONTHS, **kw)
    C = kw.get("C", 100_000)
    assert names(p) == [("bcsd_fx_kernel_full", 20, WHOLE), ("bcsd_fx_kernel", 20, RAGGED), ("bcsd_rs_rank_kernel", 21, 0),
                        ("bcsd_rs_apply_kernel", 21, 0)]
    assert p["launches"][0]["grid"] == (tiled(C, WHOLE), 1)
    assert p["launches"][0]["lds"] == p["launches"][1]["lds"] == (8 * p["launches"][0]["rs"] + 88) * 8


def test_a_ragged_set_with_a_short_group_leaves_the_dma_kernel(plan):
    lens = list(MONTHS)
    lens[1] = 630  # shortest ragged group <= 640 samples: 32 lanes of data or fewer
    assert names(plan(lens)) == [("bcsd_fd_kernel", 20, WHOLE), ("bcsd_fx_kernel", 20, RAGGED), ("bcsd_rs_rank_kernel", 21, 0),
                                 ("bcsd_rs_apply_kernel", 21, 0)]
    lens = list(MONTHS)
    lens[0] = 1280  # two workgroups of the whole-lane set no longer fit a CU: it takes the register tiles, the ragged set stays
    assert names(plan(lens))[:2] == [("bcsd_fx_kernel_full", 20, WHOLE), ("bcsd_fd_kernel_ragged", 20, RAGGED)]


def test_predict_from_a_state_never_takes_the_dma_kernel(plan):
    p = plan(MONTHS, op=PREDICT)
    assert names(p) == [("bcsd_fx_kernel_full", 20, WHOLE), ("bcsd_fx_kernel", 20, RAGGED), ("bcsd_rs_rank_kernel", 21, 0),
                        ("bcsd_rs_apply_kernel", 21, 0)]
    assert p["rank_apply"] and p["fused"]


def test_precipitation_fit_predict_takes_the_compacting_kernel(plan):
    p = plan(MONTHS, kind=PR)
    assert names(p) == [("bcsd_fxc_kernel_full", 20, WHOLE), ("bcsd_fxc_kernel", 20, RAGGED), ("bcsd_fxp_kernel_list", 20, 0),
                        ("bcsd_rs_rank_kernel", 21, 0), ("bcsd_rs_apply_kernel", 21, 0)]
    lst = p["launches"][2]
    assert lst["list"] == 2 and lst["grid"] == (2 * CU, 1) and lst["ident"]
    assert [L["list"] for L in p["launches"][3:]] == [1, 1]
    # predict from a state: the register-tile precipitation kernels
    assert names(plan(MONTHS, op=PREDICT, kind=PR))[:2] == [("bcsd_fxp_kernel_full", 20, WHOLE), ("bcsd_fxp_kernel", 20, RAGGED)]


def test_unequal_fit_and_predict_lengths(plan):
    p = plan(MONTHS, month_lengths(3000))
    assert names(p) == [("bcsd_fx_kernel", 20, 0), ("bcsd_rs_rank_kernel", 21, 0), ("bcsd_rs_apply_kernel", 21, 0)]
    assert not p["identity"] and not p["launches"][0]["ident"] and not p["launches"][2]["ident"]
    longer = month_lengths(20000)
    assert max(longer) == 1705
    p = plan(MONTHS, longer)
    assert names(p) == [("bcsd_rs_rank_kernel", 33, 0), ("bcsd_rs_apply_kernel", 33, 0)]
    assert not p["fused"] and [L["list"] for L in p["launches"]] == [0, 0] and p["launches"][0]["grid"] == (tiled(100_000, 0), 1)


def test_more_than_64_groups_have_no_group_masks(plan):
    p = plan([1240] * 65)
    assert names(p) == [("bcsd_fx_kernel", 20, 0), ("bcsd_rs_rank_kernel", 21, 0), ("bcsd_rs_apply_kernel", 21, 0)]
    assert p["launches"][0]["grid"] == (tiled(100_000, 0, G=65), 1)


def test_detrend_takes_rank_apply_only(plan):
    p = plan(MONTHS, detrend=True)
    assert names(p) == [("bcsd_rs_rank_kernel", 21, WIDE), ("bcsd_rs_rank_kernel", 19, NARROW), ("bcsd_rs_apply_kernel", 21, WIDE),
                        ("bcsd_rs_apply_kernel", 19, NARROW)] and not p["fused"]
    assert names(plan(MONTHS, op=FIT, detrend=True)) == [("bcsd_rs_fit_kernel", 21, WIDE), ("bcsd_rs_fit_kernel", 19, NARROW)]


def test_a_360_day_calendar_is_all_whole_lanes(plan):
    lens = month_lengths(14400, calendar="360_day")
    assert lens == [1200] * 12
    assert names(plan(lens)) == [("bcsd_fd_kernel", 20, mask(range(12))), ("bcsd_rs_rank_kernel", 19, 0), ("bcsd_rs_apply_kernel", 19, 0)]


@pytest.mark.parametrize("n,K", [(256, 4), (257, 8), (512, 8), (513, 12), (768, 12), (769, 16), (1024, 16), (1025, 20), (1280, 20),
                                 (1281, 24), (1536, 24)])
def test_fused_width_ladder(plan, n, K):
    p = plan([n, n - 1], C=1000)
    assert p["launches"][0]["width"] == K and p["fused"]


@pytest.mark.parametrize("n,K", [(320, 5), (321, 13), (832, 13), (833, 19), (1216, 19), (1217, 21), (1344, 21), (1345, 33), (1537, 33),
                                 (2112, 33)])
def test_register_sort_ladder(plan, n, K):
    assert names(plan([n], op=FIT, C=1000)) == [("bcsd_rs_fit_kernel", K, 0)]


def test_beyond_the_fused_kernels_and_the_register_sort(plan):
    assert names(plan([1537], C=1000)) == [("bcsd_rs_rank_kernel", 33, 0), ("bcsd_rs_apply_kernel", 33, 0)]
    p = plan([2113], op=FIT, C=1000)
    assert names(p) == [("bcsd_long_fit_kernel", 3, 0)] and p["launches"][0]["grid"] == (1000, 1) and p["launches"][0]["block"] == 1024
    p = plan([2113, 2000], C=1000)
    assert p["via_state"] and names(p) == [("bcsd_long_fit_kernel", 3, 0), ("bcsd_long_predict_kernel", 3, 0)]
    assert names(plan([19456], op=FIT, C=10)) == [("bcsd_long_fit_kernel", 19, 0)]
    assert names(plan([19457], op=FIT, C=10))[0][0] == "bcsd_fit_kernel"


def test_the_19_21_split_of_rank_and_apply(plan):
    lens = [1216, 1217, 1300, 1000]
    p = plan(lens, C=1000, no_fused=True)
    assert names(p) == [("bcsd_rs_rank_kernel", 21, mask([1, 2])), ("bcsd_rs_rank_kernel", 19, mask([0, 3])),
                        ("bcsd_rs_apply_kernel", 21, mask([1, 2])), ("bcsd_rs_apply_kernel", 19, mask([0, 3]))]
    assert {L["slab_k"] for L in p["launches"]} == {21} and len({L["rs"] for L in p["launches"]}) == 1
    assert names(plan(lens, op=FIT, C=1000)) == [("bcsd_rs_fit_kernel", 21, mask([1, 2])), ("bcsd_rs_fit_kernel", 19, mask([0, 3]))]
    # behind the fused kernels RANK / APPLY walk the work list in one launch each
    assert names(plan(lens, C=1000))[-2:] == [("bcsd_rs_rank_kernel", 21, 0), ("bcsd_rs_apply_kernel", 21, 0)]


def test_a_20000_sample_fit_takes_the_generic_kernel(plan):
    p = plan([20000], op=FIT, C=10)
    assert names(p) == [("bcsd_fit_kernel", 1, 0)]
    L = p["launches"][0]
    assert L["rs"] == 20001 and L["lds"] == 20001 * 8 and L["grid"] == (10, 1) and L["block"] == 64


def test_segments_beyond_every_kernel_are_refused(plan):
    p = plan([20000], op=PREDICT, C=10)
    assert p["error"] == 3 and p["message"] == "BCSD segment of 20000 samples does not fit the 163840-byte LDS"
    p = plan([20000], C=10)  # fit + predict: the fit would run, the predict does not fit
    assert p["error"] == 3 and "does not fit" in p["message"]
    p = plan([20000], op=FIT, C=10, detrend=True)
    assert p["error"] == 3 and p["message"] == "detrended quantile mapping serves group segments of up to 19456 samples (longest here: 20000)"


def test_pitches_of_2_29_elements_take_the_generic_kernels(plan):
    big = 1 << 29
    p = plan(MONTHS, C=64, ld_out=big)
    assert p["via_state"]
    assert [n for n, _, _ in names(p)] == ["bcsd_rs_fit_kernel", "bcsd_rs_fit_kernel", "bcsd_predict_kernel"]
    assert [n for n, _, _ in names(plan(MONTHS, C=64, ld=big))] == ["bcsd_fit_kernel", "bcsd_fx_kernel_full", "bcsd_fx_kernel",
                                                                      "bcsd_rs_rank_kernel", "bcsd_rs_apply_kernel"]
    assert names(plan(MONTHS, op=FIT, C=64, ld=big - 1))[0][0] == "bcsd_rs_fit_kernel"


@pytest.mark.parametrize("switch", SWITCHES)
def test_each_development_switch(plan, switch):
    base = names(plan(MONTHS))
    got = names(plan(MONTHS, **{switch: True}))
    if switch == "path_v1":
        assert [n for n, _, _ in got] == ["bcsd_fit_kernel", "bcsd_predict_kernel"]
    elif switch == "no_fused":
        assert got == [("bcsd_rs_rank_kernel", 21, WIDE), ("bcsd_rs_rank_kernel", 19, NARROW), ("bcsd_rs_apply_kernel", 21, WIDE),
                       ("bcsd_rs_apply_kernel", 19, NARROW)]
        assert names(plan(MONTHS, no_fused=True, no_rs_split=True)) == [("bcsd_rs_rank_kernel", 21, 0), ("bcsd_rs_apply_kernel", 21, 0)]
    elif switch == "no_rs_split":
        assert got == base
        assert names(plan(MONTHS, op=FIT, no_rs_split=True)) == [("bcsd_rs_fit_kernel", 21, 0)]
    elif switch == "no_dma":
        assert got == [("bcsd_fx_kernel_full", 20, WHOLE), ("bcsd_fx_kernel", 20, RAGGED)] + base[2:]
    elif switch == "no_full":
        assert got == [("bcsd_fx_kernel", 20, 0)] + base[2:]
        assert names(plan(MONTHS, kind=PR, no_full=True))[:2] == [("bcsd_fxc_kernel", 20, mask(range(12))), ("bcsd_fxp_kernel_list", 20, 0)]
    elif switch == "no_compact":
        assert got == base
        assert names(plan(MONTHS, kind=PR, no_compact=True))[:2] == [("bcsd_fxp_kernel_full", 20, WHOLE), ("bcsd_fxp_kernel", 20, RAGGED)]
