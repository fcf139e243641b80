"""The analog launch plan (scikit-downscale_amd/csrc/sd_analog_plan.h), checked on the host: which kernels a PureAnalog /
AnalogRegression call launches, with which widths, grids and LDS sizes.  The header is compiled with g++ into a small driver
(tests/analog_plan_check.cpp) that reads calls on stdin and prints their plans.  The expectations restate the conditions the entry
points of csrc/sd_analog.hip carried inline before the plan existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024  # MI355X
CU = 256
BEST, SAMPLE, WEIGHT, MEAN = 0, 1, 2, 3
FIT, PREDICT, REGRESS, FIT_PREDICT = 0, 1, 2, 3
NONE, MEAN3, MEANK, WINDOW, WALK, SLAB, BF2, BF, FUSED, SPLIT = range(10)
SWITCHES = ("no_slab", "heap", "no_tile", "reg_prefix", "no_runs", "runs_always", "readlane")
NUMBERS = (("slab_classes", -1), ("prune_at", -1), ("ablate", 0))


def sort2_width(T, lds_max=LDS):
    for K in (5, 9, 13, 15, 17, 19):
        if T <= 1024 * K and T <= 65535 and 8 * ((T + K - 1) // K * K + 1) + 4 * 1025 <= lds_max:
            return K
    return 0


def bf2_lds(k, F, it):
    return (k * 64 * (8 + it) + 15) // 16 * 16 + F * 64 * 8 + 64 * 4


def state(T, F, lds_max=LDS, pq=False, rx=False, no_slab=False):
    """what sd_analog_fit leaves behind for a series of T samples"""
    f1 = F == 1 and sort2_width(T, lds_max) != 0 and 8 * (T + 1) <= lds_max
    return dict(has_xs=f1, has_yx=f1, has_ybar=f1, has_ps=F > 1 and sort2_width(T, lds_max) != 0 and not no_slab, has_pq=pq, has_rx=rx)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "analog_plan_check"
    src = os.path.join(ROOT, "tests", "analog_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(op, T=14600, F=1, C=100_000, Tq=14600, k=30, kind=MEAN, thresh=False, neighbors=False, sample=False, ld=None, ld_q=None,
            ld_out=None, lds_max=LDS, cu=CU, cc=None, st=None, **kw):
        ld, ld_q, ld_out = (C if v is None else v for v in (ld, ld_q, ld_out))
        st = dict(state(T, F, lds_max, no_slab=kw.get("no_slab", False)) if st is None and op in (PREDICT, REGRESS) else (st or {}))
        for key in ("has_pq", "has_rx"):
            if key in kw:
                st[key] = kw.pop(key)
        assert set(kw) <= set(SWITCHES) | {n for n, _ in NUMBERS}, kw
        cc = min(C, 4096 if F > 1 else 16384) if cc is None else cc
        words = [op, T, F, C, Tq, k, kind, int(thresh), int(neighbors), int(sample), ld, ld_q, ld_out, lds_max, cu]
        words += [int(st.get(s, False)) for s in ("has_xs", "has_yx", "has_ybar", "has_ps", "has_pq", "has_rx")]
        words += [int(kw.get(s, False)) for s in SWITCHES] + [kw.get(n, dflt) for n, dflt in NUMBERS] + [cc]
        out = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return {"error": int(code), "message": msg}
        p = {k_: int(v) for k_, v in (w.split("=") for w in lines[0].split()[1:])}
        # geometry of the launches the operation can make (whether one runs is in the decisions above): (grid, block, LDS bytes)
        p["g"] = {f[0]: ((int(f[1]), int(f[2]), int(f[3])), int(f[4]), int(f[5])) for f in (ln.split() for ln in lines[1:-1])}
        return p

    return run


def tiled(C, rows):
    return 8 * (((C + 7) // 8 + 7) // 8) * rows


# ---- the bench configurations ---------------------------------------------------------------------------------------------
def test_config_4_is_one_fused_kernel_per_chunk(plan):
    assert sort2_width(14600) == 15
    p = plan(FIT_PREDICT)
    assert (p["path"], p["K"], p["np_runs"], p["tiled"], p["runs_q"], p["skip_prob"], p["chunk"], p["nb"]) == (FUSED, 15, 15360, 1, 0, 1, 16384, 256)
    assert p["lds"] == 8 * 15361 + 4 * 1026 + 29200
    g = p["g"]
    assert g["tile_sort"] == ((tiled(100_000, 16), 1, 1), 512, 8 * (8 * 962 + 88))
    assert g["stage_in"] == ((512, 457, 1), 256, 0)  # plain transposes
    assert g["per_cell"] == ((256, 1, 1), 1024, p["lds"])
    assert g["stage_out"] == ((512, 457, 2), 256, 0) and g["status_public"][0] == (391, 1, 1)
    # the last chunk of the 100 000 cells
    assert plan(FIT_PREDICT, cc=100_000 - 6 * 16384)["g"]["per_cell"][0] == (256, 1, 1)
    assert plan(FIT_PREDICT, thresh=True)["path"] == SPLIT and plan(FIT_PREDICT, kind=WEIGHT)["path"] == SPLIT
    assert plan(FIT_PREDICT, k=1, kind=WEIGHT)["path"] == FUSED  # a single analog is best_analog


def test_fit_of_the_bench_series(plan):
    p = plan(FIT)
    assert (p["sorted"], p["K"], p["tiled"], p["np_runs"], p["tagged"], p["Ks"]) == (1, 15, 1, 15360, 1, 0)
    g = p["g"]
    assert g["sort2_tagged"] == ((1024, 1, 1), 1024, 8 * 15361 + 4100)  # the presorted runs are padded to 16 x 960
    assert g["sort2_exact"] == ((256, 1, 1), 1024, 8 * 15361 + 4100)
    assert g["tile_sort"] == ((tiled(100_000, 16), 1, 1), 512, 8 * (8 * 962 + 88))


def test_default_pure_analog_takes_the_window_kernel(plan):
    p = plan(PREDICT, k=200, kind=BEST)
    assert (p["path"], p["npass"], p["runs_q"], p["skip_prob"], p["need_pq"], p["lds"]) == (WINDOW, 2, 1, 0, 0, 8 * (2 * 7701 + 1))
    g = p["g"]
    assert g["stage_in"] == ((tiled(16384, 15), 1, 1), 512, 8 * (8 * 1058 + 88))  # value-ordered runs
    assert g["per_cell"] == ((256, 1, 1), 1024, p["lds"])
    assert g["stage_out"] == ((tiled(16384, 15), 3, 1), 512, 8 * (8 * 1026 + 88))


def test_mean_and_weight_analogs_from_a_state(plan):
    p = plan(PREDICT)
    assert (p["path"], p["per"], p["runs_q"], p["skip_prob"], p["lds"]) == (MEAN3, 16, 0, 1, 8 * 14601)
    assert p["g"]["stage_in"][1] == p["g"]["stage_out"][1] == 256 and p["g"]["stage_out"][0] == (512, 457, 2)
    p = plan(PREDICT, kind=WEIGHT)
    assert (p["path"], p["runs_q"], p["skip_prob"], p["need_pq"], p["chunk_qsplit"], p["reg_direct"]) == (MEANK, 1, 1, 0, 1, 0)
    assert p["g"]["stage_out"][0] == (tiled(16384, 15), 2, 1) and p["g"]["per_cell"] == ((256, 1, 1), 1024, 8 * 14601)
    p = plan(PREDICT, thresh=True)  # thresholded mean: the analog values themselves, probability plane written
    assert (p["path"], p["skip_prob"], p["need_pq"]) == (MEANK, 0, 0)


def test_analog_regression(plan):
    p = plan(REGRESS)  # k = 30: direct sums
    assert (p["path"], p["reg_direct"], p["chunk_qsplit"], p["need_pq"], p["need_rx"], p["runs_q"], p["skip_prob"]) == (MEANK, 1, 1, 0, 0, 1, 1)
    p = plan(REGRESS, k=200)  # the default n_analogs: prefix differences, built once
    assert (p["path"], p["reg_direct"], p["chunk_qsplit"], p["need_pq"], p["need_rx"]) == (MEANK, 0, 2, 1, 1)
    assert p["g"]["prefix_sums"] == p["g"]["rx"] == ((512, 1, 1), 1024, 8 * 14601)
    p = plan(REGRESS, k=200, has_pq=True, has_rx=True)
    assert (p["need_pq"], p["need_rx"]) == (0, 0)
    assert plan(REGRESS, k=2)["path"] == WINDOW  # fewer than three analogs: no regression line
    assert plan(REGRESS, thresh=True)["path"] == WALK  # logistic fit and subset OLS need the analogs themselves


def test_three_features_take_the_slab_search(plan):
    f = plan(FIT, F=3, C=16384)
    assert (f["sorted"], f["Ks"], f["tagged"], f["tiled"]) == (0, 15, 1, 0)
    g = f["g"]
    assert g["transpose"] == ((512, 457, 1), 256, 0) and g["sort2_tagged"] == ((1024, 1, 1), 1024, 8 * 14611 + 4100)
    assert g["sort2_exact"][0] == (256, 1, 1) and g["gather_sorted"] == ((16384, 1, 1), 256, 0)
    p = plan(PREDICT, F=3, C=16384)
    assert (p["path"], p["topk"], p["nclass"], p["Kq"], p["chunk"], p["nb"], p["nthr"], p["prune_at"], p["use_mfma"], p["tagged"]) == (
        SLAB, 1, 8, 15, 4096, 1024, 256, 16, 1, 1)
    g = p["g"]
    assert g["transpose"] == ((128, 457, 1), 256, 0) and g["slab_aux"] == ((2048, 1, 1), 256, 0)
    assert g["sort2_tagged"][0] == (1024, 1, 1) and g["sort2_exact"][0] == (256, 1, 1)
    assert g["slab_topk"] == ((4096 * 229, 1, 1), 64, 10 * 32 * 64)


# ---- every limit, both sides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,F,topk", [(30, 3, 1), (31, 3, 0), (30, 6, 1), (30, 7, 0)])
def test_top_k_limits(plan, k, F, topk):
    p = plan(PREDICT, F=F, C=4096, k=k)
    assert p["path"] == SLAB and p["topk"] == topk
    assert p["lds"] == (10 * 32 * 64 if topk else bf2_lds(k, F, 2))
    assert p["g"]["slab_topk"] == ((4096 * 229, 1, 1), 64, p["lds"]) and p["g"]["slab_heap"] == ((4096 * 229, 1, 1), 64, bf2_lds(k, F, 2))


def test_short_query_series_have_fewer_classes(plan):
    assert [plan(PREDICT, F=2, C=64, Tq=tq)["nclass"] for tq in (100, 1023, 1024, 2048, 4095, 4096, 14600)] == [1, 1, 2, 4, 7, 8, 8]


@pytest.mark.parametrize("k,direct", [(64, 1), (65, 0)])
def test_direct_regression_limit(plan, k, direct):
    p = plan(REGRESS, k=k)
    assert (p["reg_direct"], p["need_pq"], p["need_rx"], p["qsplit"]) == (direct, 1 - direct, 1 - direct, 2 - direct)


def test_query_runs_and_qsplit_limits(plan):
    assert [plan(PREDICT, kind=WEIGHT, Tq=tq)["runs_q"] for tq in (2047, 2048)] == [0, 1]
    assert [plan(REGRESS, k=200, Tq=tq)["chunk_qsplit"] for tq in (4095, 4096)] == [1, 2]
    # only when every XCD still gets whole groups of workgroups, and every workgroup a cell
    assert plan(REGRESS, k=200, C=100)["chunk_qsplit"] == 1  # 104 workgroups
    assert plan(REGRESS, k=200, C=16384, cc=255)["chunk_qsplit"] == 1 and plan(REGRESS, k=200, C=16384, cc=256)["chunk_qsplit"] == 2


def test_tags_and_the_tile_sort_end_at_16384_samples(plan):
    a, b = plan(FIT, T=16384), plan(FIT, T=16385)
    assert (a["K"], a["tiled"], a["tagged"], a["np_runs"]) == (17, 1, 1, 16 * 1088) and (b["K"], b["tiled"], b["tagged"], b["sorted"]) == (17, 0, 0, 1)
    assert b["g"]["sort2_exact"] == ((1024, 1, 1), 1024, 8 * (16388 + 1) + 4100)  # no tagged pass: the exact one over every cell
    # (the fused kernel ends earlier: at 17 samples per thread keys, co-ranks and tags need 8 * 16321 + 4104 + 2 * T + 512 bytes)
    assert [plan(FIT_PREDICT, T=T)["path"] for T in (15360, 15361, 16384, 16385)] == [FUSED, SPLIT, SPLIT, SPLIT]
    # widths 13 / 15 / 17 only (at most 16 chunks of 64 * K follows from T <= 1024 * K: shadowed)
    assert [(plan(FIT, T=T)["K"], plan(FIT, T=T)["tiled"]) for T in (9216, 9217, 13312, 13313, 15360, 15361)] == [
        (9, 0), (13, 1), (13, 1), (15, 1), (15, 1), (17, 1)]
    assert plan(FIT_PREDICT, T=9216)["path"] == SPLIT
    q = plan(PREDICT, F=2, C=64, T=1000, Tq=16385)
    assert q["path"] == SLAB and q["tagged"] == 0 and plan(PREDICT, F=2, C=64, T=1000, Tq=16384)["tagged"] == 1


def test_the_fused_kernel_answers_up_to_16384_queries(plan):
    assert plan(FIT_PREDICT, Tq=16384)["path"] == FUSED and plan(FIT_PREDICT, Tq=16385)["path"] == SPLIT


@pytest.mark.parametrize("T,K", [(5120, 5), (5121, 9), (9216, 9), (9217, 13), (13312, 13), (13313, 15), (15360, 15), (15361, 17), (17408, 17),
                                 (17409, 19), (19456, 19), (19457, 0)])
def test_sort_width_ladder(plan, T, K):
    p = plan(FIT, T=T, C=100)
    assert (p["K"], p["sorted"]) == (K, int(K != 0))
    assert plan(FIT, T=T, F=2, C=100)["Ks"] == K
    if K == 0:  # no sorted view, no slab copy beyond
        assert (p["tiled"], p["tagged"]) == (0, 0)
        assert plan(PREDICT, T=T, C=100)["path"] == BF2 and plan(PREDICT, T=T, F=2, C=100)["path"] == BF2
        assert plan(PREDICT, T=1000, F=2, C=100, Tq=T)["path"] == BF2  # the queries are sorted by the same kernels


def test_sort_width_at_a_64_kb_lds(plan):
    small = 64 * 1024
    assert (plan(FIT, T=7670, C=100, lds_max=small)["K"], plan(FIT, T=7700, C=100, lds_max=small)["sorted"]) == (9, 0)


def test_heap_sizes_decide_between_slab_scanner_and_brute_force(plan):
    slab_max = max(k for k in range(1, 400) if bf2_lds(k, 3, 2) <= LDS)
    bf2_max = max(k for k in range(1, 400) if bf2_lds(k, 3, 4) <= LDS)
    assert (slab_max, bf2_max) == (253, 211) and max(k for k in range(1, 400) if bf2_lds(k, 8, 4) <= LDS) == 207  # "k > 208"
    assert [plan(PREDICT, F=3, C=64, k=k)["path"] for k in (slab_max, slab_max + 1)] == [SLAB, BF]
    p = plan(PREDICT, F=3, C=64, k=bf2_max, no_slab=True)
    assert (p["path"], p["it_bytes"], p["lds"]) == (BF2, 2, bf2_lds(bf2_max, 3, 2))
    assert p["g"]["bf2"] == ((64 * 229, 1, 1), 64, p["lds"])
    p = plan(PREDICT, F=3, C=64, k=bf2_max + 1, no_slab=True)
    assert (p["path"], p["lds"], p["nb"], p["nthr"]) == (BF, 8 * 3 * 1024, 64, 256)
    assert p["g"]["per_cell"] == ((64, 1, 1), 256, p["lds"])


@pytest.mark.parametrize("T,it", [(65535, 2), (65536, 4)])
def test_heap_indices_are_16_bit_up_to_65535_samples(plan, T, it):
    p = plan(PREDICT, T=T, F=2, C=8, Tq=100, k=5)  # (no slab copy beyond 19 456 samples)
    assert (p["path"], p["it_bytes"], p["lds"]) == (BF2, it, bf2_lds(5, 2, it)) and p["g"]["bf2"] == ((16, 1, 1), 64, p["lds"])


@pytest.mark.parametrize("T,per", [(8192, 8), (8193, 16), (16384, 16), (16385, 20), (19456, 20)])
def test_mean3_generations(plan, T, per):
    p = plan(PREDICT, T=T, Tq=1000, C=100)
    assert (p["path"], p["per"], p["lds"]) == (MEAN3, per, 8 * (T + 1))


@pytest.mark.parametrize("T,npass", [(9838, 1), (9839, 2)])
def test_window_passes(plan, T, npass):
    p = plan(PREDICT, T=T, k=200, kind=BEST, Tq=1000, C=100)
    assert (p["path"], p["npass"]) == (WINDOW, npass) and p["lds"] == 8 * (2 * (-(-T // npass) + 401) + 1)


def test_calls_that_need_the_neighbours_walk(plan):
    for kw in (dict(neighbors=True), dict(kind=SAMPLE, sample=True)):
        p = plan(PREDICT, **kw)
        assert p["path"] == WALK and p["chunk"] == 0 and p["g"]["per_cell"] == ((256, 1, 1), 1024, 8 * 14600)
    p = plan(PREDICT, k=1, kind=WEIGHT)
    assert (p["kind"], p["path"]) == (BEST, MEAN3)
    assert plan(REGRESS, k=1)["kind"] == MEAN


def test_persistent_grids_are_multiples_of_eight(plan):
    assert plan(PREDICT, cu=250)["nb"] == 248 and plan(PREDICT, cu=4)["nb"] == 8 and plan(PREDICT, C=100)["nb"] == 104
    assert plan(PREDICT, C=100)["g"]["per_cell"][0] == (104, 1, 1)
    assert plan(PREDICT, cc=50)["g"]["per_cell"][0] == (56, 1, 1)
    assert plan(PREDICT, F=2, cu=250)["nb"] == 1000 and plan(FIT_PREDICT, cu=250)["nb"] == 248
    assert plan(PREDICT)["chunk"] == 16384 and plan(PREDICT, F=2)["chunk"] == 4096  # (halving needs 2^25 queries: shadowed by the sort width)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors(plan):
    def err(*a, **kw):
        p = plan(*a, **kw)
        return p["error"], p["message"]

    assert err(FIT, T=0) == err(FIT, C=10, ld=9) == (1, "sd_analog_fit: bad sizes")
    assert err(FIT, F=0) == (1, "sd_analog_fit: F=0 outside [1,8]") and err(FIT, F=9) == (1, "sd_analog_fit: F=9 outside [1,8]")
    assert err(PREDICT, Tq=0) == err(PREDICT, ld_q=99_999) == err(REGRESS, ld_out=99_999) == (1, "sd_analog_predict: bad sizes")
    assert err(PREDICT, k=0) == (1, "sd_analog_predict: k=0 must be in [1, T=14600]")
    assert err(PREDICT, k=14601) == (1, "sd_analog_predict: k=14601 must be in [1, T=14600]")
    assert err(PREDICT, kind=4) == (1, "sd_analog_predict: unknown kind 4") and "error" not in plan(REGRESS, kind=4)
    assert err(PREDICT, kind=SAMPLE) == (1, "sd_analog_predict: sample_analogs needs sample_inds")
    assert err(PREDICT, T=19456, k=5000, C=10) == (1, "sd_analog_predict: k=5000 too large for the windowed path")
    assert err(PREDICT, T=1000, F=2, C=1 << 24, Tq=20000, k=5) == (1, "sd_analog_predict: too many (cell, query batch) pairs for one launch")
    assert err(FIT_PREDICT, Tq=0) == err(FIT_PREDICT, ld=5) == (1, "sd_analog_fit_predict: bad sizes")
    assert err(FIT_PREDICT, F=9) == (1, "sd_analog_fit_predict: F=9 outside [1,8]")
    assert err(FIT_PREDICT, k=0) == (1, "sd_analog_fit_predict: k=0 must be in [1, T=14600]")
    assert err(FIT_PREDICT, kind=SAMPLE) == (1, "sd_analog_fit_predict: kind 1 (sample_analogs needs the split calls)")
    assert err(FIT, T=16384, C=(1 << 31) - 1) == err(FIT_PREDICT, C=(1 << 31) - 1) == (1, "analog fit: grid too large")
    # value-ordered runs of 2^30 queries: 2^20 runs x 2 048 workgroups per chunk (a fused call has at most 16 runs: no such error there)
    assert err(PREDICT, kind=WEIGHT, C=16384, Tq=1 << 30) == err(REGRESS, C=16384, Tq=1 << 30) == (1, "analog predict: grid too large")
    assert "error" not in plan(PREDICT, kind=WEIGHT, C=16384, Tq=(1 << 30) - 1024) and "error" not in plan(PREDICT, C=16384, Tq=1 << 30)
    assert plan(FIT_PREDICT, C=1 << 20, Tq=16384, runs_always=True)["g"]["stage_in"][0] == (tiled(16384, 16), 1, 1)


# ---- development switches -----------------------------------------------------------------------------------------------------
def test_each_switch_flips_the_decision_it_names(plan):
    def changed(a, b):
        return {k for k in a if k != "g" and a[k] != b[k]}

    base = plan(PREDICT, F=3, C=4096)
    p = plan(PREDICT, F=3, C=4096, st=state(14600, 3), no_slab=True)
    assert p["path"] == BF2 and plan(FIT, F=3, no_slab=True)["Ks"] == 0
    assert changed(base, plan(PREDICT, F=3, C=4096, heap=True)) == {"topk", "lds"}
    assert changed(base, plan(PREDICT, F=3, C=4096, slab_classes=1)) == {"nclass"} and plan(PREDICT, F=3, C=4096, slab_classes=20)["nclass"] == 8
    assert changed(base, plan(PREDICT, F=3, C=4096, readlane=True)) == {"use_mfma"}
    assert changed(base, plan(PREDICT, F=3, C=4096, prune_at=8)) == {"prune_at"} and plan(PREDICT, F=3, C=4096, prune_at=99)["prune_at"] == 32
    assert changed(base, plan(PREDICT, F=3, C=4096, ablate=4)) == {"ablate"}
    assert changed(plan(FIT), plan(FIT, no_tile=True)) == {"tiled", "np_runs"}
    assert plan(FIT, no_tile=True)["g"]["sort2_tagged"][2] == 8 * 14611 + 4100 and "tile_sort" not in plan(FIT, no_tile=True)["g"]
    assert plan(FIT_PREDICT, no_tile=True)["path"] == SPLIT
    assert changed(plan(REGRESS), plan(REGRESS, reg_prefix=True)) == {"reg_direct", "need_pq", "need_rx", "qsplit", "chunk_qsplit"}
    assert changed(plan(PREDICT, kind=WEIGHT), plan(PREDICT, kind=WEIGHT, no_runs=True)) == {"runs_q"}
    assert changed(plan(PREDICT), plan(PREDICT, runs_always=True)) == {"runs_q"} and changed(plan(PREDICT, kind=WEIGHT), plan(PREDICT, kind=WEIGHT, runs_always=True)) == set()
    assert changed(plan(FIT_PREDICT), plan(FIT_PREDICT, runs_always=True)) == {"runs_q"}
    assert plan(FIT_PREDICT, runs_always=True, no_runs=True)["runs_q"] == 0


# ---- reachability -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_max", [21 * 1024, 64 * 1024, LDS])
def test_no_series_needs_a_single_sort_kernel(exe, lds_max):
    """The fit once kept a single-sort kernel for F == 1 series without a sort2 width whose keys and 16-bit indices fit the LDS
    (10 * T bytes).  No T = 1 .. 20 480 is such a series, so the kernel is gone and a sorted view needs a width."""
    out = subprocess.run([exe], input=f"sweep {lds_max}\n", capture_output=True, text=True, timeout=120)
    rows = [tuple(map(int, ln.split()[1:])) for ln in out.stdout.splitlines() if ln.startswith("w ")]
    assert [r[0] for r in rows] == list(range(1, 20481))
    for T, K, is_sorted in rows:
        assert K == sort2_width(T, lds_max)
        old_sorted = T <= 65535 and (10 * T <= lds_max or K != 0) and 8 * (T + 1) <= lds_max
        assert not (old_sorted and K == 0), T  # the single-sort branch
        assert is_sorted == int(old_sorted)
