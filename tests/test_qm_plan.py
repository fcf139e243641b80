"""The quantile-mapping launch plan (scikit-downscale_amd/csrc/sd_qm_plan.h), checked on the host: which kernels a
QuantileMappingReressor / EquidistantCdfMatcher / CunnaneTransformer call launches, with which widths, grids and LDS sizes, and which
calls it refuses.  The header is compiled with g++ into a small driver (tests/qm_plan_check.cpp) that reads calls on stdin and prints
their plans.  The expectations restate the conditions the entry points and launchers of csrc/sd_qm.hip carried inline before the plan
existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024  # MI355X
CU = 256
FIT, PREDICT, CUNNANE = 0, 1, 2
QMR, ECM_DIFF, ECM_RATIO = 0, 1, 2
EX_NONE, EX_MIN, EX_MAX, EX_BOTH, EX_1TO1 = 0, 1, 2, 3, 4
FORWARD, INVERSE = 0, 1
INVALID, UNSUPPORTED = 1, 3
SWITCHES = ("no_tile", "divide", "trace")


# ---- the conditions as sd_qm.hip wrote them ---------------------------------------------------------------------------------
def block_lds(np_):
    return 8 * (np_ + 1) + 4 * 1025


def sort_width(T, lds_max=LDS):
    for K in (1, 3, 5, 9, 13, 15, 17, 19):
        if T <= 1024 * K and block_lds((T + K - 1) // K * K) <= lds_max:
            return K
    return 0


def tile_width(T, lds_max=LDS):
    for K in (13, 15, 17):
        chunk = 64 * K
        nchunks = (T + chunk - 1) // chunk
        if nchunks <= 16 and block_lds(nchunks * chunk) <= lds_max:
            return K
    return 0


def tile_lds(K):
    chunk = 64 * K
    rs = chunk + 2 + ((4 - (chunk + 2) % 4) + 2) % 4
    return 8 * (8 * rs + 88)


def tiled(C, rows):
    return 8 * (((C + 7) // 8 + 7) // 8) * rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "qm_plan_check"
    src = os.path.join(ROOT, "tests", "qm_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(op, T=14600, Tp=14600, C=8192, ld=None, ld_out=None, has_y=True, model=QMR, ex=EX_NONE, ne=10, direction=FORWARD, lds_max=LDS,
            cu=CU, **kw):
        ld, ld_out = (C if v is None else v for v in (ld, ld_out))
        assert set(kw) <= set(SWITCHES), kw
        words = [op, T, Tp, C, ld, ld_out, int(has_y), model, ex, ne, direction, lds_max, cu] + [int(kw.get(s, False)) for s in SWITCHES]
        out = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return {"error": int(code), "message": msg}
        p = {k: int(v) for k, v in (w.split("=") for w in lines[0].split()[1:])}
        # geometry of the launches the call makes, in their order: (grid x, grid y), block, LDS bytes
        p["g"] = {f[0]: ((int(f[1]), int(f[2])), int(f[3]), int(f[4])) for f in (ln.split() for ln in lines[1:-1])}
        p["order"] = [ln.split()[0] for ln in lines[1:-1]]
        return p

    return run


@pytest.fixture(scope="module")
def sweep(exe):
    def run(lds_max):
        out = subprocess.run([exe], input=f"sweep {lds_max}\n", capture_output=True, text=True, timeout=120)
        rows = [tuple(map(int, ln.split()[1:])) for ln in out.stdout.splitlines() if ln.startswith("w ")]
        assert [r[0] for r in rows] == list(range(2, 19601))
        return rows

    return run


# ---- the decision table of the fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_max", [LDS, 64 * 1024])
def test_fit_widths_of_every_length(sweep, lds_max):
    for T, err, K, Kt, nchunks, np_ in sweep(lds_max):
        k, kt = sort_width(T, lds_max), tile_width(T, lds_max)
        if k == 0:
            assert err == UNSUPPORTED, T
            continue
        assert (err, K, Kt) == (0, k, kt), T
        assert (nchunks, np_) == ((-(-T // (64 * kt)), -(-T // (64 * kt)) * 64 * kt) if kt else (0, 0)), T


@pytest.mark.parametrize("T,K,Kt", [(2, 1, 13), (1024, 1, 13), (1025, 3, 13), (3072, 3, 13), (3073, 5, 13), (5120, 5, 13), (5121, 9, 13),
                                    (9216, 9, 13), (9217, 13, 13), (13312, 13, 13), (13313, 15, 15), (15360, 15, 15), (15361, 17, 17),
                                    (17408, 17, 17), (17409, 19, 0), (19456, 19, 0)])
def test_fit_width_ladder_at_160_kb(plan, T, K, Kt):
    p = plan(FIT, T=T)
    assert (p["K"], p["Kt"], p["tiled"]) == (K, Kt, int(Kt != 0))
    assert p["order"] == (["tile_runs", "merge_runs"] if Kt else ["transpose", "sort"])


def test_series_beyond_the_workgroup_sort_are_unsupported(plan, sweep):
    p = plan(FIT, T=19457)
    assert (p["error"], p["message"]) == (UNSUPPORTED, "sd_qm_fit: series of 19457 samples exceed the workgroup sort (19456)")
    # a 64 KB LDS: the longest sortable series has 7 677 samples, the longest tiled one 7 616 (the message keeps its literal)
    rows = sweep(64 * 1024)
    assert max(T for T, err, *_ in rows if err == 0) == 7677 and max(T for T, err, K, Kt, *_ in rows if err == 0 and Kt != 0) == 7616
    assert all(err == 0 for T, err, *_ in rows if T <= 7677)
    p = plan(FIT, T=7678, lds_max=64 * 1024)
    assert (p["error"], p["message"]) == (UNSUPPORTED, "sd_qm_fit: series of 7678 samples exceed the workgroup sort (19456)")
    assert (plan(FIT, T=7616, lds_max=64 * 1024)["Kt"], plan(FIT, T=7617, lds_max=64 * 1024)["Kt"]) == (17, 0)


def test_fit_of_the_40_year_daily_series(plan):
    p = plan(FIT)  # the shape of tools/bench_extra.py --workload qmr / ecm: 8 192 cells x 14 600 steps
    assert (p["K"], p["tiled"], p["Kt"], p["nchunks"], p["np"], p["runs_bytes"]) == (15, 1, 15, 16, 15360, 8 * 15360 * 8192)
    assert p["g"]["tile_runs"] == ((tiled(8192, 16), 1), 512, tile_lds(15)) and tiled(8192, 16) == 16384 and tile_lds(15) == 8 * (8 * 962 + 88)
    assert p["g"]["merge_runs"] == ((1024, 1), 1024, 8 * 15361 + 4100)
    assert plan(FIT, has_y=False) == p  # y only repeats the launches


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_predict_of_the_bench_shapes(plan):
    p = plan(PREDICT)
    assert (p["rank_K"], p["tails"], p["map_per"], p["lds"], p["nb"]) == (0, 0, 16, 8 * 14600, 256)
    assert p["order"] == ["transpose", "ppcheck_fit", "ppcheck_new", "map", "untranspose", "status_public"]
    g = p["g"]
    assert g["transpose"] == g["untranspose"] == ((256, 457), 256, 0)
    assert g["ppcheck_fit"] == g["ppcheck_new"] == ((58, 1), 256, 0)
    assert g["map"] == ((256, 1), 1024, 8 * 14600) and g["status_public"] == ((32, 1), 256, 0)
    e = plan(PREDICT, model=ECM_DIFF)
    assert (e["rank_K"], e["tails"], e["map_per"], e["lds"], e["nb"]) == (15, 0, 8, 8 * 14600, 256)
    assert e["order"] == ["transpose", "rank", "ppcheck_fit", "ppcheck_new", "map", "untranspose", "status_public"]
    assert e["g"]["rank"] == ((1024, 1), 1024, 8 * (14610 + 1) + 4100)
    assert plan(PREDICT, model=ECM_RATIO) == e


@pytest.mark.parametrize("C,blocks", [(1, 8), (7, 8), (8, 8), (9, 8), (64, 8), (65, 16)])
def test_partial_tiles(plan, C, blocks):
    p = plan(FIT, T=3000, C=C)  # 4 chunks of 832
    assert (p["Kt"], p["nchunks"], p["np"], p["runs_bytes"]) == (13, 4, 3328, 8 * 3328 * C)
    assert p["g"]["tile_runs"] == ((blocks * 4, 1), 512, tile_lds(13)) and blocks * 4 == tiled(C, 4)
    assert p["g"]["merge_runs"] == ((C, 1), 1024, block_lds(3328))
    q = plan(PREDICT, T=3000, Tp=100, C=C, model=ECM_DIFF, ex=EX_BOTH)
    g = q["g"]
    assert g["transpose"] == g["untranspose"] == (((C + 31) // 32, 4), 256, 0)
    assert g["rank"] == ((C, 1), 1024, block_lds(100)) and g["map"] == ((C, 1), 1024, 8 * 3000)
    assert g["tails"] == g["status_public"] == ((1, 1), 256, 0)


def test_sort_rank_and_merge_grids_stop_at_four_workgroups_per_cu(plan):
    for C, nb in ((1023, 1023), (1024, 1024), (1025, 1024), (100_000, 1024)):
        assert plan(FIT, C=C)["g"]["merge_runs"][0] == (nb, 1)
        assert plan(FIT, C=C, no_tile=True)["g"]["sort"] == ((nb, 1), 1024, block_lds(14610))
        assert plan(PREDICT, C=C, model=ECM_DIFF)["g"]["rank"][0] == (nb, 1)
    assert plan(FIT, C=100, cu=4)["g"]["merge_runs"][0] == (16, 1) and plan(FIT, C=100, cu=4, no_tile=True)["g"]["sort"][0] == (16, 1)
    assert plan(FIT, C=257)["g"]["tile_runs"][0] == (tiled(257, 16), 1) and tiled(257, 16) == 8 * 5 * 16


def test_map_grid_is_one_workgroup_per_cu_above_half_the_lds(plan):
    a, b = plan(PREDICT, T=10240), plan(PREDICT, T=10241)
    assert (a["lds"], a["nb"], a["g"]["map"]) == (81920, 512, ((512, 1), 1024, 81920))
    assert (b["lds"], b["nb"], b["g"]["map"]) == (81928, 256, ((256, 1), 1024, 81928))
    assert plan(PREDICT, T=10240, C=300)["nb"] == 300 and plan(PREDICT, T=10241, C=300)["nb"] == 256 and plan(PREDICT, T=10241, C=7)["nb"] == 7
    assert plan(PREDICT, T=10240, cu=4, model=ECM_DIFF)["nb"] == 8


def test_cunnane_forward_keeps_the_fit_in_lds_and_inverse_does_not(plan):
    f, i = plan(CUNNANE, direction=FORWARD, ex=EX_BOTH), plan(CUNNANE, direction=INVERSE, ex=EX_BOTH)
    assert (f["lds"], f["nb"], f["g"]["cunnane"]) == (8 * 14600, 256, ((256, 1), 1024, 8 * 14600))
    assert (i["lds"], i["nb"], i["g"]["cunnane"]) == (8, 512, ((512, 1), 1024, 8))
    assert f["order"] == i["order"] == ["transpose", "cunnane", "untranspose", "status_public"]
    assert f["g"]["transpose"] == ((256, 457), 256, 0)
    assert plan(CUNNANE, T=10240)["nb"] == 512 and plan(CUNNANE, T=10241)["nb"] == 256
    # (a state cannot hold more than 19 456 samples; the limit is kept as written)
    assert plan(CUNNANE, T=20480)["lds"] == LDS and plan(CUNNANE, T=20481, direction=INVERSE)["lds"] == 8
    p = plan(CUNNANE, T=20481)
    assert (p["error"], p["message"]) == (INVALID, "sd_qm_cunnane: fitted series too long for the LDS-resident search")
    assert "error" not in plan(CUNNANE, has_y=False)  # the transformer is fitted without y


# ---- predict ----------------------------------------------------------------------------------------------------------------
def test_only_the_rank_sort_limits_the_new_series(plan):
    for Tp in (19456, 19457, 100_000):
        p = plan(PREDICT, Tp=Tp, C=16)
        assert (p["rank_K"], p["map_per"]) == (0, 16) and "rank" not in p["g"]
    for model in (ECM_DIFF, ECM_RATIO):
        assert plan(PREDICT, Tp=19456, C=16, model=model)["rank_K"] == 19
        p = plan(PREDICT, Tp=19457, C=16, model=model)
        assert (p["error"], p["message"]) == (UNSUPPORTED, "sd_qm_predict: series of 19457 samples exceed the workgroup sort (19456)")
    assert [plan(PREDICT, Tp=Tp, C=16, model=ECM_DIFF)["rank_K"] for Tp in (1, 1024, 1025, 5000, 9000, 17409)] == [1, 1, 3, 5, 9, 19]


@pytest.mark.parametrize("model", [QMR, ECM_DIFF, ECM_RATIO])
def test_tails_kernel_runs_for_the_synthetic_end_points_only(plan, model):
    for ex, tails in ((EX_NONE, 0), (EX_MIN, 1), (EX_MAX, 1), (EX_BOTH, 1), (EX_1TO1, 0)):
        p = plan(PREDICT, model=model, ex=ex)
        assert p["tails"] == tails and ("tails" in p["g"]) == bool(tails)
        if tails:
            assert p["g"]["tails"] == ((32, 1), 256, 0) and p["order"].index("tails") == p["order"].index("map") - 1


# ---- errors: code, text and order of the entry points -----------------------------------------------------------------------
def test_errors_come_in_the_order_of_the_entry_points(plan):
    def err(*a, **kw):
        p = plan(*a, **kw)
        return p["error"], p["message"]

    # fit: sizes, then the sort, then the grid of the tile stage
    bad = dict(T=1, C=10, ld=9)
    assert err(FIT, **bad) == err(FIT, T=19457, C=0) == err(FIT, T=19457, C=10, ld=9) == (INVALID, "sd_qm_fit: bad sizes")
    assert err(FIT, T=19457, C=1 << 31)[0] == UNSUPPORTED
    cmax = 64 * ((1 << 24) - 1)  # 16 chunks: 8 * tx * 16 < 2^31
    assert "error" not in plan(FIT, C=cmax) and plan(FIT, C=cmax)["g"]["tile_runs"][0] == ((1 << 31) - 128, 1)
    assert err(FIT, C=cmax + 1) == (INVALID, "sd_qm_fit: grid too large")
    assert "error" not in plan(FIT, C=cmax + 1, no_tile=True) and "error" not in plan(FIT, T=17409, C=cmax + 1)
    # predict: a call that violates every condition, mended one condition at a time
    kw = dict(ex=7, ne=1, model=5, has_y=False, Tp=0, T=20481)
    assert err(PREDICT, **kw) == (INVALID, "sd_qm_predict: unknown extrapolate code 7")
    assert err(PREDICT, **dict(kw, ex=-1))[1] == "sd_qm_predict: unknown extrapolate code -1" and err(PREDICT, **dict(kw, ex=5))[1].endswith("code 5")
    kw["ex"] = EX_1TO1
    assert err(PREDICT, **kw) == (INVALID, "Invalid number of n_endpoints, must be >= 2")
    kw["ne"] = 2
    assert err(PREDICT, **kw) == (INVALID, "sd_qm_predict: unknown model 5") and err(PREDICT, **dict(kw, model=-1))[1].endswith("model -1")
    kw["model"] = ECM_RATIO
    assert err(PREDICT, **kw) == (INVALID, "sd_qm_predict: the state was fitted without y")
    kw["has_y"] = True
    assert err(PREDICT, **kw) == err(PREDICT, **dict(kw, Tp=5, ld=8191)) == err(PREDICT, **dict(kw, Tp=5, ld_out=8191)) == (
        INVALID, "sd_qm_predict: bad sizes")
    kw["Tp"] = 19457
    assert err(PREDICT, **kw) == (UNSUPPORTED, "sd_qm_predict: series of 19457 samples exceed the workgroup sort (19456)")
    kw["Tp"] = 1 << 31
    kw["model"] = QMR
    assert err(PREDICT, **kw) == (INVALID, "sd_qm_predict: fitted series too long for the LDS-resident search")
    kw["T"] = 20480
    assert err(PREDICT, **kw) == (INVALID, "sd_qm_predict: series too long")
    kw["Tp"] = (1 << 31) - 1
    assert "error" not in plan(PREDICT, **kw)
    # Cunnane
    kw = dict(direction=2, ex=EX_1TO1, ne=0, Tp=0, T=20481)
    assert err(CUNNANE, **kw) == (INVALID, "sd_qm_cunnane: unknown direction 2")
    kw["direction"] = FORWARD
    assert err(CUNNANE, **kw) == (INVALID, "sd_qm_cunnane: unknown extrapolate code 4")
    kw["ex"] = EX_MIN
    assert err(CUNNANE, **kw) == (INVALID, "sd_qm_cunnane: n_endpoints must be positive")
    kw["ne"] = 1
    assert err(CUNNANE, **kw) == err(CUNNANE, **dict(kw, Tp=3, ld=1)) == err(CUNNANE, **dict(kw, Tp=3, ld_out=1)) == (INVALID, "sd_qm_cunnane: bad sizes")
    kw["Tp"] = 1 << 40
    assert err(CUNNANE, **kw) == (INVALID, "sd_qm_cunnane: fitted series too long for the LDS-resident search")
    assert "error" not in plan(CUNNANE, **dict(kw, T=20480))


# ---- development switches -----------------------------------------------------------------------------------------------------
def test_each_switch_changes_what_it_names_and_nothing_else(plan):
    def changed(a, b):
        return {k for k in a if a[k] != b[k]}

    for T in (3000, 14600, 17408):
        a, b = plan(FIT, T=T), plan(FIT, T=T, no_tile=True)
        assert changed(a, b) == {"tiled", "Kt", "nchunks", "np", "runs_bytes", "g", "order"}
        assert (b["tiled"], b["Kt"], b["runs_bytes"]) == (0, 0, 0) and b["order"] == ["transpose", "sort"]
        assert b["g"]["transpose"] == ((256, (T + 31) // 32), 256, 0) and b["g"]["sort"] == ((1024, 1), 1024, block_lds(-(-T // a["K"]) * a["K"]))
    assert changed(plan(FIT, T=17409), plan(FIT, T=17409, no_tile=True)) == set()
    for op in (FIT, PREDICT, CUNNANE):
        base = plan(op, model=ECM_DIFF, ex=EX_BOTH)
        assert (base["divide"], base["trace"]) == (0, 0)
        assert changed(base, plan(op, model=ECM_DIFF, ex=EX_BOTH, divide=True)) == {"divide"}
        assert changed(base, plan(op, model=ECM_DIFF, ex=EX_BOTH, trace=True)) == {"trace"}
    assert changed(plan(PREDICT), plan(PREDICT, no_tile=True)) == set()
