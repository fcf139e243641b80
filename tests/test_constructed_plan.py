"""The constructed-analog launch plans (scikit-downscale_amd/csrc/sd_constructed_plan.h), checked on the host: the header is compiled
with g++ into a small driver (tests/constructed_plan_check.cpp) that prints plans and walks the grids the way the kernels of
sd_constructed.hip decode them.  Every refusal, their order, the limits and the tile geometry."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "constructed_plan_check"
    src = os.path.join(ROOT, "tests", "constructed_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(*words):
        out = subprocess.run([str(path)], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end" and len(lines) == 2, lines
        first = lines[0]
        if first.startswith("error "):
            _, code, msg = first.split(" ", 2)
            return {"error": int(code), "message": msg}
        return {k: int(v) for k, v in (w.split("=") for w in first.split()[1:])}

    return run


@pytest.fixture(scope="module")
def consts(ask):
    return ask("consts")


def select(ask, Tl=14600, Tq=3650, Cc=400, ld_l=None, ld_q=None, k=30, period=366, window=45, wc=("ones",)):
    return ask("select", Tl, Tq, Cc, Cc if ld_l is None else ld_l, Cc if ld_q is None else ld_q, k, period, window, *wc)


def weights(ask, Tl=14600, Tq=3650, Cc=400, ld_l=None, ld_q=None, k=30, kind=0, ridge=1e-6, wc=("ones",)):
    return ask("weights", Tl, Tq, Cc, Cc if ld_l is None else ld_l, Cc if ld_q is None else ld_q, k, kind, repr(float(ridge)), *wc)


def apply(ask, Tl=14600, Cf=100_000, ld_f=None, Tq=3650, q0=0, q1=None, ld_out=None, k=30):
    return ask("apply", Tl, Cf, Cf if ld_f is None else ld_f, Tq, q0, Tq if q1 is None else q1, Cf if ld_out is None else ld_out, k)


def err(p):
    return p["error"], p["message"]


def test_tile_constants(consts):
    c = consts
    assert c["max_k"] == 32 and c["wgt_entries"] == 32 * 33 // 2 + 32 and c["wgt_per_thread"] * c["wgt_block"] >= c["wgt_entries"]
    assert c["sel_block"] % 64 == 0 and c["sel_q"] % (c["sel_block"] // 64) == 0 and c["sel_l"] % 64 == 0
    assert c["sel_lds"] <= 64 * 1024  # at least two workgroups per CU
    assert c["app_block"] == 64 * c["app_waves"] and c["app_rows"] % c["app_waves"] == 0 and c["app_cells"] == 64
    assert c["max_tl"] >= 32_768 and c["max_cc"] >= 4_096  # what the plan must at least take


def test_plans_of_the_benchmark_shape(ask, consts):
    c = consts
    p = select(ask)
    assert p == dict(block=c["sel_block"], lds_bytes=c["sel_lds"], blocks=-(-3650 // c["sel_q"]), q_tiles=-(-3650 // c["sel_q"]),
                     l_tiles=-(-14600 // c["sel_l"]))
    assert weights(ask) == dict(block=c["wgt_block"], blocks=3650)
    a = apply(ask)
    ctiles = -(-100_000 // c["app_cells"])
    assert a == dict(block=c["app_block"], ctiles=ctiles, row_groups=-(-3650 // c["app_rows"]),
                     blocks=-(-ctiles // 8) * 8 * -(-3650 // c["app_rows"]))  # whole rounds of 8 tiles, one per XCD
    assert "error" not in select(ask, Tl=32_768, Cc=4_096, Tq=1)


@pytest.mark.parametrize("Tl", [1, 63, 64, 127, 128, 129, 257])
@pytest.mark.parametrize("Tq", [1, 3, 7, 8, 9, 15, 16, 17, 33])
def test_select_visits_every_target_and_day_once(ask, consts, Tl, Tq):
    assert ask("cover_select", Tl, Tq) == dict(q_min=1, q_max=1, q_outside=0, t_min=1, t_max=1, t_outside=0)
    p = select(ask, Tl=Tl, Tq=Tq, Cc=3, k=1)
    assert (p["q_tiles"], p["l_tiles"]) == (-(-Tq // consts["sel_q"]), -(-Tl // consts["sel_l"]))


@pytest.mark.parametrize("Cf", [1, 63, 64, 65, 130, 8 * 64, 8 * 64 + 1, 17 * 64])
@pytest.mark.parametrize("rows", [(9, 0, 9), (40, 0, 40), (40, 7, 8), (70, 5, 70), (33, 0, 33)])
def test_apply_writes_every_row_and_cell_once(ask, Cf, rows):
    Tq, q0, q1 = rows
    got = ask("cover_apply", Cf, Tq, q0, q1)
    assert got == dict(min=1, max=1, outside=0, tiles_in_first=1)  # (the row groups of one cell tile come first)


def test_coarse_refusals_and_their_order(ask):
    for call, who in ((select, "sd_ca_select"), (weights, "sd_ca_weights")):
        assert err(call(ask, Tl=0)) == (INVALID, f"{who}: bad sizes (Tl=0, Tq=3650, Cc=400)")
        assert err(call(ask, Tq=-1))[1].startswith(f"{who}: bad sizes") and err(call(ask, Cc=0))[0] == INVALID
        assert err(call(ask, k=0)) == (INVALID, f"{who}: k = 0 lies outside [1, 32]")
        assert err(call(ask, k=33)) == (INVALID, f"{who}: k = 33 lies outside [1, 32]")
        assert "error" not in call(ask, k=1) and "error" not in call(ask, k=32)
        assert err(call(ask, ld_l=399)) == (INVALID, f"{who}: ld_l = 399 is less than the 400 columns of a row")
        assert err(call(ask, ld_q=399)) == (INVALID, f"{who}: ld_q = 399 is less than the 400 columns of a row")
        assert "error" not in call(ask, ld_l=401, ld_q=777)
        assert err(call(ask, wc=("set", 7, "-1"))) == (INVALID, f"{who}: wc[7] = -1, expected a finite weight >= 0")
        assert err(call(ask, wc=("set", 0, "nan")))[1].startswith(f"{who}: wc[0] = nan")
        assert err(call(ask, wc=("set", 399, "inf")))[1].startswith(f"{who}: wc[399] = inf")
        assert "error" not in call(ask, wc=("set", 3, "0"))
        # the limits of the plan
        assert err(call(ask, Tl=(1 << 24) + 1)) == (UNSUPPORTED, f"{who}: Tl = 16777217 library days, at most 16777216 are supported")
        assert "error" not in call(ask, Tl=1 << 24, Tq=1, Cc=1)
        assert err(call(ask, Cc=(1 << 16) + 1)) == (UNSUPPORTED, f"{who}: Cc = 65537 columns, at most 65536 are supported")
        assert "error" not in call(ask, Cc=1 << 16, Tl=1, Tq=1)
        assert err(call(ask, Tq=1 << 62, Cc=4))[1] == f"{who}: field too large"
        # the order: sizes, k, leading dimensions, wc, limits
        assert err(call(ask, Tl=0, k=0, ld_l=1))[1].startswith(f"{who}: bad sizes")
        assert err(call(ask, k=0, ld_l=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: k = 0")
        assert err(call(ask, ld_l=1, ld_q=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: ld_l = 1 ")
        assert err(call(ask, ld_q=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: ld_q = 1 ")
        assert err(call(ask, Tl=(1 << 24) + 1, wc=("set", 0, "-1")))[1].startswith(f"{who}: wc[0]")


def test_select_refusals(ask, consts):
    assert err(select(ask, period=0)) == (INVALID, "sd_ca_select: period = 0 with window = 45, expected a period > 0")
    assert err(select(ask, period=-5, window=0))[0] == INVALID
    assert "error" not in select(ask, period=0, window=-1)  # no window: the period is not read
    assert err(select(ask, period=1 << 31))[1] == "sd_ca_select: period and window must fit 32 bits"
    assert err(select(ask, Tl=(1 << 24) + 1, period=0))[0] == UNSUPPORTED  # (the coarse checks come first)
    most = (1 << 31) - 1
    assert select(ask, Tl=1, Tq=most * consts["sel_q"], Cc=1, k=1)["blocks"] == most
    assert err(select(ask, Tl=1, Tq=most * consts["sel_q"] + 1, Cc=1, k=1)) == (INVALID, "sd_ca_select: grid too large")


def test_weights_refusals(ask):
    assert err(weights(ask, kind=2)) == (INVALID, "sd_ca_weights: unknown kind 2")
    assert err(weights(ask, kind=-1))[0] == INVALID and "error" not in weights(ask, kind=1)
    assert err(weights(ask, ridge=-1e-9)) == (INVALID, "sd_ca_weights: ridge = -1e-09, expected a finite factor >= 0")
    assert err(weights(ask, ridge=float("nan")))[1].startswith("sd_ca_weights: ridge = nan")
    assert err(weights(ask, ridge=float("inf")))[0] == INVALID and "error" not in weights(ask, ridge=0.0)
    assert err(weights(ask, kind=5, ridge=-1.0))[1].startswith("sd_ca_weights: unknown kind")  # the order
    assert err(weights(ask, Tl=1, Tq=1 << 31, Cc=1, k=1)) == (INVALID, "sd_ca_weights: grid too large")
    assert weights(ask, Tl=1, Tq=(1 << 31) - 1, Cc=1, k=1)["blocks"] == (1 << 31) - 1


def test_apply_refusals_and_their_order(ask, consts):
    assert err(apply(ask, Tl=0)) == (INVALID, "sd_ca_apply: bad sizes (Tl=0, Tq=3650, Cf=100000)")
    assert err(apply(ask, Cf=0))[0] == INVALID and err(apply(ask, Tq=0, q1=0))[1].startswith("sd_ca_apply: bad sizes")
    assert err(apply(ask, k=0))[1] == "sd_ca_apply: k = 0 lies outside [1, 32]" and err(apply(ask, k=33))[0] == INVALID
    assert err(apply(ask, q0=5, q1=5)) == (INVALID, "sd_ca_apply: rows [5, 5) lie outside the 3650 targets")
    assert err(apply(ask, q0=-1, q1=3))[0] == INVALID and err(apply(ask, q1=3651))[0] == INVALID
    assert "error" not in apply(ask, q0=3649, q1=3650)
    assert err(apply(ask, ld_f=99_999)) == (INVALID, "sd_ca_apply: ld_f = 99999 is less than the 100000 cells of a row")
    assert err(apply(ask, ld_out=99_999)) == (INVALID, "sd_ca_apply: ld_out = 99999 is less than the 100000 cells of a row")
    assert "error" not in apply(ask, ld_f=100_001, ld_out=100_003)
    assert err(apply(ask, Tl=(1 << 24) + 1))[0] == UNSUPPORTED
    assert err(apply(ask, Tl=1 << 24, Cf=1 << 40))[1] == "sd_ca_apply: field too large"
    # the order: sizes, k, rows, leading dimensions (library, output), limits
    assert err(apply(ask, Tl=0, k=0))[1].startswith("sd_ca_apply: bad sizes")
    assert err(apply(ask, k=0, q0=9, q1=3, ld_f=1))[1].startswith("sd_ca_apply: k = 0")
    assert err(apply(ask, q0=9, q1=3, ld_f=1))[1].startswith("sd_ca_apply: rows")
    assert err(apply(ask, ld_f=1, ld_out=1))[1].startswith("sd_ca_apply: ld_f")
    # workgroups < 2^31
    cells, rows = consts["app_cells"], consts["app_rows"]
    Tq = rows * 1024
    Cf_most = ((1 << 31) - 1) // 1024 // 8 * 8 * cells
    assert apply(ask, Tl=1, Tq=Tq, Cf=Cf_most, k=1)["blocks"] == Cf_most // cells * 1024
    assert err(apply(ask, Tl=1, Tq=Tq, Cf=Cf_most + 1, k=1)) == (INVALID, "sd_ca_apply: grid too large")
