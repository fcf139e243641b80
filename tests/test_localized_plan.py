"""The localized-analog launch plans (scikit-downscale_amd/csrc/sd_localized_plan.h), checked on the host: the header is compiled with
g++ into a small driver (tests/localized_plan_check.cpp) that prints plans and walks the grids the way the kernels of sd_localized.hip
decode them.  Every refusal, their order, the limits and the tile geometry."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 3
NONE, SHIFT, SCALE = 0, 1, 2


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "localized_plan_check"
    src = os.path.join(ROOT, "tests", "localized_plan_check.cpp")
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


def local(ask, Tl=14600, Tq=3650, ny=20, nx=20, ld_l=None, ld_q=None, k=30, ry=2, rx=2, wc=("ones",)):
    return ask("local", Tl, Tq, ny, nx, ny * nx if ld_l is None else ld_l, ny * nx if ld_q is None else ld_q, k, ry, rx, *wc)


def apply(ask, Tl=14600, Cf=100_000, ld_f=None, Cc=400, ld_l=None, ld_q=None, Tq=3650, q0=0, q1=None, ld_out=None, adjust=SHIFT, max_scale=0.0,
          has_coarse=1):
    return ask("apply", Tl, Cf, Cf if ld_f is None else ld_f, Cc, Cc if ld_l is None else ld_l, Cc if ld_q is None else ld_q, Tq, q0,
               Tq if q1 is None else q1, Cf if ld_out is None else ld_out, adjust, repr(float(max_scale)), has_coarse)


def err(p):
    return p["error"], p["message"]


def test_tile_constants(consts):
    c = consts
    assert c["loc_block"] % 64 == 0 and c["loc_block"] <= 1024 and c["loc_max_cells"] == c["loc_block"] * c["loc_per_thread"]
    assert c["loc_max_cells"] >= 4096 and c["loc_max_cells"] == c["header_max_cells"]  # what the plan must at least take; the header's name
    assert c["loc_lds_max"] == 16 * c["loc_max_cells"] <= 64 * 1024  # Q[q] and one row of terms: what a workgroup may ask for
    assert c["lap_block"] == 64 * c["lap_waves"] == c["lap_cells"] and c["lap_rows"] % c["lap_batch"] == 0
    assert c["max_k"] == 32 and c["max_tl"] == 1 << 24


def test_plans_of_the_benchmark_shape(ask, consts):
    c = consts
    assert local(ask) == dict(block=c["loc_block"], lds_bytes=16 * 400, blocks=3650, ry=2, rx=2)
    ctiles, groups = -(-100_000 // c["lap_cells"]), -(-3650 // c["lap_rows"])
    assert apply(ask) == dict(block=c["lap_block"], ctiles=ctiles, row_groups=groups, blocks=ctiles * groups)
    assert local(ask, ny=64, nx=64, Tq=1) == dict(block=c["loc_block"], lds_bytes=65536, blocks=1, ry=2, rx=2)  # 4 096 cells
    assert local(ask, ny=3, nx=4, ry=5, rx=1 << 40)["ry"] == 2 and local(ask, ny=3, nx=4, ry=5, rx=1 << 40)["rx"] == 3  # cut to the grid


def grids_around(c):
    one, whole = c["loc_block"], c["loc_max_cells"]
    return [(3, 4), (9, 17), (1, 7), (7, 1), (1, one - 1), (1, one), (one + 1, 1), (one // 16, 17), (whole - 1, 1), (64, whole // 64), (1, whole)]


def test_local_owns_every_cell_once_and_adds_in_the_order_of_the_rule(ask, consts):
    for ny, nx in grids_around(consts):
        for ry, rx in ((0, 0), (1, 1), (1, 2), (2, 0), (5, 5), (ny, nx)):
            got = ask("cover_local", ny, nx, ry, rx)
            rows, cols = min(ny, 2 * ry + 1), min(nx, 2 * rx + 1)
            assert got == dict(min=1, max=1, outside=0, terms_min=min(ny, ry + 1) * min(nx, rx + 1), terms_max=rows * cols, bad_order=0), (ny, nx, ry, rx)
    assert err(ask("cover_local", 1, consts["loc_max_cells"] + 1, 0, 0))[0] == UNSUPPORTED


def test_apply_writes_every_row_and_cell_once(ask, consts):
    cells, rows, batch = consts["lap_cells"], consts["lap_rows"], consts["lap_batch"]
    for Cf in (1, 63, 130, cells - 1, cells, cells + 1, 3 * cells + 5):
        for Tq, q0, q1 in ((9, 0, 9), (rows - 1, 0, rows - 1), (rows, 0, rows), (rows + 1, 0, rows + 1), (40, 7, 8), (70, 5, 70),
                           (2 * rows + batch + 1, 0, 2 * rows + batch + 1), (batch + 1, 1, batch + 1)):
            assert ask("cover_apply", Cf, Tq, q0, q1) == dict(min=1, max=1, outside=0, reads_outside=0), (Cf, Tq, q0, q1)


def test_local_refusals_and_their_order(ask, consts):
    who, most = "sd_ca_local", consts["loc_max_cells"]
    assert err(local(ask, Tl=0)) == (INVALID, f"{who}: bad sizes (Tl=0, Tq=3650, ny=20, nx=20)")
    assert err(local(ask, Tq=-1))[1].startswith(f"{who}: bad sizes") and err(local(ask, ny=0))[0] == INVALID and err(local(ask, nx=0, ld_l=1))[0] == INVALID
    assert err(local(ask, k=0)) == (INVALID, f"{who}: k = 0 lies outside [1, 32]")
    assert err(local(ask, k=33)) == (INVALID, f"{who}: k = 33 lies outside [1, 32]")
    assert "error" not in local(ask, k=1) and "error" not in local(ask, k=32)
    assert err(local(ask, ry=-1)) == (INVALID, f"{who}: radii (-1, 2), expected two numbers of coarse cells >= 0")
    assert err(local(ask, rx=-3))[0] == INVALID and "error" not in local(ask, ry=0, rx=0)
    assert err(local(ask, ld_l=399)) == (INVALID, f"{who}: ld_l = 399 is less than the 400 columns of a row")
    assert err(local(ask, ld_q=399)) == (INVALID, f"{who}: ld_q = 399 is less than the 400 columns of a row")
    assert "error" not in local(ask, ld_l=401, ld_q=777)
    assert err(local(ask, wc=("set", 7, "-1"))) == (INVALID, f"{who}: wc[7] = -1, expected a finite weight >= 0")
    assert err(local(ask, wc=("set", 0, "nan")))[1].startswith(f"{who}: wc[0] = nan")
    assert err(local(ask, wc=("set", 399, "inf")))[1].startswith(f"{who}: wc[399] = inf")
    assert "error" not in local(ask, wc=("set", 3, "0"))
    # the limits of the plan
    assert err(local(ask, Tl=(1 << 24) + 1)) == (UNSUPPORTED, f"{who}: Tl = 16777217 library days, at most 16777216 are supported")
    assert "error" not in local(ask, Tl=1 << 24, Tq=1, ny=1, nx=1)
    assert err(local(ask, ny=1, nx=most + 1)) == (UNSUPPORTED, f"{who}: a coarse grid of 1 x {most + 1} cells, at most {most} cells are supported")
    assert err(local(ask, ny=65, nx=64))[0] == UNSUPPORTED and "error" not in local(ask, ny=64, nx=64) and "error" not in local(ask, ny=most, nx=1)
    assert err(local(ask, ny=1 << 40, nx=1 << 40, ld_l=1, ld_q=1))[0] == UNSUPPORTED  # (ny * nx is never formed)
    assert err(local(ask, Tq=1 << 62, ny=2, nx=2))[1] == f"{who}: field too large"
    assert err(local(ask, Tl=1, Tq=1 << 31, ny=1, nx=1, k=1)) == (INVALID, f"{who}: grid too large")
    assert local(ask, Tl=1, Tq=(1 << 31) - 1, ny=1, nx=1, k=1)["blocks"] == (1 << 31) - 1
    # the order: sizes, k, radii, leading dimensions, wc, limits
    assert err(local(ask, Tl=0, k=0, ry=-1))[1].startswith(f"{who}: bad sizes")
    assert err(local(ask, k=0, ry=-1, ld_l=1))[1].startswith(f"{who}: k = 0")
    assert err(local(ask, ry=-1, ld_l=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: radii")
    assert err(local(ask, ld_l=1, ld_q=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: ld_l = 1 ")
    assert err(local(ask, ld_q=1, wc=("set", 0, "-1")))[1].startswith(f"{who}: ld_q = 1 ")
    assert err(local(ask, Tl=(1 << 24) + 1, wc=("set", 0, "-1")))[1].startswith(f"{who}: wc[0]")
    assert err(local(ask, Tl=(1 << 24) + 1, ny=1, nx=most + 1))[1].startswith(f"{who}: Tl = ")


def test_apply_refusals_and_their_order(ask, consts):
    who = "sd_ca_local_apply"
    assert err(apply(ask, Tl=0)) == (INVALID, f"{who}: bad sizes (Tl=0, Tq=3650, Cf=100000, Cc=400)")
    assert err(apply(ask, Cf=0))[0] == INVALID and err(apply(ask, Cc=0))[0] == INVALID and err(apply(ask, Tq=0, q1=0))[1].startswith(f"{who}: bad sizes")
    assert err(apply(ask, adjust=3)) == (INVALID, f"{who}: unknown adjust 3") and err(apply(ask, adjust=-1))[0] == INVALID
    for adjust in (NONE, SHIFT, SCALE):
        assert "error" not in apply(ask, adjust=adjust)
    assert err(apply(ask, adjust=SHIFT, has_coarse=0)) == (INVALID, f"{who}: adjust 1 needs L_dev and Q_dev")
    assert err(apply(ask, adjust=SCALE, has_coarse=0))[0] == INVALID and "error" not in apply(ask, adjust=NONE, has_coarse=0)
    assert err(apply(ask, max_scale=-1.0)) == (INVALID, f"{who}: max_scale = -1, expected 0 (no limit) or a limit > 0")
    assert err(apply(ask, max_scale=float("nan")))[1].startswith(f"{who}: max_scale = nan")
    assert "error" not in apply(ask, max_scale=0.0) and "error" not in apply(ask, max_scale=2.5) and "error" not in apply(ask, max_scale=float("inf"))
    assert err(apply(ask, q0=5, q1=5)) == (INVALID, f"{who}: rows [5, 5) lie outside the 3650 targets")
    assert err(apply(ask, q0=-1, q1=3))[0] == INVALID and err(apply(ask, q1=3651))[0] == INVALID
    assert "error" not in apply(ask, q0=3649, q1=3650)
    assert err(apply(ask, ld_f=99_999)) == (INVALID, f"{who}: ld_f = 99999 is less than the 100000 cells of a row")
    assert err(apply(ask, ld_out=99_999)) == (INVALID, f"{who}: ld_out = 99999 is less than the 100000 cells of a row")
    assert err(apply(ask, ld_l=399)) == (INVALID, f"{who}: ld_l = 399 is less than the 400 columns of a row")
    assert err(apply(ask, ld_q=399)) == (INVALID, f"{who}: ld_q = 399 is less than the 400 columns of a row")
    assert "error" not in apply(ask, adjust=NONE, ld_l=0, ld_q=0, has_coarse=0)  # (not read)
    assert "error" not in apply(ask, ld_f=100_001, ld_out=100_003, ld_l=401, ld_q=402)
    assert err(apply(ask, Tl=(1 << 24) + 1)) == (UNSUPPORTED, f"{who}: Tl = 16777217 library days, at most 16777216 are supported")
    most = consts["loc_max_cells"]
    assert err(apply(ask, Cc=most + 1)) == (UNSUPPORTED, f"{who}: Cc = {most + 1} coarse cells, at most {most} are supported")
    assert "error" not in apply(ask, Cc=most)
    assert err(apply(ask, Tl=1 << 24, Cf=1 << 40))[1] == f"{who}: field too large"
    # the order: sizes, adjust, the coarse fields, max_scale, rows, leading dimensions (library, output, coarse), limits
    assert err(apply(ask, Tl=0, adjust=7))[1].startswith(f"{who}: bad sizes")
    assert err(apply(ask, adjust=7, has_coarse=0, max_scale=-1.0))[1].startswith(f"{who}: unknown adjust")
    assert err(apply(ask, has_coarse=0, max_scale=-1.0))[1].startswith(f"{who}: adjust 1 needs")
    assert err(apply(ask, max_scale=-1.0, q0=9, q1=3))[1].startswith(f"{who}: max_scale")
    assert err(apply(ask, q0=9, q1=3, ld_f=1))[1].startswith(f"{who}: rows")
    assert err(apply(ask, ld_f=1, ld_out=1, ld_l=1))[1].startswith(f"{who}: ld_f")
    assert err(apply(ask, ld_out=1, ld_l=1))[1].startswith(f"{who}: ld_out")
    assert err(apply(ask, ld_l=1, ld_q=1, Tl=(1 << 24) + 1))[1].startswith(f"{who}: ld_l")
    # workgroups < 2^31
    cells, rows = consts["lap_cells"], consts["lap_rows"]
    Tq = rows * 1024
    Cf_most = ((1 << 31) - 1) // 1024 * cells
    assert apply(ask, Tl=1, Tq=Tq, Cf=Cf_most, Cc=1, adjust=NONE)["blocks"] == Cf_most // cells * 1024
    assert err(apply(ask, Tl=1, Tq=Tq, Cf=Cf_most + 1, Cc=1, adjust=NONE)) == (INVALID, f"{who}: grid too large")
