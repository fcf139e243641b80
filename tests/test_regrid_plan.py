"""The regridding launch plan and axis tables (scikit-downscale_amd/csrc/sd_regrid_plan.h), checked on the host: the header is
compiled with g++ into a small driver (tests/regrid_plan_check.cpp) that prints plans, walks the grid of a plan the way regrid_kernel
decodes it, and prints axis tables."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR, NEAREST = 0, 1
INVALID = 1
CHUNK, PER_WAVE, BATCH = 64, 16, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "regrid_plan_check"
    src = os.path.join(ROOT, "tests", "regrid_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def ask(exe):
    def run(line):
        out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        return lines[:-1]

    return run


@pytest.fixture(scope="module")
def plan(ask):
    def run(what="plan", method=LINEAR, T=14600, ny=16, nx=25, Ny=250, Nx=400, ld=None, aligned=True):
        ld = Ny * Nx if ld is None else ld
        first = ask(f"{what} {method} {T} {ny} {nx} {Ny} {Nx} {ld} {int(aligned)}")[0]
        if first.startswith("error "):
            _, code, msg = first.split(" ", 2)
            return {"error": int(code), "message": msg}
        return {k: int(v) for k, v in (w.split("=") for w in first.split()[1:])}

    return run


def test_plan_of_the_benchmark_shape(plan):
    p = plan()
    assert p == dict(cols=2, block=256, xtiles=4, nchunks=229, blocks=4 * 250 * 229, time_chunk=CHUNK, steps_per_wave=PER_WAVE, batch=BATCH)
    assert plan(method=NEAREST) == p


@pytest.mark.parametrize("Nx,ld,aligned,cols,xtiles", [(400, None, True, 2, 4), (400, None, False, 1, 7), (401, None, True, 1, 7),
                                                       (400, 250 * 400 + 1, True, 1, 7), (400, 250 * 400 + 2, True, 2, 4),
                                                       (64, None, True, 1, 1), (66, None, True, 2, 1), (128, None, True, 2, 1),
                                                       (130, None, True, 2, 2), (129, None, True, 1, 3), (1, None, True, 1, 1)])
def test_two_columns_per_lane_need_aligned_pairs_and_a_row_wider_than_a_wave(plan, Nx, ld, aligned, cols, xtiles):
    p = plan(Nx=Nx, ld=ld, aligned=aligned)
    assert (p["cols"], p["xtiles"], p["blocks"]) == (cols, xtiles, xtiles * 250 * 229)


@pytest.mark.parametrize("Ny,Nx", [(1, 1), (5, 64), (37, 53), (16, 129), (3, 130), (2, 258), (3, 65)])
@pytest.mark.parametrize("T", [1, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + PER_WAVE + 1])
def test_the_grid_covers_every_cell_and_time_step_once(plan, Ny, Nx, T):
    c = plan("cover", T=T, ny=3, nx=4, Ny=Ny, Nx=Nx)
    assert c == dict(cells_min=1, cells_max=1, steps_min=1, steps_max=1, outside=0)
    assert plan(T=T, Ny=Ny, Nx=Nx)["nchunks"] == -(-T // CHUNK)


def test_refusals_and_their_messages(plan):
    def err(**kw):
        p = plan(**kw)
        return p["error"], p["message"]

    assert err(method=2) == (INVALID, "sd_regrid: unknown method code 2") and err(method=-1)[1].endswith("code -1")
    for bad in (dict(T=0), dict(ny=0), dict(nx=-1), dict(Ny=0), dict(Nx=0)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_regrid: bad sizes (T="), bad
    assert err(T=0, ny=0) == (INVALID, "sd_regrid: bad sizes (T=0, source 0 x 25, target 250 x 400)")
    assert err(ny=1) == (INVALID, "sd_regrid: a source dimension of length 1 cannot be interpolated (source 1 x 25)")
    assert err(nx=1)[1].endswith("(source 16 x 1)")
    assert err(ld=99_999) == (INVALID, "sd_regrid: ld_out = 99999 is less than the 100000 cells of the target grid")
    assert "error" not in plan(ld=100_000)
    # the order: method, sizes, short source dimension, leading dimension
    assert err(method=5, T=0, ny=1, ld=1)[1].startswith("sd_regrid: unknown method")
    assert err(T=0, ny=1, ld=1)[1].startswith("sd_regrid: bad sizes")
    assert err(ny=1, ld=1)[1].startswith("sd_regrid: a source dimension")


def test_the_limit_of_two_to_the_31(plan):
    big = (INVALID, "sd_regrid: grid too large")

    def err(**kw):
        p = plan(**kw)
        return p.get("error"), p.get("message")

    # workgroups: 4 x 250 x nchunks < 2^31
    most = ((1 << 31) - 1) // 1000
    assert plan(T=most * CHUNK)["blocks"] == most * 1000 and err(T=most * CHUNK + 1) == big
    # a source plane and a target row are indexed with int
    assert "error" not in plan(ny=1 << 15, nx=(1 << 16) - 1) and err(ny=1 << 15, nx=1 << 16) == big
    assert err(Ny=1, Nx=1 << 31, T=1) == big and "error" not in plan(Ny=1, Nx=(1 << 31) - 2, T=1)
    assert err(Ny=1 << 40, Nx=1 << 40, T=1) == big and err(T=1 << 62, Ny=1 << 20) == big


# ---- axis tables ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def axis(ask):
    def run(method, x, xn):
        lines = ask(" ".join(["axis", str(method), str(len(x))] + [repr(float(v)) for v in x] + [str(len(xn))] + [repr(float(v)) for v in xn]))
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return int(code), msg
        rows = [ln.split() for ln in lines[1:]]
        return (np.array([[int(r[0]), int(r[1])] for r in rows]), np.array([float(r[2]) for r in rows]), np.array([float(r[3]) for r in rows]))

    return run


def test_linear_axis_table_is_searchsorted_left_clipped(axis):
    x = np.array([1.0, 2.5, 3.0, 7.0])
    xn = np.array([0.5, 1.0, 1.7, 2.5, 3.0, 6.9, 7.0, 7.5])
    idx, t, r = axis(LINEAR, x, xn)
    hi = np.clip(np.searchsorted(x, xn, side="left"), 1, 3)
    assert np.array_equal(idx, np.stack([hi - 1, hi], axis=1))  # node 0 uses the interval above it, node k >= 1 the one below
    outside = (xn < 1.0) | (xn > 7.0)
    assert np.array_equal(np.isnan(t), outside) and np.array_equal(t[~outside], (xn - x[hi - 1])[~outside])
    assert np.array_equal(r, 1.0 / (x[hi] - x[hi - 1]))
    # descending storage: the same brackets, positions counted in the stored order; any order of the targets
    idx_d, t_d, r_d = axis(LINEAR, x[::-1], xn[::-1])
    assert np.array_equal(idx_d[::-1], 3 - idx) and np.array_equal(t_d[::-1], t, equal_nan=True) and np.array_equal(r_d[::-1], r)


def test_nearest_axis_table_sends_midpoints_down(axis):
    x = np.arange(4.0)
    xn = np.array([-0.25, 0.0, 0.5, 0.75, 1.5, 2.5, 3.0, 3.25])
    idx, t, r = axis(NEAREST, x, xn)
    assert np.array_equal(idx[:, 0], [0, 0, 0, 1, 1, 2, 3, 3]) and np.array_equal(idx[:, 0], idx[:, 1])
    assert np.array_equal(np.isnan(t), [True] + [False] * 6 + [True]) and not t[1:-1].any() and not r.any()
    assert np.array_equal(axis(NEAREST, x[::-1], xn)[0][:, 0], 3 - idx[:, 0])


def test_axis_refusals(axis):
    assert axis(LINEAR, [0.0, 2.0, 1.0], [0.5]) == (INVALID, "sd_regrid: non-monotonic or duplicated source coordinate 'lat'")
    assert axis(LINEAR, [0.0, 1.0, 1.0], [0.5])[1].startswith("sd_regrid: non-monotonic or duplicated")
    assert axis(NEAREST, [2.0, 2.0], [0.5])[0] == INVALID
    assert axis(LINEAR, [0.0, float("nan"), 1.0], [0.5]) == (INVALID, "sd_regrid: NaN in the source coordinate 'lat'")
    assert axis(LINEAR, [0.0, 1.0], [float("nan")]) == (INVALID, "sd_regrid: NaN in the target coordinate 'lat'")
