"""The conservative-remapping launch plan and axis tables (scikit-downscale_amd/csrc/sd_remap_plan.h), checked on the host: the header
is compiled with g++ into a small driver (tests/remap_plan_check.cpp) that prints axis tables and plans and walks the grid of a plan
the way remap_kernel decodes it.  The axis tables must equal the NumPy restatement (tests/_remap_oracle.py, brute force over all
pairs of cells) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _remap_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
CHUNK, PER_WAVE, BATCH, LANES = 64, 16, 4, 64


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "remap_plan_check"
    src = os.path.join(ROOT, "tests", "remap_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(line):
        out = subprocess.run([str(path)], input=line + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        return lines[:-1]

    return run


def words(b):
    return [str(len(b) - 1)] + ([repr(float(v)) for v in b] if len(b) > 1 else [])  # (no cell: the driver reads no bound)


# ---- axis tables ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def axis(ask):
    def run(sb, db):
        lines = ask(" ".join(["axis"] + words(sb) + words(db)))
        if lines[0].startswith("error "):
            _, code, msg = lines[0].split(" ", 2)
            return int(code), msg
        rows = [ln.split() for ln in lines[1:]]
        return dict(entries=int(lines[0].split("=")[1]), first=np.array([int(r[0]) for r in rows]), count=np.array([int(r[1]) for r in rows]),
                    full=np.array([float(r[2]) for r in rows]), w=[np.array([float(x) for x in r[3:]]) for r in rows])

    return run


def equals_oracle(got, sb, db):
    first, count, w, full = mo.axis_table(sb, db)
    assert np.array_equal(got["first"], first) and np.array_equal(got["count"], count)
    assert got["full"].tobytes() == full.tobytes()  # bit for bit
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["w"], w))
    assert got["entries"] == count.sum() <= (len(sb) - 1) + (len(db) - 1) - 1 or count.sum() == 0
    return first, count, w, full


AXES = {
    "integer_factor": (np.arange(13) / 4.0, np.arange(4.0)),
    "straddling": (np.linspace(0.0, 10.0, 38), np.array([0.0, 0.9, 3.3, 3.35, 7.77, 10.0])),
    "random": (np.sort(np.random.default_rng(0).uniform(-3, 3, 30)), np.sort(np.random.default_rng(1).uniform(-3, 3, 8))),
    "finer_target": (np.array([0.0, 1.0, 2.5, 4.0]), np.linspace(0.0, 4.0, 14)),
    "partly_outside": (np.linspace(1.0, 2.0, 11), np.array([0.0, 1.05, 1.5, 2.5, 3.0])),
    "wholly_outside": (np.linspace(1.0, 2.0, 5), np.array([-2.0, -1.0, 0.5, 1.0, 2.0, 2.5])),  # touching at 1.0 and 2.0: no overlap
    "one_cell_each": (np.array([0.0, 1.0]), np.array([0.25, 0.5])),
}


@pytest.mark.parametrize("name", sorted(AXES))
@pytest.mark.parametrize("src_desc", [False, True])
@pytest.mark.parametrize("dst_desc", [False, True])
def test_axis_tables_equal_the_numpy_restatement(axis, name, src_desc, dst_desc):
    sb, db = AXES[name]
    sb, db = (sb[::-1] if src_desc else sb), (db[::-1] if dst_desc else db)
    first, count, w, full = equals_oracle(axis(sb, db), sb, db)
    if name == "wholly_outside":
        want = np.array([0, 0, 0, 4, 0])
        assert np.array_equal(count, want[::-1] if dst_desc else want)  # touching cells have no overlap
    if name == "partly_outside":
        assert (count > 0).sum() == 3 and count.min() == 0
    if name == "integer_factor":
        assert np.array_equal(count, [4, 4, 4]) and np.array_equal(full, [1.0, 1.0, 1.0])
        assert np.array_equal(first, [8, 4, 0] if src_desc != dst_desc else [0, 4, 8])
    if name == "finer_target":
        assert count.max() == 2 and (count == 1).any()  # most target cells lie inside one source cell


def test_descending_storage_reverses_the_runs(axis):
    sb, db = AXES["straddling"]
    up, down = axis(sb, db), axis(sb[::-1], db)
    n = len(sb) - 1
    assert np.array_equal(down["first"], n - up["first"] - up["count"])
    assert all(np.array_equal(a, b[::-1]) for a, b in zip(down["w"], up["w"]))


def test_axis_refusals_and_their_order(axis):
    good = [0.0, 1.0, 2.0]
    assert axis([0.0, 2.0, 1.0], good) == (INVALID, "sd_remap: non-monotonic or duplicated source bounds of 'lat'")
    assert axis([0.0, 1.0, 1.0], good)[1].startswith("sd_remap: non-monotonic or duplicated source")
    assert axis(good, [2.0, 2.0]) == (INVALID, "sd_remap: non-monotonic or duplicated target bounds of 'lat'")
    assert axis(good, [2.0, 1.0, 1.5])[0] == INVALID
    assert axis([0.0, float("nan"), 2.0], good) == (INVALID, "sd_remap: NaN in the source bounds of 'lat'")
    assert axis(good, [float("nan"), 1.0]) == (INVALID, "sd_remap: NaN in the target bounds of 'lat'")
    assert axis([0.0], good) == (INVALID, "sd_remap: no source cell along 'lat'")
    assert axis(good, [0.0]) == (INVALID, "sd_remap: no target cell along 'lat'")
    # the order: sizes, NaN (source, target), monotonicity (source, target)
    assert axis([0.0], [float("nan"), 1.0])[1].startswith("sd_remap: no source cell")
    assert axis([0.0, float("nan"), 0.0], [float("nan"), 1.0])[1].startswith("sd_remap: NaN in the source")
    assert axis([0.0, 2.0, 1.0], [float("nan"), 1.0])[1].startswith("sd_remap: NaN in the target")
    assert axis([0.0, 2.0, 1.0], [1.0, 1.0])[1].startswith("sd_remap: non-monotonic or duplicated source")


# ---- plans ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(ask):
    def run(what="plan", T=14600, ny=250, nx=400, Ny=16, Nx=25, ld=None, ld_out=None, min_valid=0.5, f32=False, aligned=True, grids=None):
        ld = ny * nx if ld is None else ld
        ld_out = Ny * Nx if ld_out is None else ld_out
        tail = ["uniform"] if grids is None else sum((words(b) for b in grids), [])
        lines = ask(" ".join([what] + [str(v) for v in (T, ny, nx, Ny, Nx, ld, ld_out, repr(float(min_valid)), int(f32), int(aligned))] + tail))
        first = lines[0]
        if first.startswith("error "):
            _, code, msg = first.split(" ", 2)
            return {"error": int(code), "message": msg}
        p = {k: int(v) for k, v in (w.split("=") for w in first.split()[1:])}
        if what == "plan":
            p["tiles"] = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[1:]]
        return p

    return run


def test_plan_of_the_benchmark_shape(plan):
    p = plan()
    tiles = p.pop("tiles")
    assert p == dict(cols=2, block=256, tile_width=128, lds_bytes=32768, ntiles=4, nchunks=229, blocks=4 * 16 * 229, time_chunk=CHUNK,
                     steps_per_wave=PER_WAVE, batch=BATCH)
    assert tiles == [(0, 8, 0, 128), (8, 8, 128, 128), (16, 8, 256, 128), (24, 1, 384, 16)]  # (first column, columns, span start, span)
    q = plan(f32=True)
    assert (q["cols"], q["tile_width"], q["lds_bytes"], q["tiles"]) == (4, 256, 65536, [(0, 16, 0, 256), (16, 9, 256, 144)])
    assert q["lds_bytes"] <= 160 * 1024 // 2  # at least two workgroups per CU


@pytest.mark.parametrize("nx,ld,aligned,f32,cols", [(400, None, True, False, 2), (400, None, False, False, 1), (401, None, True, False, 1),
                                                    (400, 250 * 400 + 1, True, False, 1), (400, 250 * 400 + 2, True, False, 2),
                                                    (400, 250 * 400 + 2, True, True, 2), (400, 250 * 400 + 4, True, True, 4),
                                                    (402, None, True, True, 2), (64, None, True, False, 1), (66, None, True, False, 2),
                                                    (68, None, True, True, 4), (400, None, False, True, 1)])
def test_columns_per_lane_need_aligned_groups_and_a_row_wider_than_a_wave(plan, nx, ld, aligned, f32, cols):
    p = plan(nx=nx, ld=ld, aligned=aligned, f32=f32, Nx=2)
    assert (p["cols"], p["tile_width"]) == (cols, LANES * cols)
    assert all(s0 % cols == 0 and ns % cols == 0 and s0 + ns <= nx for _, _, s0, ns in p["tiles"])


def uniform(n, lo=0.0, hi=1.0):
    return lo + (hi - lo) * np.arange(n + 1) / n


SHAPES = [((2, 2), (1, 1)), ((7, 9), (3, 4)), ((16, 130), (4, 13)), ((5, 257), (2, 3)), ((3, 700), (1, 66)), ((9, 9), (12, 11)), ((3, 600), (2, 1))]


@pytest.mark.parametrize("src,dst", SHAPES)
@pytest.mark.parametrize("T", [1, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + PER_WAVE + 1])
@pytest.mark.parametrize("f32", [False, True])
def test_every_tile_row_and_step_is_visited_once(plan, src, dst, T, f32):
    (ny, nx), (Ny, Nx) = src, dst
    kw = dict(T=T, ny=ny, nx=nx, Ny=Ny, Nx=Nx, f32=f32)
    assert plan("cover", **kw) == dict(cells_min=1, cells_max=1, steps_min=1, steps_max=1, outside=0, src_missed=0, wide_shared=0)
    p = plan(**kw)
    assert p["nchunks"] == -(-T // CHUNK) and p["blocks"] == p["ntiles"] * Ny * p["nchunks"]
    # every target column lies in exactly one tile, in order
    cols = [c for c0, nc, _, _ in p["tiles"] for c in range(c0, c0 + nc)]
    assert cols == list(range(Nx))
    assert all(nc == 1 or ns <= p["tile_width"] for _, nc, _, ns in p["tiles"])  # only a single column is walked in strips


def test_a_target_beyond_the_hull_and_descending_grids_are_covered(plan):
    grids = (uniform(9, 40.0, 30.0), uniform(140, 0.0, 7.0), uniform(5, 25.0, 45.0), uniform(70, 9.0, -2.0))  # (src y, src x, dst y, dst x)
    kw = dict(T=7, ny=9, nx=140, Ny=5, Nx=70, grids=grids)
    assert plan("cover", **kw) == dict(cells_min=1, cells_max=1, steps_min=1, steps_max=1, outside=0, src_missed=0, wide_shared=0)
    tiles = plan(**kw)["tiles"]
    assert [c for c0, nc, _, _ in tiles for c in range(c0, c0 + nc)] == list(range(70)) and len(tiles) > 1


def test_a_single_column_wider_than_a_tile_gets_its_own(plan):
    p = plan(T=1, ny=5, nx=257, Ny=2, Nx=3)
    assert p["cols"] == 1 and p["tile_width"] == 64
    assert p["tiles"] == [(0, 1, 0, 86), (1, 1, 85, 87), (2, 1, 171, 86)]  # each column alone: 86 > 64 source columns
    p = plan(T=1, ny=3, nx=600, Ny=2, Nx=1)
    assert p["cols"] == 2 and p["tiles"] == [(0, 1, 0, 600)]


def test_refusals_and_their_messages(plan):
    def err(**kw):
        p = plan(**kw)
        return p["error"], p["message"]

    assert err(T=0) == (INVALID, "sd_remap: bad sizes (T=0, source 250 x 400, target 16 x 25)")
    assert err(T=-3)[1].startswith("sd_remap: bad sizes (T=-3")
    assert err(ld=99_999) == (INVALID, "sd_remap: ld = 99999 is less than the 100000 cells of the source grid")
    assert err(ld_out=399) == (INVALID, "sd_remap: ld_out = 399 is less than the 400 cells of the target grid")
    assert "error" not in plan(ld=100_000, ld_out=400)
    assert err(min_valid=1.5) == (INVALID, "sd_remap: min_valid = 1.5 lies outside [0, 1]")
    assert err(min_valid=-0.25)[1] == "sd_remap: min_valid = -0.25 lies outside [0, 1]"
    assert err(min_valid=float("nan"))[1].startswith("sd_remap: min_valid = ") and "error" not in plan(min_valid=0.0) and "error" not in plan(min_valid=1.0)
    # the order: sizes, leading dimensions (source, output), min_valid
    assert err(T=0, ld=1, ld_out=1, min_valid=2.0)[1].startswith("sd_remap: bad sizes")
    assert err(ld=1, ld_out=1, min_valid=2.0)[1].startswith("sd_remap: ld = 1 ")
    assert err(ld_out=1, min_valid=2.0)[1].startswith("sd_remap: ld_out = 1 ")


def test_the_limit_of_two_to_the_31(plan):
    big = (INVALID, "sd_remap: grid too large")

    def err(**kw):
        p = plan(**kw)
        return p.get("error"), p.get("message")

    # workgroups: 4 x 16 x nchunks < 2^31
    most = ((1 << 31) - 1) // 64
    assert plan(T=most * CHUNK)["blocks"] == most * 64 and err(T=most * CHUNK + 1) == big
    # rows, columns and table entries are indexed with int: source + target cells of a dimension < 2^31
    assert err(T=1, ny=1, Ny=1, nx=(1 << 31) - 1, Nx=1) == big and err(T=1, nx=1, Nx=1, ny=1 << 30, Ny=1 << 30) == big
    assert err(T=1, ny=1 << 40, nx=1 << 40, Ny=1, Nx=1, ld=1) == big  # (ny * nx itself does not fit)
    assert err(T=1 << 62) == big  # T * ld
