"""The groupby launch plans (scikit-downscale_amd/csrc/sd_groupby_plan.h), checked on the host: the header is compiled with g++ into a
small driver (tests/groupby_plan_check.cpp) that prints plans, checks and sorts the group ids of a call and walks the grid of a plan
the way groupby_reduce_kernel / groupby_apply_kernel decode it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, SUM = 0, 1
SUB, ADD, MUL, DIV = 0, 1, 2, 3
INVALID = 1
WAVES, PER_WAVE, BATCH, RUN, FEW = 4, 2, 8, 16, 16  # waves of a workgroup, bins of a wave, rows in flight, rows of an apply run, few groups


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("plan") / "groupby_plan_check"
    src = os.path.join(ROOT, "tests", "groupby_plan_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(path)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return str(path)


@pytest.fixture(scope="module")
def ask(exe):
    def run(words):
        out = subprocess.run([exe], input=" ".join(str(int(w) if not isinstance(w, str) else w) for w in words) + "\n", capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end", lines
        first = lines[0]
        if first.startswith("error "):
            _, code, msg = first.split(" ", 2)
            return {"error": int(code), "message": msg}
        return {k: (v if "," in v or first.startswith("tables") else int(v)) for k, v in (w.split("=") for w in first.split()[1:])}

    return run


@pytest.fixture(scope="module")
def reduce(ask):
    def run(what="reduce", op=MEAN, f32=False, T=14600, C=100_000, ld=None, G=12, ld_acc=None, out=True, ld_out=None, aligned=(True,) * 4, group=None):
        ld, ld_acc, ld_out = (C if v is None else v for v in (ld, ld_acc, ld_out))
        return ask([what, op, f32, T, C, ld, G, ld_acc, out, ld_out, *aligned, *([] if group is None else group)])

    return run


@pytest.fixture(scope="module")
def apply(ask):
    def run(what="apply", op=SUB, f32=False, T=14600, C=100_000, ld=None, G=12, ld_t=None, ld_out=None, aligned=(True,) * 3, group=None):
        ld, ld_t, ld_out = (C if v is None else v for v in (ld, ld_t, ld_out))
        return ask([what, op, f32, T, C, ld, G, ld_t, ld_out, *aligned, *([] if group is None else group)])

    return run


def test_plans_of_the_benchmark_shape(reduce, apply):
    # 12 groups: one per wave, three workgroups of four per cell tile, no idle wave
    month = dict(cols=2, block=256, ctiles=782, bin_groups=3, blocks=782 * 3, bins_per_wave=1, batch=BATCH, run=RUN)
    assert reduce() == month and reduce(op=SUM) == month and reduce(out=False) == month
    assert reduce(f32=True) == dict(month, cols=4, ctiles=391, blocks=391 * 3)
    # 366 groups: two per wave, 46 workgroups of eight per cell tile
    doy = dict(month, bin_groups=46, blocks=782 * 46, bins_per_wave=PER_WAVE)
    assert reduce(G=366) == doy and reduce(G=366, f32=True) == dict(doy, cols=4, ctiles=391, blocks=391 * 46)
    # apply: 913 runs of 16 rows, two per wave
    sub = dict(cols=2, block=256, ctiles=782, bin_groups=115, blocks=782 * 115, bins_per_wave=PER_WAVE, batch=BATCH, run=RUN)
    assert all(apply(op=op) == sub for op in (SUB, ADD, MUL, DIV)) and apply(G=366) == sub
    assert apply(f32=True) == sub  # two cells per lane for float32 too: the table and the output go as one 16-byte access per lane


@pytest.mark.parametrize("G,per_wave,groups", [(1, 1, 1), (3, 1, 1), (4, 1, 1), (5, 1, 2), (8, 1, 2), (9, 1, 3), (12, 1, 3), (16, 1, 4), (17, 2, 3),
                                               (24, 2, 3), (25, 2, 4), (366, 2, 46)])
def test_few_groups_take_one_bin_per_wave(reduce, G, per_wave, groups):
    p = reduce(G=G)
    assert (p["bins_per_wave"], p["bin_groups"]) == (per_wave, groups) == (1 if G <= FEW else PER_WAVE, -(-G // (WAVES * per_wave)))
    assert p["blocks"] == p["ctiles"] * groups


@pytest.mark.parametrize("f32,C,kw,cols", [
    # float64: two cells per lane need C and every leading dimension even and every pointer on 16 bytes
    (False, 100, {}, 2), (False, 101, {}, 1), (False, 1, {}, 1), (False, 2, {}, 2),
    (False, 100, dict(ld=101), 1), (False, 100, dict(ld_acc=101), 1), (False, 100, dict(ld_out=101), 1),
    (False, 100, dict(ld=102, ld_acc=104, ld_out=106), 2),
    (False, 100, dict(aligned=(False, True, True, True)), 1), (False, 100, dict(aligned=(True, False, True, True)), 1),
    (False, 100, dict(aligned=(True, True, False, True)), 1), (False, 100, dict(aligned=(True, True, True, False)), 1),
    # the output counts only when there is one
    (False, 100, dict(ld_out=101, out=False), 2), (False, 100, dict(aligned=(True, True, True, False), out=False), 2),
    # float32: four where everything divides by four, else two, else one
    (True, 100, {}, 4), (True, 102, {}, 2), (True, 101, {}, 1), (True, 4, {}, 4), (True, 260, {}, 4),
    (True, 100, dict(ld=102), 2), (True, 100, dict(ld_acc=102), 2), (True, 100, dict(ld_out=102), 2),
    (True, 100, dict(ld=104, ld_acc=108, ld_out=112), 4), (True, 100, dict(ld=101), 1), (True, 100, dict(aligned=(True, True, False, True)), 1)])
def test_reduce_cells_per_lane_follow_alignment_and_evenness(reduce, f32, C, kw, cols):
    p = reduce(f32=f32, C=C, **kw)
    assert p["cols"] == cols and p["ctiles"] == -(-C // (64 * cols)) and p["blocks"] == p["ctiles"] * 3


@pytest.mark.parametrize("f32,C,kw,cols", [
    (False, 100, {}, 2), (False, 101, {}, 1), (False, 100, dict(ld=101), 1), (False, 100, dict(ld_t=101), 1), (False, 100, dict(ld_out=101), 1),
    (False, 100, dict(ld=102, ld_t=104, ld_out=106), 2), (False, 100, dict(aligned=(False, True, True)), 1),
    (False, 100, dict(aligned=(True, False, True)), 1), (False, 100, dict(aligned=(True, True, False)), 1),
    # float32: never four (the 32 bytes of table and output of a lane would be two accesses 32 bytes apart)
    (True, 100, {}, 2), (True, 102, {}, 2), (True, 101, {}, 1), (True, 100, dict(ld_t=102), 2), (True, 100, dict(ld=104, ld_t=108, ld_out=112), 2),
    (True, 100, dict(ld=101), 1), (True, 100, dict(aligned=(True, False, True)), 1)])
def test_apply_cells_per_lane_follow_alignment_and_evenness(apply, f32, C, kw, cols):
    p = apply(f32=f32, C=C, **kw)
    assert p["cols"] == cols and p["ctiles"] == -(-C // (64 * cols)) and p["blocks"] == p["ctiles"] * 115


def test_reduce_refusals_and_their_messages(reduce):
    def err(**kw):
        p = reduce(**kw)
        return p["error"], p["message"]

    assert err(op=2) == (INVALID, "sd_groupby_reduce: unknown op code 2") and err(op=-1)[1].endswith("code -1")
    for bad in (dict(T=0), dict(C=0), dict(T=-1), dict(C=-5)):
        code, msg = err(**bad)
        assert code == INVALID and msg.startswith("sd_groupby_reduce: bad sizes (T="), bad
    assert err(T=0) == (INVALID, "sd_groupby_reduce: bad sizes (T=0, C=100000)")
    assert err(G=0) == (INVALID, "sd_groupby_reduce: bad sizes (G=0)") and err(G=-3) == (INVALID, "sd_groupby_reduce: bad sizes (G=-3)")
    for name in ("ld", "ld_acc", "ld_out"):
        assert err(**{name: 99_999}) == (INVALID, f"sd_groupby_reduce: {name} = 99999 is less than the 100000 cells of a row")
    assert "error" not in reduce(ld_out=5, out=False)  # (not read without an output)
    # the order: op, sizes, groups, leading dimensions
    assert err(op=5, T=0, G=0, ld=1)[1].startswith("sd_groupby_reduce: unknown op")
    assert err(T=0, G=0, ld=1)[1].startswith("sd_groupby_reduce: bad sizes (T=")
    assert err(G=0, ld=1)[1].startswith("sd_groupby_reduce: bad sizes (G=")
    assert err(ld=1, ld_acc=1)[1].startswith("sd_groupby_reduce: ld = 1")


def test_apply_refusals_and_their_messages(apply):
    def err(**kw):
        p = apply(**kw)
        return p["error"], p["message"]

    assert err(op=4) == (INVALID, "sd_groupby_apply: unknown op code 4") and err(op=-1)[1].endswith("code -1")
    assert err(T=0) == (INVALID, "sd_groupby_apply: bad sizes (T=0, C=100000)") and err(C=-1)[1].startswith("sd_groupby_apply: bad sizes (T=")
    assert err(G=0) == (INVALID, "sd_groupby_apply: bad sizes (G=0)")
    for name in ("ld", "ld_t", "ld_out"):
        assert err(**{name: 99_999}) == (INVALID, f"sd_groupby_apply: {name} = 99999 is less than the 100000 cells of a row")
    assert err(op=9, T=0, G=0)[1].startswith("sd_groupby_apply: unknown op") and err(T=0, G=0, ld=1)[1].startswith("sd_groupby_apply: bad sizes (T=")


def test_group_ids_outside_the_groups_are_refused(reduce, apply):
    ok = [0, 2, 1, 2, 0]
    for run, who in ((reduce, "sd_groupby_reduce"), (apply, "sd_groupby_apply")):
        what = who[3:].split("_")[1] + "_groups"
        assert "error" not in run(what, T=5, C=4, G=3, group=ok)
        assert run(what, T=5, C=4, G=3, group=[0, 3, 1, 2, 0]) == dict(error=INVALID, message=f"{who}: group[1] = 3 lies outside the 3 groups")
        assert run(what, T=5, C=4, G=3, group=[0, 2, 1, 2, -1]) == dict(error=INVALID, message=f"{who}: group[4] = -1 lies outside the 3 groups")
        assert run(what, T=5, C=4, G=2, group=ok)["message"] == f"{who}: group[1] = 2 lies outside the 2 groups"
        # a refusal of the plan comes first and the ids are not read
        assert run(what, T=5, C=4, G=3, op=7, group=[9] * 5)["message"] == f"{who}: unknown op code 7"


def test_the_limit_of_two_to_the_31(reduce, apply):
    most = (1 << 31) - 1
    big = dict(error=INVALID, message="sd_groupby_reduce: grid too large")
    # one cell tile, many groups: runs of eight groups
    assert reduce(T=1, C=1, G=most * 8)["blocks"] == most and reduce(T=1, C=1, G=most * 8 + 1) == big
    # few groups, many cell tiles: runs of four groups
    C = (most // 4) * 128  # two cells per lane
    assert reduce(T=1, C=C, G=FEW, out=False)["blocks"] == (most // 4) * 4 and reduce(T=1, C=C + 128, G=FEW, out=False) == big
    groups = most // 782
    assert apply(T=groups * 8 * RUN)["blocks"] == groups * 782
    assert apply(T=groups * 8 * RUN + 1) == dict(error=INVALID, message="sd_groupby_apply: grid too large")
    too_large = dict(error=INVALID, message="sd_groupby_reduce: field too large")
    assert reduce(T=1 << 40, C=1 << 30) == too_large and reduce(T=1, C=1 << 30, G=1 << 40) == too_large
    assert apply(T=1 << 40, C=1 << 30) == dict(error=INVALID, message="sd_groupby_apply: field too large")


def tables(ask, group, G):
    t = ask(["tables", len(group), G, *group])
    return [int(v) for v in t["rows"].split(",")], [int(v) for v in t["offsets"].split(",")]


@pytest.mark.parametrize("name,group,G", [
    ("scattered", list(np.random.default_rng(5).integers(0, 7, size=200)), 7),
    ("consecutive", [0] * 5 + [1] * 3 + [2] * 9, 3),
    ("empty groups first, inside and last", [1, 3, 3, 1, 5, 1], 8),
    ("single group", [0] * 11, 1),
    ("descending", [4, 3, 2, 1, 0], 5),
    ("one row", [2], 4)])
def test_groupby_tables_are_a_stable_counting_sort(ask, name, group, G):
    rows, offsets = tables(ask, group, G)
    T = len(group)
    assert len(offsets) == G + 1 and offsets[0] == 0 and offsets[G] == T and all(a <= b for a, b in zip(offsets, offsets[1:]))
    assert sorted(rows) == list(range(T))  # every row exactly once
    for g in range(G):
        mine = rows[offsets[g]:offsets[g + 1]]
        assert mine == [t for t in range(T) if group[t] == g]  # the rows of the group, in row order
    assert rows == list(np.argsort(group, kind="stable"))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130, 257, 260])
@pytest.mark.parametrize("G", [1, 3, 8, 9, 12, 16, 17, 25])  # one bin per wave up to 16 groups, two above
def test_every_cell_of_every_group_is_owned_by_exactly_one_lane(reduce, f32, C, G):
    rng = np.random.default_rng(G)
    group = rng.integers(0, G, size=40)
    if G > 1:
        group[group == G // 2] = 0  # an absent group
    c = reduce("reduce_cover", f32=f32, T=40, C=C, G=G, group=list(group))
    assert c == dict(owned_min=1, owned_max=1, added_min=1, added_max=1, outside=0)
    p = reduce(f32=f32, T=40, C=C, G=G)
    assert p["bins_per_wave"] == (1 if G <= FEW else PER_WAVE) and p["ctiles"] == -(-C // (64 * p["cols"]))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("C", [1, 65, 130, 260])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 16, 17, 32, 33, 120, 128, 129, 300])
def test_the_apply_grid_writes_every_row_and_cell_once(apply, f32, C, T):
    assert apply("apply_cover", f32=f32, T=T, C=C) == dict(written_min=1, written_max=1, outside=0)
    assert apply(f32=f32, T=T, C=C)["bin_groups"] == -(-(-(-T // RUN)) // (WAVES * PER_WAVE))
