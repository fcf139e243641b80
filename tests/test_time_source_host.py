"""CPU: how the source of every lazy time-axis array comes into HBM -- which of the three paths it takes (taken whole from another lazy
array's ``device_field``, produced in HBM block by block, uploaded from the host) and how the axis is cut --, pinned for every consumer x
source kind x ``scratch_bytes`` on the stand-in engine of tests/_oracle_engine.py, which records every upload and engine call.

The expected traces are written out from the block rule, not computed by the package's cutters: a block holds at most
``max(1, scratch_bytes // (C * itemsize))`` steps (itemsize 8 for a produced source, the host dtype's for an upload); the bin plans take
whole bins, at least one; the halo plan takes the steps of the windows around its rows in as well; ``quantile`` takes the whole axis.
90 daily steps from 2001-01-01 on a 4 x 5 grid (C = 20), ``"MS"`` bins of 31 / 28 / 31 steps; the lazy sources over the month have 3.

The ``test_failure_*`` cases make the k-th engine call raise and ask that no device buffer outlives it."""
import numpy as np
import pandas as pd
import pytest

import _groupby_oracle as go
import _quantile_oracle as qo
import _remap_oracle as mo
import _resample_oracle as so
import _rolling_oracle as rol
import _spells_oracle as sp
from _oracle_engine import EngineFailure, engine  # noqa: F401  (engine: the fixture)

F4, F8 = np.dtype(np.float32), np.dtype(np.float64)
T, NY, NX, C = 90, 4, 5, 20
TIME = pd.date_range("2001-01-01", periods=T, freq="D")
LAT, LON = np.array([44.0, 42.0, 40.0, 38.0]), np.array([-110.0, -108.0, -106.0, -104.0, -102.0])
RNG = np.random.default_rng(11)
V = 5.0 * RNG.normal(size=(T, NY, NX))
V[RNG.uniform(size=V.shape) < 0.05] = np.nan
V8 = 5.0 * RNG.normal(size=(T, 8, 10))  # a finer grid whose cells tile those of the 4 x 5 one
VC = 5.0 * RNG.normal(size=(T, 2, 2))  # a coarser grid whose hull holds the 4 x 5 one
CLIM = RNG.normal(size=(3, NY, NX))
TABLE = RNG.normal(size=(2, NY, NX))
ROOMS = (None, 40, 60, 1)  # steps of the source one block has room for (None: the default scratch_bytes; 1: scratch_bytes=1)


def grid(values, lat=LAT, lon=LON, time=TIME):
    from skdownscale_amd import GridArray

    return GridArray(values, ("time", "lat", "lon"), dict(time=time, lat=lat, lon=lon))


def fine():
    return grid(V8, np.linspace(44.5, 37.5, 8), np.linspace(-110.5, -101.5, 10))


def coarse():
    return grid(VC, np.array([45.0, 37.0]), np.array([-111.0, -101.0]))


# kind -> (the source, the dim a consumer walks)
SOURCES = {
    "f4": lambda: (grid(V.astype(np.float32)), "time"),
    "f8": lambda: (grid(V), "time"),
    "interp": lambda: (coarse().interp_like(grid(V)), "time"),
    "remap_host": lambda: (fine().remap_like(grid(V)), "time"),
    "resample": lambda: (grid(V).resample(time="MS").mean(), "time"),
    "rolling": lambda: (grid(V).rolling(time=5).mean(), "time"),
    "group_reduced": lambda: (grid(V).groupby("time.month").mean(), "month"),
    "group_applied": lambda: (grid(V).groupby("time.month") - CLIM, "time"),
    "disagg": lambda: (grid(CLIM, time=TIME[[0, 31, 59]]).disaggregate(grid(V), years="same"), "time"),
    "quantile": lambda: (grid(V).quantile(0.5, "time", by="time.month"), "month"),
    "remap": lambda: (fine().rolling(time=5).mean().remap_like(grid(V)), "time"),
}
HOST, PRODUCED = ("f4", "f8"), ("interp", "remap_host")
STEPS = dict.fromkeys(SOURCES, T) | dict(resample=3, group_reduced=3, quantile=3)
up = lambda n, dtype=F8: ("upload", n, dtype)  # noqa: E731
# what making the field of a lazy source (at the default scratch_bytes) leaves in the trace
OWN = {
    "interp": [("regrid", 0, T)],
    "remap_host": [up(T), ("remap", T, 0, T)],
    "resample": [up(T), ("resample", T, 0, 3)],
    "rolling": [up(T), ("rolling", T, 0, 0, T)],
    "group_reduced": [up(T), ("groupby_reduce", T, True)],
    "group_applied": [up(3), up(T), ("groupby_apply", T, 0, T)],
    "disagg": [up(T), up(3), ("disaggregate", 0, 3, 0, T)],
    "quantile": [up(T), ("quantile", T)],
    "remap": [up(T), ("rolling", T, 0, 0, T), ("remap", T, 0, T)],
}
# consumer -> the kinds of lazy source it takes whole from HBM (the table of DESIGN.md, copied by hand)
TAKES = {
    "resample": set(),
    "group_reduced": {"resample", "rolling"},
    "group_applied": {"resample", "rolling"},
    "rolling": {"resample", "rolling", "group_reduced", "group_applied", "quantile"},
    "quantile": {"resample", "rolling", "group_reduced", "group_applied", "disagg", "quantile", "remap"},
    "spells": {"resample", "rolling", "group_reduced", "group_applied", "disagg", "quantile", "remap"},
    "remap": {"resample", "rolling", "group_reduced", "group_applied", "disagg", "quantile"},
}

# ---- the cuts, by hand: steps -> room -> blocks ----
ROWS = {T: {None: [(0, 90)], 40: [(0, 40), (40, 80), (80, 90)], 60: [(0, 60), (60, 90)], 1: [(i, i + 1) for i in range(90)]},
        3: {None: [(0, 3)], 40: [(0, 3)], 60: [(0, 3)], 1: [(0, 1), (1, 2), (2, 3)]}}
# (first bin, behind the last bin, first step, behind the last step) of the "MS" bins: 31 + 28 fit into 60 steps, 28 + 31 do not
BINS = {T: {None: [(0, 3, 0, 90)], 40: [(0, 1, 0, 31), (1, 2, 31, 59), (2, 3, 59, 90)], 60: [(0, 2, 0, 59), (2, 3, 59, 90)],
            1: [(0, 1, 0, 31), (1, 2, 31, 59), (2, 3, 59, 90)]},
        3: {None: [(0, 3, 0, 3)], 40: [(0, 3, 0, 3)], 60: [(0, 3, 0, 3)], 1: [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]}}
ONE_BIN = dict.fromkeys(ROOMS, [(0, 1, 0, 3)])  # (the whole axis of the 3 months: a bin is never cut)
# window 3, centred: one step before and one behind; (first row, behind the last row, first step held, behind the last step held);
# 40 steps hold 38 rows and their halo, 60 hold 58; one step holds no row beside its halo: refused
HALO = {T: {None: [(0, 90, 0, 90)], 40: [(0, 38, 0, 39), (38, 76, 37, 77), (76, 90, 75, 90)], 60: [(0, 58, 0, 59), (58, 90, 57, 90)], 1: None},
        3: {None: [(0, 3, 0, 3)], 40: [(0, 3, 0, 3)], 60: [(0, 3, 0, 3)], 1: None}}


def fill(feed, b0, b1, at=0):
    """what bringing the steps [b0, b1) of a source into the rows at .. of a buffer leaves in the trace"""
    n = b1 - b0
    return {"taken": [], "f4": [up(n, F4)], "f8": [up(n)], "interp": [("regrid", b0, b1)], "remap_host": [up(n), ("remap", n, at, at + n)]}[feed]


def labels(n):
    return np.arange(n) % 2


def bins_of(dim, n):
    return np.array([0, n]) if dim == "month" else np.array([0, 31, 59, 90] if n == T else [0, 1, 2, 3])


def scratch(kw):
    return {} if kw is None else dict(scratch_bytes=kw)


# consumer -> (source, dim, scratch_bytes or None) -> the lazy array
CONSUMERS = {
    "resample": lambda s, d, sb: s.resample(time="MS", **scratch(sb)).mean(),
    "group_reduced": lambda s, d, sb: s.groupby(**{d: labels(s.sizes[d])}, **scratch(sb)).sum(),
    "group_applied": lambda s, d, sb: s.groupby(**{d: labels(s.sizes[d])}, **scratch(sb)) - TABLE,
    "rolling": lambda s, d, sb: s.rolling(**{d: 3}, center=True, min_periods=1, **scratch(sb)).mean(),
    "quantile": lambda s, d, sb: s.quantile(0.5, d, **scratch(sb)),
    "spells": lambda s, d, sb: (s.where(">", 0.5, dim=d, **scratch(sb)).count() if d == "month" else
                                s.where(">", 0.5, dim=d, **scratch(sb)).resample(time="MS").count()),
    "remap": lambda s, d, sb: s.remap_like(coarse(), **scratch(sb)),
}


def oracle(consumer, m, dim):
    """the consumer's result [rows, cells] of the materialised source ``m`` [steps, 20]"""
    n = len(m)
    if consumer == "resample":
        return so.resample(m, bins_of(dim, n), "mean")
    if consumer == "group_reduced":
        return go.reduce(m, labels(n), 2, "sum")
    if consumer == "group_applied":
        return go.apply(m, labels(n), TABLE.reshape(2, C), "sub")
    if consumer == "rolling":
        return rol.rolling(m, 3, "mean", center=True, min_periods=1)
    if consumer == "quantile":
        return qo.quantile_field(m, 0.5)
    if consumer == "spells":
        return sp.spells(m, bins_of(dim, n), ">", 0.5, ("count",))
    lat, lon, c = mo.area_bounds(mo.cell_bounds(LAT)), mo.cell_bounds(LON), coarse()
    return mo.remap(m.reshape(n, NY, NX), lat, lon, mo.area_bounds(mo.cell_bounds(c.coords["lat"])), mo.cell_bounds(c.coords["lon"]),
                    0.5).reshape(n, -1)


def expected(consumer, feed, room, n, dim):
    """the trace of the consumer's ``device_field`` over a source of ``n`` steps that comes as ``feed``; None: refused"""
    if feed == "taken":
        room = None  # (one block whatever scratch_bytes)
    tr = []
    if consumer in ("resample", "spells"):
        for a, b, r0, r1 in (ONE_BIN if dim == "month" else BINS[n])[room]:
            tr += fill(feed, r0, r1) + [(consumer, r1 - r0, a, b)]
    elif consumer == "group_reduced":
        for r0, r1 in ROWS[n][room]:
            tr += fill(feed, r0, r1) + [("groupby_reduce", r1 - r0, r1 == n)]
    elif consumer == "group_applied":
        tr += [up(2)]  # (the table)
        for r0, r1 in ROWS[n][room]:
            tr += fill(feed, r0, r1) + [("groupby_apply", r1 - r0, r0, r1)]
    elif consumer == "rolling":
        if HALO[n][room] is None:
            return None
        for r0, r1, b0, b1 in HALO[n][room]:
            tr += fill(feed, b0, b1) + [("rolling", b1 - b0, r0 - b0, r0, r1)]
    elif consumer == "quantile":  # the whole axis: a host array in one upload, a produced one in pieces into its rows
        for r0, r1 in ROWS[n][room if feed in PRODUCED else None]:
            tr += fill(feed, r0, r1, at=r0)
        tr += [("quantile", n)]
    elif feed == "taken":
        tr += [("remap", n, 0, n)]
    else:  # the remapper's own block loop over a host array
        for r0, r1 in ROWS[n][room]:
            tr += fill(feed, r0, r1) + [("remap", r1 - r0, r0, r1)]
    return tr


MATERIALISED = {}


def materialised(kind, engine):
    if kind not in MATERIALISED:
        MATERIALISED[kind] = np.asarray(SOURCES[kind]()[0].values).reshape(STEPS[kind], C)
    engine.trace.clear(), engine.uploads.clear()
    engine.live = engine.calls = 0
    return MATERIALISED[kind]


def cases():
    for consumer in CONSUMERS:
        for kind in SOURCES:
            if consumer == "resample" and SOURCES[kind]()[1] != "time":
                continue  # (pandas' resampler needs the datetime coordinate)
            for room in ROOMS:
                yield consumer, kind, room


@pytest.mark.parametrize("consumer,kind,room", list(cases()))
def test_every_source_takes_its_path_and_is_cut_by_the_block_rule(engine, consumer, kind, room):
    m = materialised(kind, engine)
    src, dim = SOURCES[kind]()
    n = STEPS[kind]
    own, stays_lazy = [], None
    if kind in HOST:
        feed = kind
    elif kind in PRODUCED and consumer != "remap":  # (the remapper takes host arrays and lazy time-axis results only)
        feed, stays_lazy = kind, True
    else:
        stays_lazy = kind in TAKES[consumer]
        feed, own = ("taken" if stays_lazy else "f8"), OWN[kind]
    sb = None if room is None else 1 if room == 1 else room * C * (4 if feed == "f4" else 8)
    lazy = CONSUMERS[consumer](src, dim, sb)
    assert engine.trace == [] and not lazy.computed
    want = expected(consumer, feed, room, n, dim)
    if want is None:
        with pytest.raises(ValueError, match=f"holds 1 steps of {C} cells: too few for one step and the 1 \\+ 1 steps of its window"):
            lazy.device_field()
        return
    field = lazy.device_field()
    got = field.to_host()
    head = 1 if consumer == "group_applied" else 0  # (its table goes up before the source is touched)
    assert engine.trace == want[:head] + own + want[head:]
    assert got.dtype == np.float64 and qo.same(got, oracle(consumer, m, dim)) and np.array_equal(np.isnan(got), np.isnan(oracle(consumer, m, dim)))
    if stays_lazy is not None:
        assert src.computed == (not stays_lazy)
    field.free()
    # (InterpolatedGridArray.values leaves its field to the garbage collector)
    assert engine.live == (1 if kind == "interp" and src.computed else 0)


def test_the_issue_s_example_traces(engine):
    src, dim = SOURCES["f4"]()
    for room, want in ((40, [31, 28, 31]), (60, [59, 31])):
        engine.trace.clear()
        src.resample(time="MS", scratch_bytes=room * C * 4).mean().device_field().free()
        assert [e for e in engine.trace if e[0] == "upload"] == [("upload", n, F4) for n in want]


OTHERS = {
    "group_reduced": lambda a: a.groupby("time.month").mean(),
    "quantile": lambda a: a.quantile(0.5, "time", by="time.month"),
    "rolling": lambda a: a.groupby("time.month").mean().rolling(month=3, center=True, min_periods=1).mean(),
    "transposed": lambda a: a.transpose("lat", "time", "lon").groupby("time.month").mean(),  # (a lazy reduction in another cell order)
}


@pytest.mark.parametrize("other,stays_lazy", [("group_reduced", True), ("quantile", True), ("rolling", True), ("transposed", False)])
def test_the_table_of_a_group_applied_array(engine, other, stays_lazy):
    a = grid(V)
    table = np.asarray(OTHERS[other](a).transpose("month", "lat", "lon").values).reshape(3, C)
    o = OTHERS[other](a)
    engine.live = 0
    field = (a.groupby("time.month") - o).device_field()
    assert qo.same(field.to_host(), go.apply(V.reshape(T, C), np.asarray(TIME.month) - 1, table, "sub")) and o.computed == (not stays_lazy)
    field.free()
    assert engine.live == 0


@pytest.mark.parametrize("kind,stays_lazy", [("resample", True), ("rolling", False)])
def test_the_target_of_a_disaggregation(engine, kind, stays_lazy):
    monthly = grid(V).resample(time="MS").mean()
    if kind == "rolling":
        monthly = grid(np.asarray(monthly.values), time=TIME[[0, 31, 59]]).rolling(time=1).mean()
    field = monthly.disaggregate(grid(V), years="same").device_field()
    assert field.shape == (T, C) and monthly.computed == (not stays_lazy)
    field.free()
    assert engine.live == 0


# ---- a failing engine call leaves nothing on the device ----------------------------------------------------------------------------
def failing(engine, k, make):
    lazy = make()
    engine.live, engine.calls, engine.fail_at = 0, 0, k
    with pytest.raises(EngineFailure):
        lazy.device_field()
    assert engine.live == 0


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("consumer", [c for c in CONSUMERS if c != "quantile"])
def test_failure_in_a_two_block_walk_frees_every_buffer(engine, consumer, k):
    src, dim = SOURCES["f8"]()
    failing(engine, k, lambda: CONSUMERS[consumer](src, dim, 60 * C * 8))


def test_failure_of_the_quantile_frees_the_field(engine):
    src, dim = SOURCES["f8"]()
    failing(engine, 1, lambda: CONSUMERS["quantile"](src, dim, None))


@pytest.mark.parametrize("k", [1, 2])
def test_failure_in_a_two_block_disaggregation_frees_every_buffer(engine, k):
    failing(engine, k, lambda: grid(CLIM, time=TIME[[0, 31, 59]]).disaggregate(grid(V), years="same", scratch_bytes=60 * C * 8))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("consumer", ["group_reduced", "rolling", "quantile"])
def test_failure_while_a_lazy_source_is_held_frees_its_field(engine, consumer, k):
    """engine call 1 makes the source's field, call 2 is the consumer's"""
    src, dim = SOURCES["resample"]()
    failing(engine, k, lambda: CONSUMERS[consumer](src, dim, None))
