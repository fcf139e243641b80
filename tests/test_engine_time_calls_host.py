"""CPU: what the time-axis wrappers (``resample`` .. ``rolling`` with their ``_host`` twins), the constructed- and localized-analog wrappers
(``ca_*``) and ``RegridState`` / ``RemapState.apply`` / ``apply_host`` of engine.py hand to the C ABI, pinned on the stand-in library of
tests/_recording_lib.py (no library, no GPU), in the style of tests/test_engine_calls_host.py: the entry point and the full argument list
of each call through the ``_host`` twin (``host``), with host arrays that the wrapper uploads (``up``), on resident ``.cells()`` views whose
pitch (12) is larger than their cells (8) (``res``) and, for the calls that give statistic planes, on a row view inside a longer array
(``planes``); the allocations, uploads and frees of each call (``TRAFFIC``); what is freed when the entry point fails; and every refusal
with what had reached the library by then.

``CALLS``, ``TRAFFIC``, ``FAILED`` and ``REACHED`` are written out literally, argument by argument in the order of include/sd_downscale.h
(the notation is that of tests/test_engine_calls_host.py; in ``TRAFFIC`` an allocation is ``[ctx, bytes, &]``, an upload ``[ctx, block, host
array, bytes]``, a free ``[ctx, block]``).  All of them were recorded from the wrappers as they stood before they were folded onto the
shared argument layer, each feature with a copy of the previous one's checks, so they hold on both sides of that change: where the old
wrappers had allocated ``out`` and uploaded host fields before a refusal spoke, ``REACHED`` says so as it was.  The cases whose id carries
``rule_`` pin what the fold introduced, all in ``RegridState.apply``: a ``src`` or ``out`` of another context is refused, and an uploaded
host ``src`` is freed when the call ends, also when it fails (``-k "not rule_"`` deselects them)."""
import numpy as np
import pytest

from _recording_lib import RecordingLib, context

T, CELLS, LD, C0, M, G = 24, 8, 12, 2, 2, 3
TL, TQ, K, NY, NX = 6, 4, 3, 2, 4
PLANE_ROWS, FIRST_ROW = 5, 1  # the ``plane_rows`` form: the M bins of a call are the rows 1 .. 2 of planes of 5 rows
REGRID_INFO = ("sd_regrid_info", (0, 3, 4, 5, 6))  # method, ny, nx, Ny, Nx
REMAP_INFO = ("sd_remap_info", (3, 4, 2, 2, 7, 9))  # ny, nx, Ny, Nx, entries
FLOATS = dict(A=(T, CELLS), B=(T, CELLS), TAB=(G, CELLS), TAB1=(1, CELLS), TARGET=(M, CELLS), L=(TL, CELLS), Q=(TQ, CELLS), F=(TL, CELLS),
              SRC=(TQ, 3, 4), FINE=(TQ, 12))
INTS = dict(GROUP=np.arange(T) % G, BIN_GROUP=np.arange(M) % G, KEY_L=np.arange(TL) % 4, KEY_Q=np.arange(TQ) % 4, EXCL_L=np.arange(TL) // 2,
            EXCL_Q=np.arange(TQ) // 2)


class Boom(Exception):
    pass


class FailingLib(RecordingLib):
    """the stand-in with one entry point that is recorded and then raises"""

    def __init__(self, fail):
        super().__init__()
        self.fail = fail

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != self.fail:
            return call

        def failing(*args):
            call(*args)
            raise Boom(name)
        return failing


class Engine:
    """a recording context with the arrays of the cases: host ones by their names (``A32``: the float32 one), resident ones (``d`` + name)
    as the cells 2 .. of made-up arrays four cells wider"""

    def __init__(self, lib=None):
        self.ctx = context(lib)
        self.lib = self.ctx.lib
        self.states = []
        for name, shape in FLOATS.items():
            for suffix, dtype in (("", np.float64), ("32", np.float32)):
                setattr(self, name + suffix, self.lib.host(name + suffix, np.zeros(shape, dtype=dtype)))
                setattr(self, "d" + name + suffix, self.wide("d" + name + suffix, shape, dtype))
        for name, a in INTS.items():
            setattr(self, name, self.lib.host(name, np.ascontiguousarray(a, dtype=np.int32)))
        self.OFFSETS = self.lib.host("OFFSETS", np.array([0, 12, T], dtype=np.int64))
        self.SRC_ROW = self.lib.host("SRC_ROW", np.arange(T, dtype=np.int64) % 7)
        self.WC = self.lib.host("WC", np.ones(CELLS))
        self.dSUM, self.dCOUNT = self.wide("dSUM", (G, CELLS)), self.wide("dCOUNT", (G, CELLS), np.int32)
        self.dCELL_OF = self.lib.resident(self.ctx, "dCELL_OF", (CELLS,), np.int32)
        for name, dtype in (("dIDX", np.int32), ("dDIST", np.float64), ("dWEIGHTS", np.float64)):  # the [Tq, k] tables: contiguous
            setattr(self, name, self.lib.resident(self.ctx, name, (TQ, K), dtype))
        self.dSTATUS = self.lib.resident(self.ctx, "dSTATUS", (TQ,), np.int32)
        self.dLOCAL = self.lib.resident(self.ctx, "dLOCAL", (TQ, CELLS), np.int32)
        self.dSRC_WHOLE = self.lib.resident(self.ctx, "dSRC_WHOLE", (TQ, 3, 4))  # (the regrid kernels read a contiguous source)
        self.dSRC_WHOLE32 = self.lib.resident(self.ctx, "dSRC_WHOLE32", (TQ, 3, 4), np.float32)

    def wide(self, name, shape, dtype=np.float64):
        return self.lib.resident(self.ctx, name, shape[:-1] + (shape[-1] + LD - CELLS,), dtype).cells(C0, C0 + shape[-1])

    def out(self, *shape):
        return self.wide("dOUT", shape)

    def planes(self, nstat, bins=M):
        """the rows of this call's bins inside the first of ``nstat`` planes of a longer array"""
        return self.wide("dPLANES", (nstat * PLANE_ROWS, CELLS)).rows(FIRST_ROW, FIRST_ROW + bins)

    def a(self, form, name):
        return None if name is None else getattr(self, name if form in ("host", "up") else "d" + name)

    def call(self, form, name):
        """the wrapper of the form: the ``_host`` twin, or the resident one (which uploads the host arrays it is given)"""
        return getattr(self.ctx, name + "_host" if form == "host" else name)

    def state(self, family):
        name, values = dict(regrid=REGRID_INFO, remap=REMAP_INFO)[family]
        self.lib.info[name] = values
        if family == "regrid":
            state = self.ctx.regrid_create(np.arange(3.0), np.arange(4.0), np.arange(5.0), np.arange(6.0))
        else:
            state = self.ctx.remap_create(np.arange(4.0), np.arange(5.0), np.arange(3.0), np.arange(3.0))
        self.lib.log.clear()
        self.states.append(state)  # (kept: a state that goes away calls its destroy entry point)
        return state


FORMS = ("host", "up", "res")
CASES = {}
STATS2 = ["count", "longest_spell"]

for form in FORMS:
    for f in ("A", "A32"):
        CASES[f"resample-{form}-{f}"] = lambda e, form=form, f=f: e.call(form, "resample")(e.a(form, f), e.OFFSETS, "sum" if f == "A32" else "mean")
        CASES[f"groupby_reduce-{form}-{f}"] = lambda e, form=form, f=f: e.call(form, "groupby_reduce")(e.a(form, f), e.GROUP, G, "sum" if f == "A32" else "mean")
        CASES[f"groupby_apply-{form}-{f}"] = lambda e, form=form, f=f: e.call(form, "groupby_apply")(e.a(form, f), e.GROUP, e.a(form, "TAB"),
                                                                                                     "div" if f == "A32" else "sub")
    CASES[f"spells-{form}-scalar"] = lambda e, form=form: e.call(form, "spells")(e.a(form, "A"), ">", 1.5, e.OFFSETS, "count", 2)
    CASES[f"spells-{form}-host_table"] = lambda e, form=form: e.call(form, "spells")(e.a(form, "A32"), "<=", e.TAB1, e.OFFSETS, STATS2)
    CASES[f"spells-{form}-host_table-group"] = lambda e, form=form: e.call(form, "spells")(e.a(form, "A"), ">=", e.TAB, e.OFFSETS, STATS2, 1, e.GROUP)
    CASES[f"disaggregate-{form}-plain"] = lambda e, form=form: e.call(form, "disaggregate")(e.a(form, "TARGET"), e.a(form, "A32"), e.SRC_ROW, e.OFFSETS)
    CASES[f"disaggregate-{form}-climo"] = lambda e, form=form: e.call(form, "disaggregate")(e.a(form, "TARGET"), e.a(form, "A"), e.SRC_ROW, e.OFFSETS,
                                                                                          "scale_sum", e.a(form, "TAB"), e.BIN_GROUP)
    CASES[f"quantile-{form}-no_group"] = lambda e, form=form: e.call(form, "quantile")(e.a(form, "A"), [0.1, 0.9])
    CASES[f"quantile-{form}-group-G_None"] = lambda e, form=form: e.call(form, "quantile")(e.a(form, "A32"), 0.5, e.GROUP)
    CASES[f"quantile-{form}-group-G"] = lambda e, form=form: e.call(form, "quantile")(e.a(form, "A"), [0.1, 0.9], e.GROUP, 4, "nearest", False)
    CASES[f"quantile-{form}-median"] = lambda e, form=form: e.call(form, "quantile")(e.a(form, "A"), [0.1, 0.9], method="median")
    CASES[f"rolling-{form}-defaults"] = lambda e, form=form: e.call(form, "rolling")(e.a(form, "A"), 5)
    CASES[f"rolling-{form}-options"] = lambda e, form=form: e.call(form, "rolling")(e.a(form, "A32"), 5, "std", 2, 3, 0, True)
for form in ("up", "res"):
    CASES[f"spells-{form}-resident_table-group"] = lambda e, form=form: e.ctx.spells(e.a(form, "A"), "<", e.dTAB, e.OFFSETS, STATS2, group=e.GROUP)
    CASES[f"spells-{form}-resident_table"] = lambda e, form=form: e.ctx.spells(e.a(form, "A"), "<", e.dTAB1, e.OFFSETS, "fraction")
    CASES[f"rolling-{form}-t0-n_out"] = lambda e, form=form: e.ctx.rolling(e.a(form, "A"), 5, t0=3, n_out=7)
    CASES[f"ca_select-{form}-plain"] = lambda e, form=form: e.ctx.ca_select(e.a(form, "L"), e.a(form, "Q"), e.WC, K)
    CASES[f"ca_select-{form}-keys"] = lambda e, form=form: e.ctx.ca_select(e.a(form, "L"), e.a(form, "Q"), e.WC, K, e.KEY_L, e.KEY_Q, 4, 1, e.EXCL_L, e.EXCL_Q)
    CASES[f"ca_weights-{form}-regression"] = lambda e, form=form: e.ctx.ca_weights(e.a(form, "L"), e.a(form, "Q"), e.WC, e.dIDX, e.dDIST, e.dSTATUS)
    CASES[f"ca_weights-{form}-mean"] = lambda e, form=form: e.ctx.ca_weights(e.a(form, "L"), e.a(form, "Q"), e.WC, e.dIDX, e.dDIST, e.dSTATUS, "mean", 0.0)
    CASES[f"ca_local-{form}"] = lambda e, form=form: e.ctx.ca_local(e.a(form, "L"), e.a(form, "Q"), e.WC, (NY, NX), (1, 2), e.dIDX)
CASES["resample-res-out"] = lambda e: e.ctx.resample(e.dA, e.OFFSETS, out=e.out(M, CELLS))
CASES["spells-res-out"] = lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.out(2 * M, CELLS))
CASES["spells-planes"] = lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.planes(2), plane_rows=PLANE_ROWS)
CASES["disaggregate-res-out"] = lambda e: e.ctx.disaggregate(e.dTARGET, e.dA, e.SRC_ROW, e.OFFSETS, "scale_mean", out=e.out(T, CELLS))
CASES["disaggregate-resident_target-host_obs"] = lambda e: e.ctx.disaggregate(e.dTARGET, e.A, e.SRC_ROW, e.OFFSETS)
CASES["groupby_reduce-res-carry-out"] = lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, acc=(e.dSUM, e.dCOUNT), out=e.out(G, CELLS))
CASES["groupby_reduce-res-no_finish"] = lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, finish=False)
CASES["groupby_reduce-up-carry-no_finish"] = lambda e: e.ctx.groupby_reduce(e.A32, e.GROUP, G, "sum", (e.dSUM, e.dCOUNT), finish=False)
CASES["groupby_apply-res-host_table"] = lambda e: e.ctx.groupby_apply(e.dA, e.GROUP, e.TAB, "mul")
CASES["groupby_apply-up-resident_table-out"] = lambda e: e.ctx.groupby_apply(e.A, e.GROUP, e.dTAB, "add", out=e.out(T, CELLS))
CASES["quantile-res-out"] = lambda e: e.ctx.quantile(e.dA, [0.1, 0.9], e.GROUP, G, out=e.out(2 * G, CELLS))
CASES["rolling-res-t0-n_out-out"] = lambda e: e.ctx.rolling(e.dA, 5, "var", t0=3, n_out=7, out=e.out(7, CELLS))

# ---- the paired calls: name -> (what follows the two fields, the number of statistics) ----
PAIRED = {
    "skill": (lambda e: (e.OFFSETS, ["bias", "corr"]), 2),
    "skill_groups": (lambda e: (e.GROUP, G, "rmse"), 1),
    "twosample": (lambda e: (e.OFFSETS, "ks"), 1),
    "twosample_groups": (lambda e: (e.GROUP, G, ["ks", "nb"]), 2),
}
PAIRS = {"f8-f8": ("A", "B"), "f4-f8": ("A32", "B"), "f8-f4": ("A", "B32"), "b_is_a": ("A", "A")}
for name, (rest, nstat) in PAIRED.items():
    for form in FORMS:
        for pair, (a, b) in PAIRS.items():
            CASES[f"{name}-{form}-{pair}"] = lambda e, name=name, rest=rest, form=form, a=a, b=b: e.call(form, name)(e.a(form, a), e.a(form, b), *rest(e))
    CASES[f"{name}-res-out"] = lambda e, name=name, rest=rest, nstat=nstat: getattr(e.ctx, name)(
        e.dA, e.dB32, *rest(e), out=e.out(nstat * (M if "groups" not in name else G), CELLS))
    CASES[f"{name}-planes"] = lambda e, name=name, rest=rest, nstat=nstat: getattr(e.ctx, name)(
        e.dA, e.dB, *rest(e), out=e.planes(nstat, M if "groups" not in name else G), plane_rows=PLANE_ROWS)
for form in FORMS:
    CASES[f"twosample-{form}-perkins"] = lambda e, form=form: e.call(form, "twosample")(e.a(form, "A"), e.a(form, "B"), e.OFFSETS, ["ks", "perkins", "na"],
                                                                                       0.5, 1.0)
    CASES[f"twosample-{form}-width_not_read"] = lambda e, form=form: e.call(form, "twosample")(e.a(form, "A"), e.a(form, "B"), e.OFFSETS, "ks", 0.5, 1.0)
    CASES[f"twosample_groups-{form}-perkins"] = lambda e, form=form: e.call(form, "twosample_groups")(e.a(form, "A"), e.a(form, "B"), e.GROUP, G, "perkins",
                                                                                                     width=2, origin=-1)
    CASES[f"twosample_groups-{form}-width_not_read"] = lambda e, form=form: e.call(form, "twosample_groups")(e.a(form, "A"), e.a(form, "B"), e.GROUP, G,
                                                                                                            ["na", "nb"], width=2, origin=-1)

# ---- the analog library: resident only ----
CASES["ca_apply-F"] = lambda e: e.ctx.ca_apply(e.dF, e.dIDX, e.dWEIGHTS)
CASES["ca_apply-F32-rows-out"] = lambda e: e.ctx.ca_apply(e.dF32, e.dIDX, e.dWEIGHTS, 1, 3, out=e.out(2, CELLS))
CASES["ca_local_apply-none"] = lambda e: e.ctx.ca_local_apply(e.dF32, e.dCELL_OF, e.dLOCAL, e.dL, e.dQ)
CASES["ca_local_apply-none-no_L_Q"] = lambda e: e.ctx.ca_local_apply(e.dF, e.dCELL_OF, e.dLOCAL)
CASES["ca_local_apply-shift"] = lambda e: e.ctx.ca_local_apply(e.dF, e.dCELL_OF, e.dLOCAL, e.dL, e.dQ, "shift")
CASES["ca_local_apply-scale-rows-out"] = lambda e: e.ctx.ca_local_apply(e.dF32, e.dCELL_OF, e.dLOCAL, e.dL, e.dQ, "scale", 4.0, 1, 3, out=e.out(2, CELLS))

# ---- regridding and remapping ----
for f in ("SRC", "SRC32"):
    CASES[f"regrid_apply-up-{f}"] = lambda e, f=f: e.state("regrid").apply(getattr(e, f))
    CASES[f"regrid_apply-res-{f}"] = lambda e, f=f: e.state("regrid").apply(getattr(e, "dSRC_WHOLE" + f[3:]))
    CASES[f"regrid_apply_host-{f}"] = lambda e, f=f: e.state("regrid").apply_host(getattr(e, f))
    CASES[f"remap_apply-up-{f}"] = lambda e, f=f: e.state("remap").apply(getattr(e, f))
    CASES[f"remap_apply_host-{f}"] = lambda e, f=f: e.state("remap").apply_host(getattr(e, f), 0.25)
CASES["regrid_apply-res-out"] = lambda e: e.state("regrid").apply(e.dSRC_WHOLE, out=e.out(TQ, 30))
CASES["regrid_apply-up-out"] = lambda e: e.state("regrid").apply(e.SRC, out=e.out(TQ, 30))
CASES["remap_apply-up-flat"] = lambda e: e.state("remap").apply(e.FINE32, 0.25)
CASES["remap_apply-res"] = lambda e: e.state("remap").apply(e.dFINE)
CASES["remap_apply-res-F32-out"] = lambda e: e.state("remap").apply(e.dFINE32, 1, out=e.out(TQ, 4))
CASES["remap_apply_host-flat"] = lambda e: e.state("remap").apply_host(e.FINE)

CALLS = {'ca_apply-F': [('sd_ca_apply_dev', ['ctx', ('dF', 2), 0, 12, 6, 8, ('dIDX', 0), ('dWEIGHTS', 0), 4, 3, 0, 4, ('block0', 0), 8])],
 'ca_apply-F32-rows-out': [('sd_ca_apply_dev', ['ctx', ('dF32', 2), 1, 12, 6, 8, ('dIDX', 0), ('dWEIGHTS', 0), 4, 3, 1, 3, ('dOUT', 2), 12])],
 'ca_local-res': [('sd_ca_local_dev',
                   ['ctx', ('dL', 2), 12, 6, ('dQ', 2), 12, 4, 2, 4, ('WC', 0), 3, 1, 2, ('dIDX', 0), ('block0', 0), ('block1', 0)])],
 'ca_local-up': [('sd_ca_local_dev',
                  ['ctx', ('block0', 0), 8, 6, ('block1', 0), 8, 4, 2, 4, ('WC', 0), 3, 1, 2, ('dIDX', 0), ('block2', 0), ('block3', 0)])],
 'ca_local_apply-none': [('sd_ca_local_apply_dev',
                          ['ctx', ('dF32', 2), 1, 12, 6, 8, ('dCELL_OF', 0), ('dLOCAL', 0), 8, None, 0, None, 0, 0, 0.0, 4, 0, 4, ('block0', 0), 8])],
 'ca_local_apply-none-no_L_Q': [('sd_ca_local_apply_dev',
                                 ['ctx', ('dF', 2), 0, 12, 6, 8, ('dCELL_OF', 0), ('dLOCAL', 0), 8, None, 0, None, 0, 0, 0.0, 4, 0, 4, ('block0', 0),
                                  8])],
 'ca_local_apply-scale-rows-out': [('sd_ca_local_apply_dev',
                                    ['ctx', ('dF32', 2), 1, 12, 6, 8, ('dCELL_OF', 0), ('dLOCAL', 0), 8, ('dL', 2), 12, ('dQ', 2), 12, 2, 4.0, 4, 1,
                                     3, ('dOUT', 2), 12])],
 'ca_local_apply-shift': [('sd_ca_local_apply_dev',
                           ['ctx', ('dF', 2), 0, 12, 6, 8, ('dCELL_OF', 0), ('dLOCAL', 0), 8, ('dL', 2), 12, ('dQ', 2), 12, 1, 0.0, 4, 0, 4,
                            ('block0', 0), 8])],
 'ca_select-res-keys': [('sd_ca_select_dev',
                         ['ctx', ('dL', 2), 12, 6, ('dQ', 2), 12, 4, 8, ('WC', 0), 3, ('KEY_L', 0), ('KEY_Q', 0), 4, 1, ('EXCL_L', 0), ('EXCL_Q', 0),
                          ('block0', 0), ('block1', 0), ('block2', 0)])],
 'ca_select-res-plain': [('sd_ca_select_dev',
                          ['ctx', ('dL', 2), 12, 6, ('dQ', 2), 12, 4, 8, ('WC', 0), 3, 'mem', 'mem', 1, -1, 'mem', 'mem', ('block0', 0),
                           ('block1', 0), ('block2', 0)])],
 'ca_select-up-keys': [('sd_ca_select_dev',
                        ['ctx', ('block0', 0), 8, 6, ('block1', 0), 8, 4, 8, ('WC', 0), 3, ('KEY_L', 0), ('KEY_Q', 0), 4, 1, ('EXCL_L', 0),
                         ('EXCL_Q', 0), ('block2', 0), ('block3', 0), ('block4', 0)])],
 'ca_select-up-plain': [('sd_ca_select_dev',
                         ['ctx', ('block0', 0), 8, 6, ('block1', 0), 8, 4, 8, ('WC', 0), 3, 'mem', 'mem', 1, -1, 'mem', 'mem', ('block2', 0),
                          ('block3', 0), ('block4', 0)])],
 'ca_weights-res-mean': [('sd_ca_weights_dev',
                          ['ctx', ('dL', 2), 12, 6, ('dQ', 2), 12, 4, 8, ('WC', 0), 3, 1, 0.0, ('dIDX', 0), ('dDIST', 0), ('block0', 0),
                           ('dSTATUS', 0)])],
 'ca_weights-res-regression': [('sd_ca_weights_dev',
                                ['ctx', ('dL', 2), 12, 6, ('dQ', 2), 12, 4, 8, ('WC', 0), 3, 0, 1e-06, ('dIDX', 0), ('dDIST', 0), ('block0', 0),
                                 ('dSTATUS', 0)])],
 'ca_weights-up-mean': [('sd_ca_weights_dev',
                         ['ctx', ('block0', 0), 8, 6, ('block1', 0), 8, 4, 8, ('WC', 0), 3, 1, 0.0, ('dIDX', 0), ('dDIST', 0), ('block2', 0),
                          ('dSTATUS', 0)])],
 'ca_weights-up-regression': [('sd_ca_weights_dev',
                               ['ctx', ('block0', 0), 8, 6, ('block1', 0), 8, 4, 8, ('WC', 0), 3, 0, 1e-06, ('dIDX', 0), ('dDIST', 0), ('block2', 0),
                                ('dSTATUS', 0)])],
 'disaggregate-host-climo': [('sd_disagg',
                              ['ctx', 2, ('TARGET', 0), ('A', 0), 0, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, ('TAB', 0), 3, ('BIN_GROUP', 0),
                               'mem'])],
 'disaggregate-host-plain': [('sd_disagg',
                              ['ctx', 0, ('TARGET', 0), ('A32', 0), 1, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, None, 0, None, 'mem'])],
 'disaggregate-res-climo': [('sd_disagg_dev',
                             ['ctx', 2, ('dTARGET', 2), 12, ('dA', 2), 0, 12, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, ('dTAB', 2), 12, 3,
                              ('BIN_GROUP', 0), ('block0', 0), 8])],
 'disaggregate-res-out': [('sd_disagg_dev',
                           ['ctx', 1, ('dTARGET', 2), 12, ('dA', 2), 0, 12, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, None, 0, 0, None,
                            ('dOUT', 2), 12])],
 'disaggregate-res-plain': [('sd_disagg_dev',
                             ['ctx', 0, ('dTARGET', 2), 12, ('dA32', 2), 1, 12, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, None, 0, 0, None,
                              ('block0', 0), 8])],
 'disaggregate-resident_target-host_obs': [('sd_disagg_dev',
                                            ['ctx', 0, ('dTARGET', 2), 12, ('block1', 0), 0, 8, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, None, 0,
                                             0, None, ('block0', 0), 8])],
 'disaggregate-up-climo': [('sd_disagg_dev',
                            ['ctx', 2, ('block1', 0), 8, ('block2', 0), 0, 8, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, ('block3', 0), 8, 3,
                             ('BIN_GROUP', 0), ('block0', 0), 8])],
 'disaggregate-up-plain': [('sd_disagg_dev',
                            ['ctx', 0, ('block1', 0), 8, ('block2', 0), 1, 8, 24, 8, ('SRC_ROW', 0), 24, ('OFFSETS', 0), 2, None, 0, 0, None,
                             ('block0', 0), 8])],
 'groupby_apply-host-A': [('sd_groupby_apply', ['ctx', 0, ('A', 0), 0, 24, 8, ('GROUP', 0), 3, ('TAB', 0), 'mem'])],
 'groupby_apply-host-A32': [('sd_groupby_apply', ['ctx', 3, ('A32', 0), 1, 24, 8, ('GROUP', 0), 3, ('TAB', 0), 'mem'])],
 'groupby_apply-res-A': [('sd_groupby_apply_dev', ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, ('dTAB', 2), 12, ('block0', 0), 8])],
 'groupby_apply-res-A32': [('sd_groupby_apply_dev', ['ctx', 3, ('dA32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, ('dTAB', 2), 12, ('block0', 0), 8])],
 'groupby_apply-res-host_table': [('sd_groupby_apply_dev', ['ctx', 2, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, ('block1', 0), 8, ('block0', 0), 8])],
 'groupby_apply-up-A': [('sd_groupby_apply_dev', ['ctx', 0, ('block1', 0), 0, 8, 24, 8, ('GROUP', 0), 3, ('block2', 0), 8, ('block0', 0), 8])],
 'groupby_apply-up-A32': [('sd_groupby_apply_dev', ['ctx', 3, ('block1', 0), 1, 8, 24, 8, ('GROUP', 0), 3, ('block2', 0), 8, ('block0', 0), 8])],
 'groupby_apply-up-resident_table-out': [('sd_groupby_apply_dev',
                                          ['ctx', 1, ('block0', 0), 0, 8, 24, 8, ('GROUP', 0), 3, ('dTAB', 2), 12, ('dOUT', 2), 12])],
 'groupby_reduce-host-A': [('sd_groupby_reduce', ['ctx', 0, ('A', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem'])],
 'groupby_reduce-host-A32': [('sd_groupby_reduce', ['ctx', 1, ('A32', 0), 1, 24, 8, ('GROUP', 0), 3, 'mem'])],
 'groupby_reduce-res-A': [('sd_groupby_reduce_dev',
                           ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, ('block0', 0), ('block1', 0), 8, 0, ('block2', 0), 8])],
 'groupby_reduce-res-A32': [('sd_groupby_reduce_dev',
                             ['ctx', 1, ('dA32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, ('block0', 0), ('block1', 0), 8, 0, ('block2', 0), 8])],
 'groupby_reduce-res-carry-out': [('sd_groupby_reduce_dev',
                                   ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, ('dSUM', 2), ('dCOUNT', 2), 12, 1, ('dOUT', 2), 12])],
 'groupby_reduce-res-no_finish': [('sd_groupby_reduce_dev',
                                   ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, ('block0', 0), ('block1', 0), 8, 0, None, 0])],
 'groupby_reduce-up-A': [('sd_groupby_reduce_dev',
                          ['ctx', 0, ('block3', 0), 0, 8, 24, 8, ('GROUP', 0), 3, ('block0', 0), ('block1', 0), 8, 0, ('block2', 0), 8])],
 'groupby_reduce-up-A32': [('sd_groupby_reduce_dev',
                            ['ctx', 1, ('block3', 0), 1, 8, 24, 8, ('GROUP', 0), 3, ('block0', 0), ('block1', 0), 8, 0, ('block2', 0), 8])],
 'groupby_reduce-up-carry-no_finish': [('sd_groupby_reduce_dev',
                                        ['ctx', 1, ('block0', 0), 1, 8, 24, 8, ('GROUP', 0), 3, ('dSUM', 2), ('dCOUNT', 2), 12, 1, None, 0])],
 'quantile-host-group-G': [('sd_quantile', ['ctx', 3, 0, ('A', 0), 0, 24, 8, ('GROUP', 0), 4, 'mem', 2, 'mem'])],
 'quantile-host-group-G_None': [('sd_quantile', ['ctx', 0, 1, ('A32', 0), 1, 24, 8, ('GROUP', 0), 3, 'mem', 1, 'mem'])],
 'quantile-host-median': [('sd_quantile', ['ctx', 5, 1, ('A', 0), 0, 24, 8, None, 1, 'mem', 1, 'mem'])],
 'quantile-host-no_group': [('sd_quantile', ['ctx', 0, 1, ('A', 0), 0, 24, 8, None, 1, 'mem', 2, 'mem'])],
 'quantile-res-group-G': [('sd_quantile_dev', ['ctx', 3, 0, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 4, 'mem', 2, ('block0', 0), 8])],
 'quantile-res-group-G_None': [('sd_quantile_dev', ['ctx', 0, 1, ('dA32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8])],
 'quantile-res-median': [('sd_quantile_dev', ['ctx', 5, 1, ('dA', 2), 0, 12, 24, 8, None, 1, 'mem', 1, ('block0', 0), 8])],
 'quantile-res-no_group': [('sd_quantile_dev', ['ctx', 0, 1, ('dA', 2), 0, 12, 24, 8, None, 1, 'mem', 2, ('block0', 0), 8])],
 'quantile-res-out': [('sd_quantile_dev', ['ctx', 0, 1, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, ('dOUT', 2), 12])],
 'quantile-up-group-G': [('sd_quantile_dev', ['ctx', 3, 0, ('block1', 0), 0, 8, 24, 8, ('GROUP', 0), 4, 'mem', 2, ('block0', 0), 8])],
 'quantile-up-group-G_None': [('sd_quantile_dev', ['ctx', 0, 1, ('block1', 0), 1, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8])],
 'quantile-up-median': [('sd_quantile_dev', ['ctx', 5, 1, ('block1', 0), 0, 8, 24, 8, None, 1, 'mem', 1, ('block0', 0), 8])],
 'quantile-up-no_group': [('sd_quantile_dev', ['ctx', 0, 1, ('block1', 0), 0, 8, 24, 8, None, 1, 'mem', 2, ('block0', 0), 8])],
 'regrid_apply-res-SRC': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                          ('sd_regrid_apply_dev', ['ctx', 'state0', ('dSRC_WHOLE', 0), 0, 4, ('block0', 0), 30])],
 'regrid_apply-res-SRC32': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                            ('sd_regrid_apply_dev', ['ctx', 'state0', ('dSRC_WHOLE32', 0), 1, 4, ('block0', 0), 30])],
 'regrid_apply-res-out': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                          ('sd_regrid_apply_dev', ['ctx', 'state0', ('dSRC_WHOLE', 0), 0, 4, ('dOUT', 2), 34])],
 'regrid_apply-up-SRC': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                         ('sd_regrid_apply_dev', ['ctx', 'state0', ('block0', 0), 0, 4, ('block1', 0), 30])],
 'regrid_apply-up-SRC32': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                           ('sd_regrid_apply_dev', ['ctx', 'state0', ('block0', 0), 1, 4, ('block1', 0), 30])],
 'regrid_apply-up-out': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                         ('sd_regrid_apply_dev', ['ctx', 'state0', ('block0', 0), 0, 4, ('dOUT', 2), 34])],
 'regrid_apply_host-SRC': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']), ('sd_regrid_apply', ['ctx', 'state0', ('SRC', 0), 0, 4, 'mem'])],
 'regrid_apply_host-SRC32': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&']),
                             ('sd_regrid_apply', ['ctx', 'state0', ('SRC32', 0), 1, 4, 'mem'])],
 'remap_apply-res': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                     ('sd_remap_apply_dev', ['ctx', 'state0', ('dFINE', 2), 0, 16, 4, 0.5, ('block0', 0), 4])],
 'remap_apply-res-F32-out': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                             ('sd_remap_apply_dev', ['ctx', 'state0', ('dFINE32', 2), 1, 16, 4, 1.0, ('dOUT', 2), 8])],
 'remap_apply-up-SRC': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                        ('sd_remap_apply_dev', ['ctx', 'state0', ('block0', 0), 0, 12, 4, 0.5, ('block1', 0), 4])],
 'remap_apply-up-SRC32': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                          ('sd_remap_apply_dev', ['ctx', 'state0', ('block0', 0), 1, 12, 4, 0.5, ('block1', 0), 4])],
 'remap_apply-up-flat': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                         ('sd_remap_apply_dev', ['ctx', 'state0', ('block0', 0), 1, 12, 4, 0.25, ('block1', 0), 4])],
 'remap_apply_host-SRC': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                          ('sd_remap_apply', ['ctx', 'state0', ('SRC', 0), 0, 4, 0.25, 'mem'])],
 'remap_apply_host-SRC32': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                            ('sd_remap_apply', ['ctx', 'state0', ('SRC32', 0), 1, 4, 0.25, 'mem'])],
 'remap_apply_host-flat': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&']),
                           ('sd_remap_apply', ['ctx', 'state0', ('FINE', 0), 0, 4, 0.5, 'mem'])],
 'resample-host-A': [('sd_resample', ['ctx', 0, ('A', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem'])],
 'resample-host-A32': [('sd_resample', ['ctx', 1, ('A32', 0), 1, 24, 8, ('OFFSETS', 0), 2, 'mem'])],
 'resample-res-A': [('sd_resample_dev', ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, ('block0', 0), 8])],
 'resample-res-A32': [('sd_resample_dev', ['ctx', 1, ('dA32', 2), 1, 12, 24, 8, ('OFFSETS', 0), 2, ('block0', 0), 8])],
 'resample-res-out': [('sd_resample_dev', ['ctx', 0, ('dA', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, ('dOUT', 2), 12])],
 'resample-up-A': [('sd_resample_dev', ['ctx', 0, ('block1', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, ('block0', 0), 8])],
 'resample-up-A32': [('sd_resample_dev', ['ctx', 1, ('block1', 0), 1, 8, 24, 8, ('OFFSETS', 0), 2, ('block0', 0), 8])],
 'rolling-host-defaults': [('sd_rolling', ['ctx', 0, ('A', 0), 0, 24, 8, 5, 4, 5, 1, 0, 'mem'])],
 'rolling-host-options': [('sd_rolling', ['ctx', 3, ('A32', 0), 1, 24, 8, 5, 2, 3, 0, 1, 'mem'])],
 'rolling-res-defaults': [('sd_rolling_dev', ['ctx', 0, ('dA', 2), 0, 12, 24, 8, 5, 4, 5, 1, 0, 0, 24, ('block0', 0), 8])],
 'rolling-res-options': [('sd_rolling_dev', ['ctx', 3, ('dA32', 2), 1, 12, 24, 8, 5, 2, 3, 0, 1, 0, 24, ('block0', 0), 8])],
 'rolling-res-t0-n_out': [('sd_rolling_dev', ['ctx', 0, ('dA', 2), 0, 12, 24, 8, 5, 4, 5, 1, 0, 3, 7, ('block0', 0), 8])],
 'rolling-res-t0-n_out-out': [('sd_rolling_dev', ['ctx', 2, ('dA', 2), 0, 12, 24, 8, 5, 4, 5, 1, 0, 3, 7, ('dOUT', 2), 12])],
 'rolling-up-defaults': [('sd_rolling_dev', ['ctx', 0, ('block1', 0), 0, 8, 24, 8, 5, 4, 5, 1, 0, 0, 24, ('block0', 0), 8])],
 'rolling-up-options': [('sd_rolling_dev', ['ctx', 3, ('block1', 0), 1, 8, 24, 8, 5, 2, 3, 0, 1, 0, 24, ('block0', 0), 8])],
 'rolling-up-t0-n_out': [('sd_rolling_dev', ['ctx', 0, ('block1', 0), 0, 8, 24, 8, 5, 4, 5, 1, 0, 3, 7, ('block0', 0), 8])],
 'skill-host-b_is_a': [('sd_skill', ['ctx', ('A', 0), 0, ('A', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, 'mem'])],
 'skill-host-f4-f8': [('sd_skill', ['ctx', ('A32', 0), 1, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, 'mem'])],
 'skill-host-f8-f4': [('sd_skill', ['ctx', ('A', 0), 0, ('B32', 0), 1, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, 'mem'])],
 'skill-host-f8-f8': [('sd_skill', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, 'mem'])],
 'skill-planes': [('sd_skill_dev', ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('dPLANES', 14), 12, 60])],
 'skill-res-b_is_a': [('sd_skill_dev', ['ctx', ('dA', 2), 0, 12, ('dA', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-res-f4-f8': [('sd_skill_dev', ['ctx', ('dA32', 2), 1, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-res-f8-f4': [('sd_skill_dev', ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-res-f8-f8': [('sd_skill_dev', ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-res-out': [('sd_skill_dev', ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('dOUT', 2), 12, 24])],
 'skill-up-b_is_a': [('sd_skill_dev', ['ctx', ('block1', 0), 0, 8, ('block1', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-up-f4-f8': [('sd_skill_dev', ['ctx', ('block1', 0), 1, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-up-f8-f4': [('sd_skill_dev', ['ctx', ('block1', 0), 0, 8, ('block2', 0), 1, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill-up-f8-f8': [('sd_skill_dev', ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 2, ('block0', 0), 8, 16])],
 'skill_groups-host-b_is_a': [('sd_skill_groups', ['ctx', ('A', 0), 0, ('A', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 1, 'mem'])],
 'skill_groups-host-f4-f8': [('sd_skill_groups', ['ctx', ('A32', 0), 1, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 1, 'mem'])],
 'skill_groups-host-f8-f4': [('sd_skill_groups', ['ctx', ('A', 0), 0, ('B32', 0), 1, 24, 8, ('GROUP', 0), 3, 'mem', 1, 'mem'])],
 'skill_groups-host-f8-f8': [('sd_skill_groups', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 1, 'mem'])],
 'skill_groups-planes': [('sd_skill_groups_dev',
                          ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('dPLANES', 14), 12, 60])],
 'skill_groups-res-b_is_a': [('sd_skill_groups_dev',
                              ['ctx', ('dA', 2), 0, 12, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-res-f4-f8': [('sd_skill_groups_dev',
                             ['ctx', ('dA32', 2), 1, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-res-f8-f4': [('sd_skill_groups_dev',
                             ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-res-f8-f8': [('sd_skill_groups_dev',
                             ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-res-out': [('sd_skill_groups_dev',
                           ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('dOUT', 2), 12, 36])],
 'skill_groups-up-b_is_a': [('sd_skill_groups_dev',
                             ['ctx', ('block1', 0), 0, 8, ('block1', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-up-f4-f8': [('sd_skill_groups_dev',
                            ['ctx', ('block1', 0), 1, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-up-f8-f4': [('sd_skill_groups_dev',
                            ['ctx', ('block1', 0), 0, 8, ('block2', 0), 1, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'skill_groups-up-f8-f8': [('sd_skill_groups_dev',
                            ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, ('block0', 0), 8, 24])],
 'spells-host-host_table': [('sd_spells', ['ctx', ('A32', 0), 1, 24, 8, 3, 0.0, ('TAB1', 0), None, 1, ('OFFSETS', 0), 2, 1, 'mem', 2, 'mem'])],
 'spells-host-host_table-group': [('sd_spells',
                                   ['ctx', ('A', 0), 0, 24, 8, 1, 0.0, ('TAB', 0), ('GROUP', 0), 3, ('OFFSETS', 0), 2, 1, 'mem', 2, 'mem'])],
 'spells-host-scalar': [('sd_spells', ['ctx', ('A', 0), 0, 24, 8, 0, 1.5, None, None, 1, ('OFFSETS', 0), 2, 2, 'mem', 1, 'mem'])],
 'spells-planes': [('sd_spells_dev',
                    ['ctx', ('dA', 2), 0, 12, 24, 8, 0, 0.0, None, 0, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 2, ('dPLANES', 14), 12, 60])],
 'spells-res-host_table': [('sd_spells_dev',
                            ['ctx', ('dA32', 2), 1, 12, 24, 8, 3, 0.0, ('block1', 0), 8, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 2, ('block0', 0), 8,
                             16])],
 'spells-res-host_table-group': [('sd_spells_dev',
                                  ['ctx', ('dA', 2), 0, 12, 24, 8, 1, 0.0, ('block1', 0), 8, ('GROUP', 0), 3, ('OFFSETS', 0), 2, 1, 'mem', 2,
                                   ('block0', 0), 8, 16])],
 'spells-res-out': [('sd_spells_dev',
                     ['ctx', ('dA', 2), 0, 12, 24, 8, 0, 0.0, None, 0, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 2, ('dOUT', 2), 12, 24])],
 'spells-res-resident_table': [('sd_spells_dev',
                                ['ctx', ('dA', 2), 0, 12, 24, 8, 2, 0.0, ('dTAB1', 2), 12, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 1, ('block0', 0), 8,
                                 16])],
 'spells-res-resident_table-group': [('sd_spells_dev',
                                      ['ctx', ('dA', 2), 0, 12, 24, 8, 2, 0.0, ('dTAB', 2), 12, ('GROUP', 0), 3, ('OFFSETS', 0), 2, 1, 'mem', 2,
                                       ('block0', 0), 8, 16])],
 'spells-res-scalar': [('sd_spells_dev',
                        ['ctx', ('dA', 2), 0, 12, 24, 8, 0, 1.5, None, 0, None, 1, ('OFFSETS', 0), 2, 2, 'mem', 1, ('block0', 0), 8, 16])],
 'spells-up-host_table': [('sd_spells_dev',
                           ['ctx', ('block1', 0), 1, 8, 24, 8, 3, 0.0, ('block2', 0), 8, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 2, ('block0', 0), 8,
                            16])],
 'spells-up-host_table-group': [('sd_spells_dev',
                                 ['ctx', ('block1', 0), 0, 8, 24, 8, 1, 0.0, ('block2', 0), 8, ('GROUP', 0), 3, ('OFFSETS', 0), 2, 1, 'mem', 2,
                                  ('block0', 0), 8, 16])],
 'spells-up-resident_table': [('sd_spells_dev',
                               ['ctx', ('block1', 0), 0, 8, 24, 8, 2, 0.0, ('dTAB1', 2), 12, None, 1, ('OFFSETS', 0), 2, 1, 'mem', 1, ('block0', 0),
                                8, 16])],
 'spells-up-resident_table-group': [('sd_spells_dev',
                                     ['ctx', ('block1', 0), 0, 8, 24, 8, 2, 0.0, ('dTAB', 2), 12, ('GROUP', 0), 3, ('OFFSETS', 0), 2, 1, 'mem', 2,
                                      ('block0', 0), 8, 16])],
 'spells-up-scalar': [('sd_spells_dev',
                       ['ctx', ('block1', 0), 0, 8, 24, 8, 0, 1.5, None, 0, None, 1, ('OFFSETS', 0), 2, 2, 'mem', 1, ('block0', 0), 8, 16])],
 'twosample-host-b_is_a': [('sd_twosample', ['ctx', ('A', 0), 0, ('A', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, 'mem'])],
 'twosample-host-f4-f8': [('sd_twosample', ['ctx', ('A32', 0), 1, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, 'mem'])],
 'twosample-host-f8-f4': [('sd_twosample', ['ctx', ('A', 0), 0, ('B32', 0), 1, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, 'mem'])],
 'twosample-host-f8-f8': [('sd_twosample', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, 'mem'])],
 'twosample-host-perkins': [('sd_twosample', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 3, 0.5, 1.0, 'mem'])],
 'twosample-host-width_not_read': [('sd_twosample', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, 'mem'])],
 'twosample-planes': [('sd_twosample_dev',
                       ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('dPLANES', 14), 12, 60])],
 'twosample-res-b_is_a': [('sd_twosample_dev',
                           ['ctx', ('dA', 2), 0, 12, ('dA', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-res-f4-f8': [('sd_twosample_dev',
                          ['ctx', ('dA32', 2), 1, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-res-f8-f4': [('sd_twosample_dev',
                          ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-res-f8-f8': [('sd_twosample_dev',
                          ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-res-out': [('sd_twosample_dev',
                        ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('dOUT', 2), 12, 24])],
 'twosample-res-perkins': [('sd_twosample_dev',
                            ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 3, 0.5, 1.0, ('block0', 0), 8, 16])],
 'twosample-res-width_not_read': [('sd_twosample_dev',
                                   ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-up-b_is_a': [('sd_twosample_dev',
                          ['ctx', ('block1', 0), 0, 8, ('block1', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-up-f4-f8': [('sd_twosample_dev',
                         ['ctx', ('block1', 0), 1, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-up-f8-f4': [('sd_twosample_dev',
                         ['ctx', ('block1', 0), 0, 8, ('block2', 0), 1, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-up-f8-f8': [('sd_twosample_dev',
                         ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8, 16])],
 'twosample-up-perkins': [('sd_twosample_dev',
                           ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 3, 0.5, 1.0, ('block0', 0), 8, 16])],
 'twosample-up-width_not_read': [('sd_twosample_dev',
                                  ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('OFFSETS', 0), 2, 'mem', 1, 0.0, 0.0, ('block0', 0), 8,
                                   16])],
 'twosample_groups-host-b_is_a': [('sd_twosample_groups', ['ctx', ('A', 0), 0, ('A', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, 'mem'])],
 'twosample_groups-host-f4-f8': [('sd_twosample_groups', ['ctx', ('A32', 0), 1, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, 'mem'])],
 'twosample_groups-host-f8-f4': [('sd_twosample_groups', ['ctx', ('A', 0), 0, ('B32', 0), 1, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, 'mem'])],
 'twosample_groups-host-f8-f8': [('sd_twosample_groups', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, 'mem'])],
 'twosample_groups-host-perkins': [('sd_twosample_groups', ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 1, 2.0, -1.0, 'mem'])],
 'twosample_groups-host-width_not_read': [('sd_twosample_groups',
                                           ['ctx', ('A', 0), 0, ('B', 0), 0, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, 'mem'])],
 'twosample_groups-planes': [('sd_twosample_groups_dev',
                              ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('dPLANES', 14), 12, 60])],
 'twosample_groups-res-b_is_a': [('sd_twosample_groups_dev',
                                  ['ctx', ('dA', 2), 0, 12, ('dA', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-res-f4-f8': [('sd_twosample_groups_dev',
                                 ['ctx', ('dA32', 2), 1, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-res-f8-f4': [('sd_twosample_groups_dev',
                                 ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-res-f8-f8': [('sd_twosample_groups_dev',
                                 ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-res-out': [('sd_twosample_groups_dev',
                               ['ctx', ('dA', 2), 0, 12, ('dB32', 2), 1, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('dOUT', 2), 12, 36])],
 'twosample_groups-res-perkins': [('sd_twosample_groups_dev',
                                   ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 1, 2.0, -1.0, ('block0', 0), 8, 24])],
 'twosample_groups-res-width_not_read': [('sd_twosample_groups_dev',
                                          ['ctx', ('dA', 2), 0, 12, ('dB', 2), 0, 12, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8,
                                           24])],
 'twosample_groups-up-b_is_a': [('sd_twosample_groups_dev',
                                 ['ctx', ('block1', 0), 0, 8, ('block1', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8,
                                  24])],
 'twosample_groups-up-f4-f8': [('sd_twosample_groups_dev',
                                ['ctx', ('block1', 0), 1, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-up-f8-f4': [('sd_twosample_groups_dev',
                                ['ctx', ('block1', 0), 0, 8, ('block2', 0), 1, 8, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-up-f8-f8': [('sd_twosample_groups_dev',
                                ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0), 8, 24])],
 'twosample_groups-up-perkins': [('sd_twosample_groups_dev',
                                  ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 1, 2.0, -1.0, ('block0', 0), 8,
                                   24])],
 'twosample_groups-up-width_not_read': [('sd_twosample_groups_dev',
                                         ['ctx', ('block1', 0), 0, 8, ('block2', 0), 0, 8, 24, 8, ('GROUP', 0), 3, 'mem', 2, 0.0, 0.0, ('block0', 0),
                                          8, 24])]}
TRAFFIC = {'ca_apply-F': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'ca_local-res': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 256, '&'])],
 'ca_local-up': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]), ('sd_dev_alloc', ['ctx', 256, '&']),
                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]), ('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 256, '&']),
                 ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_local_apply-none': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'ca_local_apply-none-no_L_Q': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'ca_local_apply-shift': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'ca_select-res-keys': [('sd_dev_alloc', ['ctx', 48, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 16, '&'])],
 'ca_select-res-plain': [('sd_dev_alloc', ['ctx', 48, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 16, '&'])],
 'ca_select-up-keys': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                       ('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]),
                       ('sd_dev_alloc', ['ctx', 48, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 16, '&']),
                       ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_select-up-plain': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                        ('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]),
                        ('sd_dev_alloc', ['ctx', 48, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 16, '&']),
                        ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_weights-res-mean': [('sd_dev_alloc', ['ctx', 96, '&'])],
 'ca_weights-res-regression': [('sd_dev_alloc', ['ctx', 96, '&'])],
 'ca_weights-up-mean': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                        ('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]),
                        ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_weights-up-regression': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                              ('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]),
                              ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'disaggregate-res-climo': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'disaggregate-res-plain': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'disaggregate-resident_target-host_obs': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'disaggregate-up-climo': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 128, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TARGET', 0), 128]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 192, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block3', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                           ('sd_dev_free', ['ctx', ('block2', 0)]), ('sd_dev_free', ['ctx', ('block3', 0)])],
 'disaggregate-up-plain': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 128, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TARGET', 0), 128]), ('sd_dev_alloc', ['ctx', 768, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('A32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                           ('sd_dev_free', ['ctx', ('block2', 0)])],
 'groupby_apply-res-A': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'groupby_apply-res-A32': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'groupby_apply-res-host_table': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 192, '&']),
                                  ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'groupby_apply-up-A': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 192, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                        ('sd_dev_free', ['ctx', ('block2', 0)])],
 'groupby_apply-up-A32': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 192, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                          ('sd_dev_free', ['ctx', ('block2', 0)])],
 'groupby_apply-up-resident_table-out': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                                         ('sd_dev_free', ['ctx', ('block0', 0)])],
 'groupby_reduce-res-A': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 192, '&'])],
 'groupby_reduce-res-A32': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 192, '&'])],
 'groupby_reduce-res-no_finish': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&'])],
 'groupby_reduce-up-A': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 192, '&']),
                         ('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block3', 0), ('A', 0), 1536]),
                         ('sd_dev_free', ['ctx', ('block3', 0)])],
 'groupby_reduce-up-A32': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_alloc', ['ctx', 192, '&']),
                           ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block3', 0), ('A32', 0), 768]),
                           ('sd_dev_free', ['ctx', ('block3', 0)])],
 'groupby_reduce-up-carry-no_finish': [('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A32', 0), 768]),
                                       ('sd_dev_free', ['ctx', ('block0', 0)])],
 'quantile-res-group-G': [('sd_dev_alloc', ['ctx', 512, '&'])],
 'quantile-res-group-G_None': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'quantile-res-median': [('sd_dev_alloc', ['ctx', 64, '&'])],
 'quantile-res-no_group': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'quantile-up-group-G': [('sd_dev_alloc', ['ctx', 512, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                         ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'quantile-up-group-G_None': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                              ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'quantile-up-median': [('sd_dev_alloc', ['ctx', 64, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'quantile-up-no_group': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'regrid_apply-res-SRC': [('sd_dev_alloc', ['ctx', 960, '&'])],
 'regrid_apply-res-SRC32': [('sd_dev_alloc', ['ctx', 960, '&'])],
 'regrid_apply-up-SRC': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                         ('sd_dev_alloc', ['ctx', 960, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])],
 'regrid_apply-up-SRC32': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC32', 0), 192]),
                           ('sd_dev_alloc', ['ctx', 960, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])],
 'regrid_apply-up-out': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                         ('sd_dev_free', ['ctx', ('block0', 0)])],
 'remap_apply-res': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'remap_apply-up-SRC': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                        ('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])],
 'remap_apply-up-SRC32': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC32', 0), 192]),
                          ('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])],
 'remap_apply-up-flat': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('FINE32', 0), 192]),
                         ('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])],
 'resample-res-A': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'resample-res-A32': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'resample-up-A': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                   ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'resample-up-A32': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                     ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'rolling-res-defaults': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'rolling-res-options': [('sd_dev_alloc', ['ctx', 1536, '&'])],
 'rolling-res-t0-n_out': [('sd_dev_alloc', ['ctx', 448, '&'])],
 'rolling-up-defaults': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                         ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'rolling-up-options': [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'rolling-up-t0-n_out': [('sd_dev_alloc', ['ctx', 448, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                         ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'skill-res-b_is_a': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'skill-res-f4-f8': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'skill-res-f8-f4': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'skill-res-f8-f8': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'skill-up-b_is_a': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                     ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'skill-up-f4-f8': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                    ('sd_dev_free', ['ctx', ('block2', 0)])],
 'skill-up-f8-f4': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 768, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                    ('sd_dev_free', ['ctx', ('block2', 0)])],
 'skill-up-f8-f8': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                    ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                    ('sd_dev_free', ['ctx', ('block2', 0)])],
 'skill_groups-res-b_is_a': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'skill_groups-res-f4-f8': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'skill_groups-res-f8-f4': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'skill_groups-res-f8-f8': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'skill_groups-up-b_is_a': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                            ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'skill_groups-up-f4-f8': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                           ('sd_dev_free', ['ctx', ('block2', 0)])],
 'skill_groups-up-f8-f4': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 768, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                           ('sd_dev_free', ['ctx', ('block2', 0)])],
 'skill_groups-up-f8-f8': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                           ('sd_dev_free', ['ctx', ('block2', 0)])],
 'spells-res-host_table': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 64, '&']),
                           ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB1', 0), 64]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'spells-res-host_table-group': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 192, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'spells-res-resident_table': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'spells-res-resident_table-group': [('sd_dev_alloc', ['ctx', 256, '&'])],
 'spells-res-scalar': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'spells-up-host_table': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 64, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB1', 0), 64]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                          ('sd_dev_free', ['ctx', ('block2', 0)])],
 'spells-up-host_table-group': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 192, '&']),
                                ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                ('sd_dev_free', ['ctx', ('block2', 0)])],
 'spells-up-resident_table': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                              ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'spells-up-resident_table-group': [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                    ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'spells-up-scalar': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                      ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'twosample-res-b_is_a': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'twosample-res-f4-f8': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'twosample-res-f8-f4': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'twosample-res-f8-f8': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'twosample-res-perkins': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample-res-width_not_read': [('sd_dev_alloc', ['ctx', 128, '&'])],
 'twosample-up-b_is_a': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                         ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'twosample-up-f4-f8': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                        ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample-up-f8-f4': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 768, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                        ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample-up-f8-f8': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                        ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                        ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample-up-perkins': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                          ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample-up-width_not_read': [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                 ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample_groups-res-b_is_a': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample_groups-res-f4-f8': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample_groups-res-f8-f4': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample_groups-res-f8-f8': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample_groups-res-perkins': [('sd_dev_alloc', ['ctx', 192, '&'])],
 'twosample_groups-res-width_not_read': [('sd_dev_alloc', ['ctx', 384, '&'])],
 'twosample_groups-up-b_is_a': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'twosample_groups-up-f4-f8': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                               ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample_groups-up-f8-f4': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 768, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                               ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample_groups-up-f8-f8': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                               ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample_groups-up-perkins': [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                 ('sd_dev_free', ['ctx', ('block2', 0)])],
 'twosample_groups-up-width_not_read': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                        ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                        ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('B', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                        ('sd_dev_free', ['ctx', ('block2', 0)])]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls(name):
    e = Engine()
    kept = CASES[name](e)  # noqa: F841  (a result that goes away frees its block)
    assert e.lib.log == CALLS[name]
    assert e.lib.traffic == TRAFFIC.get(name, [])  # (not in TRAFFIC: nothing is allocated, copied or freed)


def test_b_is_a_is_one_upload():
    e = Engine()
    e.ctx.skill(e.A, e.A, e.OFFSETS, "bias")
    assert [name for name, _ in e.lib.traffic].count("sd_memcpy_h2d") == 1
    args = e.lib.log[-1][1]
    assert args[1] == args[4] == ("block1", 0)


def test_groupby_reduce_returns_the_carried_pair():
    e = Engine()
    out, (s, n) = e.ctx.groupby_reduce(e.dA, e.GROUP, G, acc=(e.dSUM, e.dCOUNT), finish=False)
    assert out is None and s is e.dSUM and n is e.dCOUNT


@pytest.mark.parametrize("name", ["resample-res-out", "spells-planes", "skill-res-out", "quantile-res-out", "ca_apply-F32-rows-out",
                                  "regrid_apply-res-out", "remap_apply-res-F32-out"])
def test_resident_out_is_returned(name):
    e = Engine()
    got = CASES[name](e)
    assert got.base is not None and got.ld == got.base.ld and got.ctx is e.ctx  # the caller's view, not a fresh array


# ---- the entry point fails: the fresh outputs and the uploads are freed, the exception propagates ----
FAILURES = {
    "ca_select": ("sd_ca_select_dev", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, K)),
    "ca_weights": ("sd_ca_weights_dev", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, e.dSTATUS)),
    "ca_local": ("sd_ca_local_dev", lambda e: e.ctx.ca_local(e.L, e.Q, e.WC, (NY, NX), (1, 2), e.dIDX)),
    "remap_apply": ("sd_remap_apply_dev", lambda e: e.state("remap").apply(e.SRC)),
    "rule_regrid_apply": ("sd_regrid_apply_dev", lambda e: e.state("regrid").apply(e.SRC)),
}
FAILED = {'ca_local': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]), ('sd_dev_alloc', ['ctx', 256, '&']),
              ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]), ('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 256, '&']),
              ('sd_dev_free', ['ctx', ('block2', 0)]), ('sd_dev_free', ['ctx', ('block3', 0)]), ('sd_dev_free', ['ctx', ('block0', 0)]),
              ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_select': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]), ('sd_dev_alloc', ['ctx', 256, '&']),
               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]), ('sd_dev_alloc', ['ctx', 48, '&']), ('sd_dev_alloc', ['ctx', 96, '&']),
               ('sd_dev_alloc', ['ctx', 16, '&']), ('sd_dev_free', ['ctx', ('block2', 0)]), ('sd_dev_free', ['ctx', ('block3', 0)]),
               ('sd_dev_free', ['ctx', ('block4', 0)]), ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'ca_weights': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]), ('sd_dev_alloc', ['ctx', 256, '&']),
                ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('Q', 0), 256]), ('sd_dev_alloc', ['ctx', 96, '&']), ('sd_dev_free', ['ctx', ('block2', 0)]),
                ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])],
 'remap_apply': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]), ('sd_dev_alloc', ['ctx', 128, '&']),
                 ('sd_dev_free', ['ctx', ('block0', 0)])],
 'rule_regrid_apply': [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                       ('sd_dev_alloc', ['ctx', 960, '&']), ('sd_dev_free', ['ctx', ('block0', 0)])]}


@pytest.mark.parametrize("name", sorted(FAILURES))
def test_failure_frees(name):
    entry, call = FAILURES[name]
    e = Engine(FailingLib(entry))
    with pytest.raises(Boom) as caught:  # noqa: F841  (held: what the frames of the traceback keep alive is not freed yet)
        call(e)
    assert [n for n, _ in e.lib.log if not n.endswith("_info")] == [entry]
    assert e.lib.traffic == FAILED[name]


# ---- refusals: (what is called, the words of the refusal); REACHED: what had reached the library by then, where anything had ----
REFUSALS = {}
ANOTHER = "sd_downscale: {}: `{}` belongs to another context"
PLANES_WORDS = r"out: expected the rows of 2 bins inside the first of 2 planes of {} rows of a DeviceArray"


def other(e):
    """an Engine of another context (nothing of it may get as far as the entry point)"""
    return Engine()


def refuse(name, words, call):
    assert name not in REFUSALS, name
    REFUSALS[name] = (call, words)


def i64(e, name, shape):
    return e.lib.resident(e.ctx, name, shape, np.int64)


EMPTY, NO_CELLS, CUBE = np.zeros((0, CELLS)), np.zeros((T, 0)), np.zeros((T, 2, CELLS))

# resample
refuse("resample-op", "resample reduction 'max': only 'mean' and 'sum' are implemented", lambda e: e.ctx.resample(e.A, e.OFFSETS, "max"))
refuse("resample-field", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\) of float64", lambda e: e.ctx.resample(CUBE, e.OFFSETS))
refuse("resample-field_dtype", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 8\) of int64",
       lambda e: e.ctx.resample(i64(e, "i", (T, CELLS)), e.OFFSETS))
refuse("resample-offsets", r"offsets: expected a table of M \+ 1 entries, got shape \(2, 2\)", lambda e: e.ctx.resample(e.A, np.zeros((2, 2))))
refuse("resample-offsets_empty", r"offsets: expected a table of M \+ 1 entries, got shape \(0,\)", lambda e: e.ctx.resample(e.A, []))
refuse("resample-sizes-T", r"sd_downscale: sd_resample: bad sizes \(T=0, C=8, M=2\)", lambda e: e.ctx.resample(EMPTY, e.OFFSETS))
refuse("resample-sizes-C", r"sd_downscale: sd_resample: bad sizes \(T=24, C=0, M=2\)", lambda e: e.ctx.resample(NO_CELLS, e.OFFSETS))
refuse("resample-sizes-M", r"sd_downscale: sd_resample: bad sizes \(T=24, C=8, M=0\)", lambda e: e.ctx.resample(e.A, [0]))
refuse("resample-out", r"out: expected a float64 DeviceArray of shape \(2, 8\)", lambda e: e.ctx.resample(e.dA, e.OFFSETS, out=e.out(M + 1, CELLS)))
refuse("resample-context-field", ANOTHER.format("sd_resample", "field"), lambda e: e.ctx.resample(other(e).dA, e.OFFSETS))
refuse("resample-context-out", ANOTHER.format("sd_resample", "out"), lambda e: e.ctx.resample(e.A, e.OFFSETS, out=other(e).out(M, CELLS)))
refuse("resample_host-resident", "resample_host: expected a host array", lambda e: e.ctx.resample_host(e.dA, e.OFFSETS))
refuse("resample-order-op-field", "resample reduction 'max'", lambda e: e.ctx.resample(CUBE, e.OFFSETS, "max"))
refuse("resample-order-field-offsets", "field: expected a float32 or float64", lambda e: e.ctx.resample(CUBE, []))
refuse("resample-order-offsets-sizes", "offsets: expected a table", lambda e: e.ctx.resample(EMPTY, []))
refuse("resample-order-sizes-out", "bad sizes", lambda e: e.ctx.resample(EMPTY, e.OFFSETS, out=e.out(M + 1, CELLS)))
refuse("resample-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.resample(other(e).dA, e.OFFSETS, out=e.out(M + 1, CELLS)))
refuse("resample_host-order-offsets-resident", "offsets: expected a table", lambda e: e.ctx.resample_host(e.dA, []))

# spells
refuse("spells-op", "where op '==': expected one of '>', '>=', '<', '<='", lambda e: e.ctx.spells(e.A, "==", 0.0, e.OFFSETS, "count"))
refuse("spells-stat", "spell statistic 'mean': expected one of 'valid', 'count', 'fraction', 'longest_spell', 'spell_days', 'spell_count'",
       lambda e: e.ctx.spells(e.A, ">", 0.0, e.OFFSETS, ["count", "mean"]))
refuse("spells-no_stats", "sd_downscale: sd_spells: nstat = 0, expected 1 to 6 statistics", lambda e: e.ctx.spells(e.A, ">", 0.0, e.OFFSETS, []))
refuse("spells-too_many_stats", "sd_downscale: sd_spells: nstat = 7, expected 1 to 6 statistics", lambda e: e.ctx.spells(e.A, ">", 0.0, e.OFFSETS, ["count"] * 7))
refuse("spells-field", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\) of float64", lambda e: e.ctx.spells(CUBE, ">", 0.0, e.OFFSETS, "count"))
refuse("spells-offsets", r"offsets: expected a table of M \+ 1 entries, got shape \(0,\)", lambda e: e.ctx.spells(e.A, ">", 0.0, [], "count"))
refuse("spells-sizes", r"sd_downscale: sd_spells: bad sizes \(T=24, C=8, M=0\)", lambda e: e.ctx.spells(e.A, ">", 0.0, [0], "count"))
refuse("spells-threshold-cells", r"threshold: expected a number or a float64 \[G, 8\] table, got shape \(3, 7\) of float64",
       lambda e: e.ctx.spells(e.A, ">", np.zeros((G, CELLS - 1)), e.OFFSETS, "count"))
refuse("spells-threshold-rank", r"threshold: expected a number or a float64 \[G, 8\] table, got shape \(8,\) of float64",
       lambda e: e.ctx.spells(e.A, ">", np.zeros(CELLS), e.OFFSETS, "count"))
refuse("spells-threshold-dtype", r"threshold: expected a number or a float64 \[G, 8\] table, got shape \(3, 8\) of float32",
       lambda e: e.ctx.spells(e.dA, ">", e.dTAB32, e.OFFSETS, "count"))
refuse("spells-threshold-no_rows", r"threshold: expected a number or a float64 \[G, 8\] table, got shape \(0, 8\)",
       lambda e: e.ctx.spells(e.A, ">", EMPTY, e.OFFSETS, "count"))
refuse("spells-group", r"group: expected one group id per row \(24\), got shape \(2,\)", lambda e: e.ctx.spells(e.A, ">", e.TAB, e.OFFSETS, "count", group=e.BIN_GROUP))
refuse("spells-scalar_with_group", "group: a scalar threshold takes no group ids", lambda e: e.ctx.spells(e.A, ">", 0.0, e.OFFSETS, "count", group=e.GROUP))
refuse("spells-out", r"out: expected a float64 DeviceArray of shape \(4, 8\)", lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.out(M, CELLS)))
refuse("spells-planes-out_shape", r"out: expected a float64 DeviceArray of shape \(2, 8\)",
       lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.out(2 * M, CELLS), plane_rows=PLANE_ROWS))
refuse("spells-planes-no_base", PLANES_WORDS.format(5),
       lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.lib.resident(e.ctx, "whole", (M, CELLS)), plane_rows=PLANE_ROWS))
refuse("spells-planes-cells_view", PLANES_WORDS.format(5), lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.out(M, CELLS), plane_rows=PLANE_ROWS))
refuse("spells-planes-short_planes", PLANES_WORDS.format(1), lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.planes(2), plane_rows=1))
refuse("spells-planes-past_the_end", PLANES_WORDS.format(8), lambda e: e.ctx.spells(e.dA, ">", 0.0, e.OFFSETS, STATS2, out=e.planes(2), plane_rows=8))
refuse("spells-context-field", ANOTHER.format("sd_spells", "field"), lambda e: e.ctx.spells(other(e).dA, ">", 0.0, e.OFFSETS, "count"))
refuse("spells-context-threshold", ANOTHER.format("sd_spells", "threshold"), lambda e: e.ctx.spells(e.A, ">", other(e).dTAB1, e.OFFSETS, "count"))
refuse("spells-context-out", ANOTHER.format("sd_spells", "out"), lambda e: e.ctx.spells(e.A, ">", e.TAB1, e.OFFSETS, "count", out=other(e).out(M, CELLS)))
refuse("spells_host-resident_field", "spells_host: expected host arrays", lambda e: e.ctx.spells_host(e.dA, ">", 0.0, e.OFFSETS, "count"))
refuse("spells_host-resident_table", "spells_host: expected host arrays", lambda e: e.ctx.spells_host(e.A, ">", e.dTAB1, e.OFFSETS, "count"))
refuse("spells-order-op-stat", "where op '=='", lambda e: e.ctx.spells(e.A, "==", 0.0, e.OFFSETS, "mean"))
refuse("spells-order-stat-count", "spell statistic 'mean'", lambda e: e.ctx.spells(e.A, ">", 0.0, e.OFFSETS, ["mean"] * 7))
refuse("spells-order-count-field", "nstat = 0", lambda e: e.ctx.spells(CUBE, ">", 0.0, e.OFFSETS, []))
refuse("spells-order-field-offsets", "field: expected", lambda e: e.ctx.spells(CUBE, ">", 0.0, [], "count"))
refuse("spells-order-offsets-sizes", "offsets: expected a table", lambda e: e.ctx.spells(EMPTY, ">", 0.0, [], "count"))
refuse("spells-order-sizes-threshold", "bad sizes", lambda e: e.ctx.spells(e.A, ">", np.zeros(CELLS), [0], "count"))
refuse("spells-order-threshold-group", "threshold: expected a number", lambda e: e.ctx.spells(e.A, ">", np.zeros(CELLS), e.OFFSETS, "count", group=e.BIN_GROUP))
refuse("spells-order-group-out", "group: expected one group id per row", lambda e: e.ctx.spells(e.dA, ">", e.dTAB, e.OFFSETS, "count", group=e.BIN_GROUP, out=e.out(1, 1)))
refuse("spells-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.spells(other(e).dA, ">", 0.0, e.OFFSETS, "count", out=e.out(1, 1)))
refuse("spells_host-order-group-resident", "group: a scalar threshold takes no group ids", lambda e: e.ctx.spells_host(e.dA, ">", 0.0, e.OFFSETS, "count", group=e.GROUP))

# the paired calls
PAIR_WORDS = {"skill": ("skill statistic 'ks': expected one of 'count', 'bias', 'ratio', 'mae', 'rmse', 'corr', 'std_ratio'", 7, "bias"),
              "twosample": ("distribution statistic 'bias': expected one of 'ks', 'perkins', 'na', 'nb'", 4, "ks")}
for name, (rest, nstat) in PAIRED.items():
    who, family, grouped = "sd_" + name, name.split("_")[0], "groups" in name
    words, most, good = PAIR_WORDS[family]
    bad = "ks" if family == "skill" else "bias"

    def paired(e, a, b, name=name, grouped=grouped, good=good, host=False, stats=None, bins=None, **more):
        bins = ((e.GROUP, G) if grouped else (e.OFFSETS,)) if bins is None else bins
        return e.call("host" if host else "res", name)(a, b, *bins, good if stats is None else stats, **more)

    refuse(f"{name}-stat", words, lambda e, paired=paired, bad=bad: paired(e, e.A, e.B, stats=["na" if bad == "bias" else "bias", bad]))
    refuse(f"{name}-no_stats", f"sd_downscale: {who}: nstat = 0, expected 1 to {most} statistics", lambda e, paired=paired: paired(e, e.A, e.B, stats=[]))
    refuse(f"{name}-too_many_stats", f"sd_downscale: {who}: nstat = {most + 1}, expected 1 to {most} statistics",
           lambda e, paired=paired, good=good, most=most: paired(e, e.A, e.B, stats=[good] * (most + 1)))
    refuse(f"{name}-a", r"a: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\) of float64", lambda e, paired=paired: paired(e, CUBE, e.B))
    refuse(f"{name}-b", r"b: expected a float32 or float64 \[T, C\] field, got shape \(24, 8\) of int64",
           lambda e, paired=paired: paired(e, e.dA, i64(e, "i", (T, CELLS))))
    refuse(f"{name}-shapes", r"b: expected a \[T, C\] field of shape \(24, 8\) like a, got shape \(3, 8\)", lambda e, paired=paired: paired(e, e.A, e.TAB))
    refuse(f"{name}-out", rf"out: expected a float64 DeviceArray of shape \({G if grouped else M}, 8\)",
           lambda e, paired=paired: paired(e, e.dA, e.dB, out=e.out(1, CELLS)))
    refuse(f"{name}-planes-short_planes", r"out: expected the rows of [23] bins inside the first of 1 planes of 1 rows of a DeviceArray",
           lambda e, paired=paired, grouped=grouped: paired(e, e.dA, e.dB, out=e.out(G if grouped else M, CELLS), plane_rows=1))
    for arg in ("a", "b", "out"):
        refuse(f"{name}-context-{arg}", ANOTHER.format(who, arg), lambda e, paired=paired, arg=arg, grouped=grouped: paired(
            e, other(e).dA if arg == "a" else e.A, other(e).dB if arg == "b" else e.B32, out=other(e).out(G if grouped else M, CELLS) if arg == "out" else None))
    refuse(f"{name}_host-resident_a", f"{name}_host: expected host arrays", lambda e, paired=paired: paired(e, e.dA, e.B, host=True))
    refuse(f"{name}_host-resident_b", f"{name}_host: expected host arrays", lambda e, paired=paired: paired(e, e.A, e.dB, host=True))
    refuse(f"{name}-order-stat-count", words.split(":")[0], lambda e, paired=paired, bad=bad, most=most: paired(e, e.A, e.B, stats=[bad] * (most + 1)))
    refuse(f"{name}-order-count-a", "nstat = 0", lambda e, paired=paired: paired(e, CUBE, e.B, stats=[]))
    refuse(f"{name}-order-a-b", "a: expected a float32 or float64", lambda e, paired=paired: paired(e, CUBE, CUBE[0, 0]))
    refuse(f"{name}-order-b-shapes", "b: expected a float32 or float64", lambda e, paired=paired: paired(e, e.A, CUBE))
    if grouped:
        refuse(f"{name}-group", r"group: expected one group id per row \(24\), got shape \(2,\)", lambda e, paired=paired: paired(e, e.A, e.B, bins=(e.BIN_GROUP, G)))
        refuse(f"{name}-sizes-T", rf"sd_downscale: {who}: bad sizes \(T=0, C=8\)", lambda e, paired=paired: paired(e, EMPTY, EMPTY, bins=([], G)))
        refuse(f"{name}-sizes-C", rf"sd_downscale: {who}: bad sizes \(T=24, C=0\)", lambda e, paired=paired: paired(e, NO_CELLS, NO_CELLS))
        refuse(f"{name}-sizes-G", rf"sd_downscale: {who}: bad sizes \(G=0\)", lambda e, paired=paired: paired(e, e.A, e.B, bins=(e.GROUP, 0)))
        refuse(f"{name}-order-shapes-group", "b: expected a .T, C. field of shape", lambda e, paired=paired: paired(e, e.A, e.TAB, bins=(e.BIN_GROUP, G)))
        refuse(f"{name}-order-group-sizes", "group: expected one group id per row", lambda e, paired=paired: paired(e, NO_CELLS, NO_CELLS, bins=(e.BIN_GROUP, G)))
        refuse(f"{name}-order-sizes-G", r"bad sizes \(T=24, C=0\)", lambda e, paired=paired: paired(e, NO_CELLS, NO_CELLS, bins=(e.GROUP, 0)))
        refuse(f"{name}-order-G-out", r"bad sizes \(G=0\)", lambda e, paired=paired: paired(e, e.dA, e.dB, bins=(e.GROUP, 0), out=e.out(1, 1)))
        refuse(f"{name}_host-order-G-resident", r"bad sizes \(G=0\)", lambda e, paired=paired: paired(e, e.dA, e.dB, bins=(e.GROUP, 0), host=True))
    else:
        refuse(f"{name}-offsets", r"offsets: expected a table of M \+ 1 entries, got shape \(0,\)", lambda e, paired=paired: paired(e, e.A, e.B, bins=([],)))
        refuse(f"{name}-sizes-T", rf"sd_downscale: {who}: bad sizes \(T=0, C=8, M=2\)", lambda e, paired=paired: paired(e, EMPTY, EMPTY))
        refuse(f"{name}-sizes-M", rf"sd_downscale: {who}: bad sizes \(T=24, C=8, M=0\)", lambda e, paired=paired: paired(e, e.A, e.B, bins=([0],)))
        refuse(f"{name}-order-shapes-offsets", "b: expected a .T, C. field of shape", lambda e, paired=paired: paired(e, e.A, e.TAB, bins=([],)))
        refuse(f"{name}-order-offsets-sizes", "offsets: expected a table", lambda e, paired=paired: paired(e, EMPTY, EMPTY, bins=([],)))
        refuse(f"{name}-order-sizes-out", "bad sizes", lambda e, paired=paired: paired(e, e.dA, e.dB, bins=([0],), out=e.out(1, 1)))
        refuse(f"{name}_host-order-sizes-resident", "bad sizes", lambda e, paired=paired: paired(e, e.dA, e.dB, bins=([0],), host=True))
    refuse(f"{name}-order-out-context", "out: expected a float64 DeviceArray", lambda e, paired=paired: paired(e, other(e).dA, e.dB, out=e.out(1, 1)))
    if family == "twosample":
        refuse(f"{name}-perkins-no_width", r"perkins needs the width of the histogram bins \(width=...\)", lambda e, paired=paired: paired(e, e.A, e.B, stats="perkins"))
        for width in (0, -1.0, np.inf, np.nan, True, "1"):
            refuse(f"{name}-perkins-width-{width}", rf"width: expected a positive finite number, got {width!r}",
                   lambda e, paired=paired, width=width: paired(e, e.A, e.B, stats="perkins", width=width))
        for origin in (np.inf, False, None):
            refuse(f"{name}-perkins-origin-{origin}", rf"origin: expected a finite number, got {origin!r}",
                   lambda e, paired=paired, origin=origin: paired(e, e.A, e.B, stats="perkins", width=1, origin=origin))
        refuse(f"{name}-order-count-width", "nstat = 5", lambda e, paired=paired: paired(e, e.A, e.B, stats=["perkins"] * 5))
        refuse(f"{name}-order-width-origin", "width: expected", lambda e, paired=paired: paired(e, e.A, e.B, stats="perkins", width=0, origin=None))
        refuse(f"{name}-order-origin-a", "origin: expected", lambda e, paired=paired: paired(e, CUBE, e.B, stats="perkins", width=1, origin=None))

# disaggregate
refuse("disaggregate-op", "disaggregation op 'copy': only 'shift', 'scale_mean' and 'scale_sum' are implemented",
       lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, e.OFFSETS, "copy"))
refuse("disaggregate-obs", r"obs: expected a float32 or float64 \[To, C\] field, got shape \(24, 2, 8\) of float64",
       lambda e: e.ctx.disaggregate(e.TARGET, CUBE, e.SRC_ROW, e.OFFSETS))
refuse("disaggregate-target-cells", r"target: expected a float64 \[M, 8\] field, got shape \(2, 7\) of float64",
       lambda e: e.ctx.disaggregate(np.zeros((M, CELLS - 1)), e.A, e.SRC_ROW, e.OFFSETS))
refuse("disaggregate-target-dtype", r"target: expected a float64 \[M, 8\] field, got shape \(2, 8\) of float32",
       lambda e: e.ctx.disaggregate(e.dTARGET32, e.dA, e.SRC_ROW, e.OFFSETS))
refuse("disaggregate-climo", r"climo: expected a float64 \[G, 8\] field, got shape \(8,\) of float64",
       lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, e.OFFSETS, climo=np.zeros(CELLS), group=e.BIN_GROUP))
refuse("disaggregate-src_row", r"src_row: expected a table of Tout entries, got shape \(2, 2\)", lambda e: e.ctx.disaggregate(e.TARGET, e.A, np.zeros((2, 2)), e.OFFSETS))
refuse("disaggregate-offsets", r"offsets: expected a table of M \+ 1 = 3 entries, got shape \(2,\)", lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, [0, T]))
refuse("disaggregate-group_without_climo", "sd_downscale: sd_disagg: group without climo", lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, e.OFFSETS, group=e.BIN_GROUP))
refuse("disaggregate-climo_without_group", "sd_downscale: sd_disagg: climo without group", lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, e.OFFSETS, climo=e.TAB))
refuse("disaggregate-group", r"group: expected one climatology row per bin \(2\), got shape \(24,\)",
       lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, e.OFFSETS, climo=e.TAB, group=e.GROUP))
refuse("disaggregate-sizes-To", r"sd_downscale: sd_disagg: bad sizes \(To=0, C=8, Tout=24, M=2\)", lambda e: e.ctx.disaggregate(e.TARGET, EMPTY, e.SRC_ROW, e.OFFSETS))
refuse("disaggregate-sizes-Tout", r"sd_downscale: sd_disagg: bad sizes \(To=24, C=8, Tout=0, M=2\)", lambda e: e.ctx.disaggregate(e.TARGET, e.A, [], e.OFFSETS))
refuse("disaggregate-sizes-M", r"sd_downscale: sd_disagg: bad sizes \(To=24, C=8, Tout=24, M=0\)", lambda e: e.ctx.disaggregate(EMPTY, e.A, e.SRC_ROW, [0]))
refuse("disaggregate-out", r"out: expected a float64 DeviceArray of shape \(24, 8\)", lambda e: e.ctx.disaggregate(e.dTARGET, e.dA, e.SRC_ROW, e.OFFSETS, out=e.out(M, CELLS)))
for arg in ("target", "obs", "climo", "out"):
    refuse(f"disaggregate-context-{arg}", ANOTHER.format("sd_disagg", arg), lambda e, arg=arg: e.ctx.disaggregate(
        other(e).dTARGET if arg == "target" else e.TARGET, other(e).dA if arg == "obs" else e.A32, e.SRC_ROW, e.OFFSETS,
        climo=other(e).dTAB if arg == "climo" else e.TAB, group=e.BIN_GROUP, out=other(e).out(T, CELLS) if arg == "out" else None))
for arg in ("target", "obs", "climo"):
    refuse(f"disaggregate_host-resident_{arg}", "disaggregate_host: expected host arrays", lambda e, arg=arg: e.ctx.disaggregate_host(
        e.a("res" if arg == "target" else "host", "TARGET"), e.a("res" if arg == "obs" else "host", "A"), e.SRC_ROW, e.OFFSETS,
        climo=e.a("res" if arg == "climo" else "host", "TAB"), group=e.BIN_GROUP))
refuse("disaggregate-order-op-obs", "disaggregation op 'copy'", lambda e: e.ctx.disaggregate(e.TARGET, CUBE, e.SRC_ROW, e.OFFSETS, "copy"))
refuse("disaggregate-order-obs-target", "obs: expected", lambda e: e.ctx.disaggregate(np.zeros(3), CUBE, e.SRC_ROW, e.OFFSETS))
refuse("disaggregate-order-target-climo", "target: expected", lambda e: e.ctx.disaggregate(np.zeros(3), e.A, e.SRC_ROW, e.OFFSETS, climo=np.zeros(3)))
refuse("disaggregate-order-climo-src_row", "climo: expected", lambda e: e.ctx.disaggregate(e.TARGET, e.A, np.zeros((2, 2)), e.OFFSETS, climo=np.zeros(3)))
refuse("disaggregate-order-src_row-offsets", "src_row: expected", lambda e: e.ctx.disaggregate(e.TARGET, e.A, np.zeros((2, 2)), [0]))
refuse("disaggregate-order-offsets-climo_without_group", "offsets: expected", lambda e: e.ctx.disaggregate(e.TARGET, e.A, e.SRC_ROW, [0], climo=e.TAB))
refuse("disaggregate-order-group-sizes", "group: expected one climatology row", lambda e: e.ctx.disaggregate(e.TARGET, e.A, [], e.OFFSETS, climo=e.TAB, group=e.GROUP))
refuse("disaggregate-order-sizes-out", "bad sizes", lambda e: e.ctx.disaggregate(e.dTARGET, e.dA, [], e.OFFSETS, out=e.out(1, 1)))
refuse("disaggregate-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.disaggregate(other(e).dTARGET, e.dA, e.SRC_ROW, e.OFFSETS, out=e.out(1, 1)))
refuse("disaggregate_host-order-group-resident", "group: expected one climatology row",
       lambda e: e.ctx.disaggregate_host(e.dTARGET, e.A, e.SRC_ROW, e.OFFSETS, climo=e.TAB, group=e.GROUP))

# groupby
for host in (False, True):
    h = "_host" if host else ""
    reduce_, apply_ = (lambda e, *a, host=host, **k: e.call("host" if host else "res", "groupby_reduce")(*a, **k),
                       lambda e, *a, host=host, **k: e.call("host" if host else "res", "groupby_apply")(*a, **k))
    refuse(f"groupby_reduce{h}-op", "groupby_reduce op 'max': only 'mean', 'sum' are implemented", lambda e, c=reduce_: c(e, e.A, e.GROUP, G, "max"))
    refuse(f"groupby_apply{h}-op", "groupby_apply op 'pow': only 'sub', 'add', 'mul', 'div' are implemented", lambda e, c=apply_: c(e, e.A, e.GROUP, e.TAB, "pow"))
    refuse(f"groupby_reduce{h}-field", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\)", lambda e, c=reduce_: c(e, CUBE, e.GROUP, G))
    refuse(f"groupby_reduce{h}-group", r"group: expected one group id per row \(24\), got shape \(2,\)", lambda e, c=reduce_: c(e, e.A, e.BIN_GROUP, G))
    refuse(f"groupby_apply{h}-group", r"group: expected one group id per row \(24\), got shape \(2,\)", lambda e, c=apply_: c(e, e.A, e.BIN_GROUP, e.TAB, "sub"))
    refuse(f"groupby_reduce{h}-sizes-T", r"sd_downscale: sd_groupby_reduce: bad sizes \(T=0, C=8\)", lambda e, c=reduce_: c(e, EMPTY, [], G))
    refuse(f"groupby_apply{h}-sizes-C", r"sd_downscale: sd_groupby_apply: bad sizes \(T=24, C=0\)", lambda e, c=apply_: c(e, NO_CELLS, e.GROUP, np.zeros((G, 0)), "sub"))
    refuse(f"groupby_reduce{h}-sizes-G", r"sd_downscale: sd_groupby_reduce: bad sizes \(G=0\)", lambda e, c=reduce_: c(e, e.A, e.GROUP, 0))
    refuse(f"groupby_apply{h}-sizes-G", r"sd_downscale: sd_groupby_apply: bad sizes \(G=0\)", lambda e, c=apply_: c(e, e.A, e.GROUP, EMPTY, "sub"))
    refuse(f"groupby_reduce{h}-order-op-field", "op 'max'", lambda e, c=reduce_: c(e, CUBE, e.GROUP, G, "max"))
    refuse(f"groupby_reduce{h}-order-field-group", "field: expected", lambda e, c=reduce_: c(e, CUBE, e.BIN_GROUP, G))
    refuse(f"groupby_reduce{h}-order-group-sizes", "group: expected one group id per row", lambda e, c=reduce_: c(e, NO_CELLS, e.BIN_GROUP, G))
    refuse(f"groupby_reduce{h}-order-sizes-G", r"bad sizes \(T=24, C=0\)", lambda e, c=reduce_: c(e, NO_CELLS, e.GROUP, 0))
refuse("groupby_reduce-acc-shape", r"acc: expected the \(sum float64, count int32\) pair of \[4, 8\] DeviceArrays of an earlier call",
       lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G + 1, acc=(e.dSUM, e.dCOUNT)))
refuse("groupby_reduce-acc-dtype", r"acc: expected the \(sum float64, count int32\) pair of \[3, 8\] DeviceArrays", lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, acc=(e.dSUM, e.dSUM)))
refuse("groupby_reduce-acc-pitch", r"acc: expected the \(sum float64, count int32\) pair of \[3, 8\] DeviceArrays",
       lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, acc=(e.dSUM, e.lib.resident(e.ctx, "n", (G, CELLS), np.int32))))
refuse("groupby_reduce-out", r"out: expected a float64 DeviceArray of shape \(3, 8\)", lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, out=e.out(M, CELLS)))
for arg in ("field", "sum", "count", "out"):
    refuse(f"groupby_reduce-context-{arg}", ANOTHER.format("sd_groupby_reduce", arg), lambda e, arg=arg: e.ctx.groupby_reduce(
        other(e).dA if arg == "field" else e.A, e.GROUP, G, acc=(other(e).dSUM if arg == "sum" else e.dSUM, other(e).dCOUNT if arg == "count" else e.dCOUNT),
        out=other(e).out(G, CELLS) if arg == "out" else None))
refuse("groupby_reduce_host-resident", "groupby_reduce_host: expected a host array", lambda e: e.ctx.groupby_reduce_host(e.dA, e.GROUP, G))
refuse("groupby_reduce-order-G-acc", r"bad sizes \(G=0\)", lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, 0, acc=(e.dSUM, e.dSUM)))
refuse("groupby_reduce-order-acc-out", "acc: expected", lambda e: e.ctx.groupby_reduce(e.dA, e.GROUP, G, acc=(e.dSUM, e.dSUM), out=e.out(1, 1)))
refuse("groupby_reduce-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.groupby_reduce(other(e).dA, e.GROUP, G, out=e.out(1, 1)))
refuse("groupby_reduce_host-order-G-resident", r"bad sizes \(G=0\)", lambda e: e.ctx.groupby_reduce_host(e.dA, e.GROUP, 0))
refuse("groupby_apply-table-rank", r"table: expected a float64 \[G, C\] field, got shape \(8,\) of float64", lambda e: e.ctx.groupby_apply(e.A, e.GROUP, np.zeros(CELLS), "sub"))
refuse("groupby_apply-table-dtype", r"table: expected a float64 \[G, C\] field, got shape \(3, 8\) of float32", lambda e: e.ctx.groupby_apply(e.dA, e.GROUP, e.dTAB32, "sub"))
refuse("groupby_apply-table-cells", r"table: expected a float64 \[G, 8\] field, got shape \(3, 7\)", lambda e: e.ctx.groupby_apply(e.A, e.GROUP, np.zeros((G, CELLS - 1)), "sub"))
refuse("groupby_apply-out", r"out: expected a float64 DeviceArray of shape \(24, 8\)", lambda e: e.ctx.groupby_apply(e.dA, e.GROUP, e.dTAB, "sub", out=e.out(M, CELLS)))
for arg in ("field", "table", "out"):
    refuse(f"groupby_apply-context-{arg}", ANOTHER.format("sd_groupby_apply", arg), lambda e, arg=arg: e.ctx.groupby_apply(
        other(e).dA if arg == "field" else e.A, e.GROUP, other(e).dTAB if arg == "table" else e.TAB, "sub", out=other(e).out(T, CELLS) if arg == "out" else None))
refuse("groupby_apply_host-resident", "groupby_apply_host: expected a host .T, C. field and a host .G, C. table", lambda e: e.ctx.groupby_apply_host(e.dA, e.GROUP, e.TAB, "sub"))
refuse("groupby_apply_host-table-cells", "groupby_apply_host: expected a host .T, C. field and a host .G, C. table",
       lambda e: e.ctx.groupby_apply_host(e.A, e.GROUP, np.zeros((G, CELLS - 1)), "sub"))
refuse("groupby_apply-order-table-op", "table: expected a float64 .G, C. field", lambda e: e.ctx.groupby_apply(e.A, e.GROUP, np.zeros(CELLS), "pow"))
refuse("groupby_apply-order-G-table_cells", r"bad sizes \(G=0\)", lambda e: e.ctx.groupby_apply(e.A, e.GROUP, np.zeros((0, CELLS - 1)), "sub"))
refuse("groupby_apply-order-table_cells-out", "table: expected a float64 .G, 8. field", lambda e: e.ctx.groupby_apply(e.dA, e.GROUP, np.zeros((G, CELLS - 1)), "sub", out=e.out(1, 1)))
refuse("groupby_apply-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.groupby_apply(other(e).dA, e.GROUP, e.dTAB, "sub", out=e.out(1, 1)))
refuse("groupby_apply_host-order-G-resident", r"bad sizes \(G=0\)", lambda e: e.ctx.groupby_apply_host(e.dA, e.GROUP, EMPTY, "sub"))

# quantile and rolling
for host in (False, True):
    h = "_host" if host else ""
    quantile, rolling = (lambda e, *a, host=host, **k: e.call("host" if host else "res", "quantile")(*a, **k),
                         lambda e, *a, host=host, **k: e.call("host" if host else "res", "rolling")(*a, **k))
    refuse(f"quantile{h}-method", "quantile method 'cubic': expected one of 'linear', 'lower', 'higher', 'nearest', 'midpoint', 'median'",
           lambda e, c=quantile: c(e, e.A, 0.5, method="cubic"))
    refuse(f"quantile{h}-field", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\)", lambda e, c=quantile: c(e, CUBE, 0.5))
    refuse(f"quantile{h}-sizes", r"sd_downscale: sd_quantile: bad sizes \(T=0, C=8\)", lambda e, c=quantile: c(e, EMPTY, 0.5))
    refuse(f"quantile{h}-group", r"group: expected one group id per row \(24\), got shape \(2,\)", lambda e, c=quantile: c(e, e.A, 0.5, e.BIN_GROUP))
    refuse(f"quantile{h}-G", r"sd_downscale: sd_quantile: bad sizes \(G=0, Q=1\)", lambda e, c=quantile: c(e, e.A, 0.5, e.GROUP, 0))
    refuse(f"quantile{h}-q_rank", r"sd_downscale: sd_quantile: bad sizes \(G=1, Q=\(2, 2\)\)", lambda e, c=quantile: c(e, e.A, np.zeros((2, 2))))
    refuse(f"quantile{h}-no_q", r"sd_downscale: sd_quantile: bad sizes \(G=3, Q=0\)", lambda e, c=quantile: c(e, e.A, [], e.GROUP))
    refuse(f"quantile{h}-order-method-field", "quantile method 'cubic'", lambda e, c=quantile: c(e, CUBE, 0.5, method="cubic"))
    refuse(f"quantile{h}-order-field-sizes", "field: expected", lambda e, c=quantile: c(e, np.zeros((0, 2, CELLS)), 0.5))
    refuse(f"quantile{h}-order-sizes-group", r"bad sizes \(T=0, C=8\)", lambda e, c=quantile: c(e, EMPTY, 0.5, e.BIN_GROUP))
    refuse(f"quantile{h}-order-group-G", "group: expected one group id per row", lambda e, c=quantile: c(e, e.A, 0.5, e.BIN_GROUP, 0))
    refuse(f"rolling{h}-op", "rolling op 'max': only 'mean', 'sum', 'var', 'std' are implemented", lambda e, c=rolling: c(e, e.A, 5, "max"))
    refuse(f"rolling{h}-field", r"field: expected a float32 or float64 \[T, C\] field, got shape \(24, 2, 8\)", lambda e, c=rolling: c(e, CUBE, 5))
    refuse(f"rolling{h}-sizes", r"sd_downscale: sd_rolling: bad sizes \(T=24, C=0\)", lambda e, c=rolling: c(e, NO_CELLS, 5))
    refuse(f"rolling{h}-order-op-field", "rolling op 'max'", lambda e, c=rolling: c(e, CUBE, 5, "max"))
    refuse(f"rolling{h}-order-field-sizes", "field: expected", lambda e, c=rolling: c(e, np.zeros((0, 2, CELLS)), 5))
refuse("quantile-out", r"out: expected a float64 DeviceArray of shape \(6, 8\)", lambda e: e.ctx.quantile(e.dA, [0.1, 0.9], e.GROUP, out=e.out(2, CELLS)))
refuse("quantile-context-field", ANOTHER.format("sd_quantile", "field"), lambda e: e.ctx.quantile(other(e).dA, 0.5))
refuse("quantile-context-out", ANOTHER.format("sd_quantile", "out"), lambda e: e.ctx.quantile(e.A, 0.5, out=other(e).out(1, CELLS)))
refuse("quantile_host-resident", "quantile_host: expected a host array", lambda e: e.ctx.quantile_host(e.dA, 0.5))
refuse("quantile-order-G-out", r"bad sizes \(G=0, Q=1\)", lambda e: e.ctx.quantile(e.dA, 0.5, e.GROUP, 0, out=e.out(3, 3)))
refuse("quantile-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.quantile(other(e).dA, 0.5, out=e.out(3, 3)))
refuse("quantile_host-order-G-resident", r"bad sizes \(G=0, Q=1\)", lambda e: e.ctx.quantile_host(e.dA, 0.5, e.GROUP, 0))
refuse("rolling-n_out", "sd_downscale: sd_rolling: the output rows 24 .. 23 lie outside the 24 rows of the source", lambda e: e.ctx.rolling(e.A, 5, t0=T))
refuse("rolling-n_out-given", "sd_downscale: sd_rolling: the output rows 3 .. 2 lie outside the 24 rows of the source", lambda e: e.ctx.rolling(e.A, 5, t0=3, n_out=0))
refuse("rolling-out", r"out: expected a float64 DeviceArray of shape \(7, 8\)", lambda e: e.ctx.rolling(e.dA, 5, t0=3, n_out=7, out=e.out(T, CELLS)))
refuse("rolling-context-field", ANOTHER.format("sd_rolling", "field"), lambda e: e.ctx.rolling(other(e).dA, 5))
refuse("rolling-context-out", ANOTHER.format("sd_rolling", "out"), lambda e: e.ctx.rolling(e.A, 5, out=other(e).out(T, CELLS)))
refuse("rolling_host-resident", "rolling_host: expected a host array", lambda e: e.ctx.rolling_host(e.dA, 5))
refuse("rolling-order-sizes-n_out", r"bad sizes \(T=24, C=0\)", lambda e: e.ctx.rolling(NO_CELLS, 5, t0=T))
refuse("rolling-order-n_out-out", "the output rows", lambda e: e.ctx.rolling(e.dA, 5, t0=T, out=e.out(1, 1)))
refuse("rolling-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.rolling(other(e).dA, 5, out=e.out(1, 1)))
refuse("rolling_host-order-sizes-resident", r"bad sizes \(T=24, C=0\)", lambda e: e.ctx.rolling_host(e.lib.resident(e.ctx, "none", (T, 0)), 5))

# the analog library: the coarse side, shared by ca_select, ca_weights and ca_local
COARSE = {
    "ca_select": lambda e, L, Q, wc=None, k=K, **more: e.ctx.ca_select(L, Q, e.WC if wc is None else wc, k, **more),
    "ca_weights": lambda e, L, Q, wc=None, k=K, **more: e.ctx.ca_weights(L, Q, e.WC if wc is None else wc, e.lib.resident(e.ctx, "idx", (TQ, k), np.int32),
                                                                         more.pop("dist", e.dDIST), more.pop("status", e.dSTATUS), **more),
    "ca_local": lambda e, L, Q, wc=None, k=K, grid=(NY, NX), radius=(1, 2): e.ctx.ca_local(L, Q, e.WC if wc is None else wc, grid, radius,
                                                                                            e.lib.resident(e.ctx, "idx", (TQ, k), np.int32)),
}
for name, coarse in COARSE.items():
    who = "sd_" + name
    refuse(f"{name}-L", r"L: expected a \[Tl, Cc\] field, got shape \(24, 2, 8\)", lambda e, c=coarse: c(e, CUBE, e.Q))
    refuse(f"{name}-L-dtype", r"L: expected a float64 \[Tl, Cc\] field, got shape \(6, 8\) of float32", lambda e, c=coarse: c(e, e.dL32, e.dQ))
    refuse(f"{name}-Q", r"Q: expected a \[Tq, Cc\] field, got shape \(8,\)", lambda e, c=coarse: c(e, e.L, np.zeros(CELLS)))
    refuse(f"{name}-Q-cells", r"Q: expected a \[Tq, 8\] field like L, got shape \(4, 7\)", lambda e, c=coarse: c(e, e.L, np.zeros((TQ, CELLS - 1))))
    refuse(f"{name}-sizes-Tl", rf"sd_downscale: {who}: bad sizes \(Tl=0, Tq=4, Cc=8\)", lambda e, c=coarse: c(e, EMPTY, e.Q))
    refuse(f"{name}-wc", r"wc: expected 8 column weights, got shape \(7,\)", lambda e, c=coarse: c(e, e.L, e.Q, np.ones(CELLS - 1)))
    refuse(f"{name}-k", rf"sd_downscale: {who}: k = 33 lies outside \[1, 32\]", lambda e, c=coarse: c(e, e.L, e.Q, k=33))
    refuse(f"{name}-context-L", ANOTHER.format(who, "L"), lambda e, c=coarse: c(e, other(e).dL, e.Q))
    refuse(f"{name}-context-Q", ANOTHER.format(who, "Q"), lambda e, c=coarse: c(e, e.L, other(e).dQ))
    refuse(f"{name}-order-L-Q", "L: expected", lambda e, c=coarse: c(e, CUBE, np.zeros(CELLS)))
    refuse(f"{name}-order-Q-cells", r"Q: expected a \[Tq, Cc\] field", lambda e, c=coarse: c(e, e.L, np.zeros(CELLS - 1)))
    refuse(f"{name}-order-cells-sizes", "Q: expected a .Tq, 8. field like L", lambda e, c=coarse: c(e, e.L, np.zeros((0, CELLS - 1))))
    refuse(f"{name}-order-sizes-wc", "bad sizes", lambda e, c=coarse: c(e, EMPTY, e.Q, np.ones(CELLS - 1)))
    refuse(f"{name}-order-wc-k", "wc: expected", lambda e, c=coarse: c(e, e.L, e.Q, np.ones(CELLS - 1), 33))
refuse("ca_select-k-0", r"sd_downscale: sd_ca_select: k = 0 lies outside \[1, 32\]", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, 0))
for arg, n in (("key_l", TL), ("key_q", TQ), ("excl_l", TL), ("excl_q", TQ)):
    refuse(f"ca_select-{arg}", rf"{arg}: expected one id per day \({n}\), got shape \(24,\)", lambda e, arg=arg: e.ctx.ca_select(e.L, e.Q, e.WC, K, **{arg: e.GROUP}))
refuse("ca_select-order-k-key_l", "k = 33", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, 33, key_l=e.GROUP))
refuse("ca_select-order-key_l-key_q", "key_l: expected", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, K, key_l=e.GROUP, key_q=e.GROUP))
refuse("ca_select-order-key_q-excl_l", "key_q: expected", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, K, key_q=e.GROUP, excl_l=e.GROUP))
refuse("ca_select-order-excl_l-excl_q", "excl_l: expected", lambda e: e.ctx.ca_select(e.L, e.Q, e.WC, K, excl_l=e.GROUP, excl_q=e.GROUP))
refuse("ca_select-order-excl_q-context", "excl_q: expected", lambda e: e.ctx.ca_select(other(e).dL, e.dQ, e.WC, K, excl_q=e.GROUP))

IDX_WORDS = r"idx: expected the int32 \[Tq, k\] DeviceArray of ca_select"
refuse("ca_weights-kind", "kind='median': expected one of 'regression', 'mean'", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, e.dSTATUS, "median"))
refuse("ca_weights-idx-host", IDX_WORDS, lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, np.zeros((TQ, K), np.int32), e.dDIST, e.dSTATUS))
refuse("ca_weights-idx-rank", IDX_WORDS, lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dSTATUS, e.dDIST, e.dSTATUS))
refuse("ca_weights-idx-rows", r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)",
       lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.lib.resident(e.ctx, "idx", (TQ + 1, K), np.int32), e.dDIST, e.dSTATUS))
refuse("ca_weights-idx-dtype", r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dDIST, e.dDIST, e.dSTATUS))
refuse("ca_weights-idx-pitch", r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)",
       lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.wide("idx", (TQ, K), np.int32), e.dDIST, e.dSTATUS))
refuse("ca_weights-dist", r"dist: expected a contiguous float64 DeviceArray of shape \(4, 3\)", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dIDX, e.dSTATUS))
refuse("ca_weights-dist-host", r"dist: expected a contiguous float64 DeviceArray of shape \(4, 3\)", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, np.zeros((TQ, K)), e.dSTATUS))
refuse("ca_weights-status", r"status: expected an int32 DeviceArray of shape \(4,\)", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, e.dCELL_OF))
refuse("ca_weights-status-host", r"status: expected an int32 DeviceArray of shape \(4,\)", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, np.zeros(TQ, np.int32)))
for ridge, words in ((-1.0, "-1"), (np.inf, "inf"), (np.nan, "nan")):
    refuse(f"ca_weights-ridge-{words}", rf"sd_downscale: sd_ca_weights: ridge = {words}, expected a finite factor >= 0",
           lambda e, ridge=ridge: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, e.dSTATUS, ridge=ridge))
for arg in ("idx", "dist", "status"):
    refuse(f"ca_weights-context-{arg}", ANOTHER.format("sd_ca_weights", arg), lambda e, arg=arg: e.ctx.ca_weights(
        e.L, e.dQ, e.WC, other(e).dIDX if arg == "idx" else e.dIDX, other(e).dDIST if arg == "dist" else e.dDIST, other(e).dSTATUS if arg == "status" else e.dSTATUS))
refuse("ca_weights-order-kind-idx", "kind='median'", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, None, e.dDIST, e.dSTATUS, "median"))
refuse("ca_weights-order-idx-L", IDX_WORDS, lambda e: e.ctx.ca_weights(CUBE, e.Q, e.WC, None, e.dDIST, e.dSTATUS))
refuse("ca_weights-order-wc-idx_rows", "wc: expected", lambda e: e.ctx.ca_weights(e.L, e.Q, np.ones(3), e.lib.resident(e.ctx, "idx", (TQ + 1, K), np.int32), e.dDIST, e.dSTATUS))
refuse("ca_weights-order-idx_rows-dist", "idx: expected a contiguous int32", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dDIST, e.dIDX, e.dSTATUS))
refuse("ca_weights-order-dist-status", "dist: expected a contiguous float64", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dIDX, e.dCELL_OF))
refuse("ca_weights-order-status-ridge", "status: expected an int32", lambda e: e.ctx.ca_weights(e.L, e.Q, e.WC, e.dIDX, e.dDIST, e.dCELL_OF, ridge=-1))
refuse("ca_weights-order-ridge-context", "ridge = -1", lambda e: e.ctx.ca_weights(other(e).dL, e.dQ, e.WC, e.dIDX, e.dDIST, e.dSTATUS, ridge=-1))

FINE_WORDS = r"F: expected a float32 or float64 \[Tl, Cf\] DeviceArray"
ROWS_WORDS = r"sd_downscale: {}: rows \[{}, {}\) lie outside the 4 targets"
refuse("ca_apply-F-host", FINE_WORDS, lambda e: e.ctx.ca_apply(e.F, e.dIDX, e.dWEIGHTS))
refuse("ca_apply-F-rank", FINE_WORDS, lambda e: e.ctx.ca_apply(e.dSRC_WHOLE, e.dIDX, e.dWEIGHTS))
refuse("ca_apply-F-dtype", FINE_WORDS, lambda e: e.ctx.ca_apply(e.dLOCAL, e.dIDX, e.dWEIGHTS))
refuse("ca_apply-idx", IDX_WORDS, lambda e: e.ctx.ca_apply(e.dF, e.dSTATUS, e.dWEIGHTS))
refuse("ca_apply-idx-dtype", r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)", lambda e: e.ctx.ca_apply(e.dF, e.dDIST, e.dWEIGHTS))
refuse("ca_apply-weights", r"weights: expected a contiguous float64 DeviceArray of shape \(4, 3\)", lambda e: e.ctx.ca_apply(e.dF, e.dIDX, e.dIDX))
for q0, q1 in ((-1, 2), (2, 2), (0, TQ + 1)):
    refuse(f"ca_apply-rows-{q0}-{q1}", ROWS_WORDS.format("sd_ca_apply", q0, q1), lambda e, q0=q0, q1=q1: e.ctx.ca_apply(e.dF, e.dIDX, e.dWEIGHTS, q0, q1))
refuse("ca_apply-out", r"out: expected a float64 DeviceArray of shape \(2, 8\)", lambda e: e.ctx.ca_apply(e.dF, e.dIDX, e.dWEIGHTS, 1, 3, out=e.out(TQ, CELLS)))
for arg in ("F", "idx", "weights", "out"):
    refuse(f"ca_apply-context-{arg}", ANOTHER.format("sd_ca_apply", arg), lambda e, arg=arg: e.ctx.ca_apply(
        other(e).dF if arg == "F" else e.dF, other(e).dIDX if arg == "idx" else e.dIDX, other(e).dWEIGHTS if arg == "weights" else e.dWEIGHTS,
        out=other(e).out(TQ, CELLS) if arg == "out" else None))
refuse("ca_apply-order-F-idx", FINE_WORDS, lambda e: e.ctx.ca_apply(e.F, None, e.dWEIGHTS))
refuse("ca_apply-order-idx-weights", IDX_WORDS, lambda e: e.ctx.ca_apply(e.dF, None, None))
refuse("ca_apply-order-idx_dtype-weights", "idx: expected a contiguous int32", lambda e: e.ctx.ca_apply(e.dF, e.dDIST, e.dIDX))
refuse("ca_apply-order-weights-rows", "weights: expected a contiguous float64", lambda e: e.ctx.ca_apply(e.dF, e.dIDX, e.dIDX, 2, 2))
refuse("ca_apply-order-rows-out", "rows .2, 2. lie outside", lambda e: e.ctx.ca_apply(e.dF, e.dIDX, e.dWEIGHTS, 2, 2, out=e.out(1, 1)))
refuse("ca_apply-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.ctx.ca_apply(other(e).dF, e.dIDX, e.dWEIGHTS, out=e.out(1, 1)))

refuse("ca_local-idx", IDX_WORDS, lambda e: e.ctx.ca_local(e.L, e.Q, e.WC, (NY, NX), (1, 2), np.zeros((TQ, K), np.int32)))
refuse("ca_local-grid-parse", r"grid=3, radius=\(1, 2\): expected \(ny, nx\) and \(ry, rx\)", lambda e: COARSE["ca_local"](e, e.L, e.Q, grid=3))
refuse("ca_local-radius-parse", r"grid=\(2, 4\), radius=\(1, 2, 3\): expected \(ny, nx\) and \(ry, rx\)", lambda e: COARSE["ca_local"](e, e.L, e.Q, radius=(1, 2, 3)))
refuse("ca_local-grid", r"grid: expected \(ny, nx\) with ny \* nx = 8 columns, got \(3, 3\)", lambda e: COARSE["ca_local"](e, e.L, e.Q, grid=(3, 3)))
refuse("ca_local-grid-0", r"grid: expected \(ny, nx\) with ny \* nx = 8 columns, got \(-2, -4\)", lambda e: COARSE["ca_local"](e, e.L, e.Q, grid=(-2, -4)))
refuse("ca_local-radius", r"sd_downscale: sd_ca_local: radii \(-1, 2\), expected two numbers of coarse cells >= 0", lambda e: COARSE["ca_local"](e, e.L, e.Q, radius=(-1, 2)))
refuse("ca_local-idx-rows", r"idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)",
       lambda e: e.ctx.ca_local(e.L, e.Q, e.WC, (NY, NX), (1, 2), e.lib.resident(e.ctx, "idx", (TQ + 1, K), np.int32)))
refuse("ca_local-context-idx", ANOTHER.format("sd_ca_local", "idx"), lambda e: e.ctx.ca_local(e.L, e.dQ, e.WC, (NY, NX), (1, 2), other(e).dIDX))
refuse("ca_local-order-idx-L", IDX_WORDS, lambda e: e.ctx.ca_local(CUBE, e.Q, e.WC, (NY, NX), (1, 2), None))
refuse("ca_local-order-k-grid", "k = 33", lambda e: COARSE["ca_local"](e, e.L, e.Q, k=33, grid=3))
refuse("ca_local-order-parse-grid", "expected .ny, nx. and .ry, rx.", lambda e: COARSE["ca_local"](e, e.L, e.Q, grid=(3, 3), radius=1))
refuse("ca_local-order-grid-radius", "grid: expected", lambda e: COARSE["ca_local"](e, e.L, e.Q, grid=(3, 3), radius=(-1, 2)))
refuse("ca_local-order-radius-idx_rows", "radii", lambda e: e.ctx.ca_local(e.L, e.Q, e.WC, (NY, NX), (-1, 2), e.lib.resident(e.ctx, "idx", (TQ + 1, K), np.int32)))
refuse("ca_local-order-idx_rows-context", "idx: expected a contiguous int32",
       lambda e: e.ctx.ca_local(other(e).dL, e.dQ, e.WC, (NY, NX), (1, 2), e.lib.resident(e.ctx, "idx", (TQ + 1, K), np.int32)))


def local_apply(e, F="dF", cell_of="dCELL_OF", local_idx="dLOCAL", L="dL", Q="dQ", src=None, **more):
    """``ca_local_apply`` on the arrays of these names; the one named ``src`` is another context's"""
    a = {name: getattr(other(e) if name == src else e, name) if isinstance(name, str) else name for name in (F, cell_of, local_idx, L, Q)}
    return e.ctx.ca_local_apply(a[F], a[cell_of], a[local_idx], a[L], a[Q], **more)


refuse("ca_local_apply-F", FINE_WORDS, lambda e: local_apply(e, F="F"))
refuse("ca_local_apply-F-dtype", FINE_WORDS, lambda e: local_apply(e, F="dLOCAL"))
refuse("ca_local_apply-cell_of", r"cell_of: expected an int32 DeviceArray of shape \(8,\)", lambda e: local_apply(e, cell_of="dSTATUS"))
refuse("ca_local_apply-cell_of-host", r"cell_of: expected an int32 DeviceArray of shape \(8,\)", lambda e: local_apply(e, cell_of="WC"))
refuse("ca_local_apply-local_idx", r"local_idx: expected the int32 \[Tq, Cc\] DeviceArray of ca_local", lambda e: local_apply(e, local_idx="dSTATUS"))
refuse("ca_local_apply-local_idx-pitch", r"local_idx: expected a contiguous int32 DeviceArray of shape \(3, 8\)", lambda e: local_apply(e, local_idx="dCOUNT"))
refuse("ca_local_apply-local_idx-dtype", r"local_idx: expected a contiguous int32 DeviceArray of shape \(4, 3\)", lambda e: local_apply(e, local_idx="dDIST"))
refuse("ca_local_apply-adjust", "adjust='add': expected one of 'none', 'shift', 'scale'", lambda e: local_apply(e, adjust="add"))
for max_scale, words in ((-1.0, "-1"), (np.nan, "nan")):
    refuse(f"ca_local_apply-max_scale-{words}", rf"sd_downscale: sd_ca_local_apply: max_scale = {words}, expected 0 \(no limit\) or a limit > 0",
           lambda e, max_scale=max_scale: local_apply(e, max_scale=max_scale))
refuse("ca_local_apply-L-missing", r"L: adjust='shift' needs a float64 DeviceArray of shape \(6, 8\) \[Tl, Cc\]", lambda e: local_apply(e, L=None, adjust="shift"))
refuse("ca_local_apply-L-rows", r"L: adjust='scale' needs a float64 DeviceArray of shape \(6, 8\) \[Tl, Cc\]", lambda e: local_apply(e, L="dQ", adjust="scale"))
refuse("ca_local_apply-Q-dtype", r"Q: adjust='shift' needs a float64 DeviceArray of shape \(4, 8\) \[Tq, Cc\]", lambda e: local_apply(e, Q="dQ32", adjust="shift"))
refuse("ca_local_apply-Q-host", r"Q: adjust='shift' needs a float64 DeviceArray of shape \(4, 8\) \[Tq, Cc\]", lambda e: local_apply(e, Q="Q", adjust="shift"))
for q0, q1 in ((-1, 2), (3, 2), (0, TQ + 1)):
    refuse(f"ca_local_apply-rows-{q0}-{q1}", ROWS_WORDS.format("sd_ca_local_apply", q0, q1), lambda e, q0=q0, q1=q1: local_apply(e, q0=q0, q1=q1))
refuse("ca_local_apply-out", r"out: expected a float64 DeviceArray of shape \(2, 8\)", lambda e: local_apply(e, q0=1, q1=3, out=e.out(TQ, CELLS)))
for arg, name in (("F", "dF"), ("cell_of", "dCELL_OF"), ("local_idx", "dLOCAL"), ("L", "dL"), ("Q", "dQ")):
    refuse(f"ca_local_apply-context-{arg}", ANOTHER.format("sd_ca_local_apply", arg), lambda e, name=name: local_apply(e, src=name, adjust="shift"))
refuse("ca_local_apply-context-out", ANOTHER.format("sd_ca_local_apply", "out"), lambda e: local_apply(e, out=other(e).out(TQ, CELLS)))
refuse("ca_local_apply-order-F-cell_of", FINE_WORDS, lambda e: local_apply(e, F="F", cell_of="WC"))
refuse("ca_local_apply-order-cell_of-local_idx", "cell_of: expected", lambda e: local_apply(e, cell_of="WC", local_idx="dSTATUS"))
refuse("ca_local_apply-order-local_idx-adjust", "local_idx: expected the int32", lambda e: local_apply(e, local_idx="dSTATUS", adjust="add"))
refuse("ca_local_apply-order-local_idx_dtype-adjust", "local_idx: expected a contiguous int32", lambda e: local_apply(e, local_idx="dDIST", adjust="add"))
refuse("ca_local_apply-order-adjust-max_scale", "adjust='add'", lambda e: local_apply(e, adjust="add", max_scale=-1))
refuse("ca_local_apply-order-max_scale-L", "max_scale = -1", lambda e: local_apply(e, L=None, adjust="shift", max_scale=-1))
refuse("ca_local_apply-order-L-Q", "L: adjust='shift' needs", lambda e: local_apply(e, L=None, Q=None, adjust="shift"))
refuse("ca_local_apply-order-Q-rows", "Q: adjust='shift' needs", lambda e: local_apply(e, Q=None, adjust="shift", q0=3, q1=2))
refuse("ca_local_apply-order-rows-out", "rows .3, 2. lie outside", lambda e: local_apply(e, q0=3, q1=2, out=e.out(1, 1)))
refuse("ca_local_apply-order-out-context", "out: expected a float64 DeviceArray", lambda e: local_apply(e, src="dF", out=e.out(1, 1)))

# regridding and remapping
refuse("regrid_apply-src-shape", r"src: expected a \[T, 3, 4\] field, got shape \(4, 12\)", lambda e: e.state("regrid").apply(e.FINE))
refuse("regrid_apply-src-no_rows", r"src: expected a \[T, 3, 4\] field, got shape \(0, 3, 4\)", lambda e: e.state("regrid").apply(np.zeros((0, 3, 4))))
refuse("regrid_apply-src-dtype", "src: expected a contiguous float32 or float64 DeviceArray", lambda e: e.state("regrid").apply(i64(e, "i", (TQ, 3, 4))))
refuse("regrid_apply-src-pitch", "src: expected a contiguous float32 or float64 DeviceArray", lambda e: e.state("regrid").apply(e.dSRC))
refuse("regrid_apply-out", r"out: expected a float64 DeviceArray of shape \(4, 30\)", lambda e: e.state("regrid").apply(e.dSRC_WHOLE, out=e.out(TQ, 12)))
refuse("regrid_apply_host-src-shape", r"src: expected a \[T, 3, 4\] field, got shape \(4, 12\)", lambda e: e.state("regrid").apply_host(e.FINE))
refuse("regrid_apply_host-resident", "apply_host: expected a host array", lambda e: e.state("regrid").apply_host(e.dSRC_WHOLE))
refuse("regrid_apply_host-order-src-resident", "src: expected a contiguous", lambda e: e.state("regrid").apply_host(e.dSRC))
refuse("rule_regrid_apply-context-src", ANOTHER.format("sd_regrid", "src"), lambda e: e.state("regrid").apply(other(e).dSRC_WHOLE))
refuse("rule_regrid_apply-context-out", ANOTHER.format("sd_regrid", "out"), lambda e: e.state("regrid").apply(e.SRC, out=other(e).out(TQ, 30)))
refuse("remap_apply-field-shape", r"field: expected a float32 or float64 \[T, 3, 4\] or \[T, 12\] field, got shape \(24, 8\) of float64", lambda e: e.state("remap").apply(e.A))
refuse("remap_apply-field-dtype", r"field: expected a float32 or float64 \[T, 3, 4\] or \[T, 12\] field, got shape \(4, 12\) of int64",
       lambda e: e.state("remap").apply(i64(e, "i", (TQ, 12))))
refuse("remap_apply-field-resident_3d", r"field: expected a float32 or float64 \[T, 3, 4\] or \[T, 12\] field, got shape \(4, 3, 4\)",
       lambda e: e.state("remap").apply(e.dSRC_WHOLE))
for min_valid in (-0.5, 1.5, np.nan):
    refuse(f"remap_apply-min_valid-{min_valid}", rf"min_valid={min_valid!r}: expected a share of the covered area in \[0, 1\]",
           lambda e, min_valid=min_valid: e.state("remap").apply(e.SRC, min_valid))
refuse("remap_apply-out", r"out: expected a float64 DeviceArray of shape \(4, 4\)", lambda e: e.state("remap").apply(e.dFINE, out=e.out(TQ, 12)))
refuse("remap_apply-context-field", ANOTHER.format("sd_remap", "field"), lambda e: e.state("remap").apply(other(e).dFINE))
refuse("remap_apply-context-out", ANOTHER.format("sd_remap", "out"), lambda e: e.state("remap").apply(e.SRC, out=other(e).out(TQ, 4)))
refuse("remap_apply_host-resident", "apply_host: expected a host array", lambda e: e.state("remap").apply_host(e.dFINE))
refuse("remap_apply_host-field-shape", "field: expected a float32 or float64", lambda e: e.state("remap").apply_host(e.A))
refuse("remap_apply_host-min_valid", "min_valid=2.0", lambda e: e.state("remap").apply_host(e.SRC, 2))
refuse("remap_apply-order-field-min_valid", "field: expected", lambda e: e.state("remap").apply(e.A, 2))
refuse("remap_apply-order-min_valid-out", "min_valid=2.0", lambda e: e.state("remap").apply(e.dFINE, 2, out=e.out(1, 1)))
refuse("remap_apply-order-out-context", "out: expected a float64 DeviceArray", lambda e: e.state("remap").apply(other(e).dFINE, out=e.out(1, 1)))
refuse("remap_apply_host-order-resident-field", "apply_host: expected a host array", lambda e: e.state("remap").apply_host(e.dA))

REACHED = {'ca_apply-context-F': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_apply-context-idx': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_apply-context-weights': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_local-context-L': ([],
                        [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('Q', 0), 256]),
                         ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_local-context-Q': ([],
                        [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                         ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_local-context-idx': ([],
                          [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                           ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_local_apply-context-F': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_local_apply-context-L': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_local_apply-context-Q': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_local_apply-context-cell_of': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_local_apply-context-local_idx': ([], [('sd_dev_alloc', ['ctx', 256, '&'])]),
 'ca_select-context-L': ([],
                         [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('Q', 0), 256]),
                          ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_select-context-Q': ([],
                         [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                          ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_weights-context-L': ([],
                          [('sd_dev_alloc', ['ctx', 256, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('Q', 0), 256]),
                           ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_weights-context-Q': ([],
                          [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                           ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_weights-context-dist': ([],
                             [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                              ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_weights-context-idx': ([],
                            [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                             ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'ca_weights-context-status': ([],
                               [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('L', 0), 384]),
                                ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'disaggregate-context-climo': ([],
                                [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 128, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TARGET', 0), 128]), ('sd_dev_alloc', ['ctx', 768, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('A32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                 ('sd_dev_free', ['ctx', ('block2', 0)])]),
 'disaggregate-context-obs': ([],
                              [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 128, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TARGET', 0), 128]), ('sd_dev_alloc', ['ctx', 192, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                               ('sd_dev_free', ['ctx', ('block2', 0)])]),
 'disaggregate-context-out': ([],
                              [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('TARGET', 0), 128]),
                               ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]),
                               ('sd_dev_alloc', ['ctx', 192, '&']), ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]),
                               ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                               ('sd_dev_free', ['ctx', ('block2', 0)])]),
 'disaggregate-context-target': ([],
                                 [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                                  ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A32', 0), 768]), ('sd_dev_alloc', ['ctx', 192, '&']),
                                  ('sd_memcpy_h2d', ['ctx', ('block2', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)]),
                                  ('sd_dev_free', ['ctx', ('block2', 0)])]),
 'groupby_apply-context-field': ([],
                                 [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 192, '&']),
                                  ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB', 0), 192]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'groupby_apply-context-out': ([],
                               [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                                ('sd_dev_alloc', ['ctx', 192, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB', 0), 192]),
                                ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'groupby_apply-context-table': ([],
                                 [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                  ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'groupby_reduce-context-count': ([],
                                  [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                   ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'groupby_reduce-context-field': ([], [('sd_dev_alloc', ['ctx', 192, '&'])]),
 'groupby_reduce-context-out': ([],
                                [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                                 ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'groupby_reduce-context-sum': ([],
                                [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'groupby_reduce-order-out-context': ([], [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&'])]),
 'groupby_reduce-out': ([], [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 96, '&'])]),
 'quantile-context-field': ([], [('sd_dev_alloc', ['ctx', 64, '&'])]),
 'quantile-context-out': ([],
                          [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                           ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'remap_apply-context-field': ([], [('sd_dev_alloc', ['ctx', 128, '&'])]),
 'remap_apply-context-out': ([],
                             [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                              ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'resample-context-field': ([], [('sd_dev_alloc', ['ctx', 128, '&'])]),
 'resample-context-out': ([],
                          [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                           ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'rolling-context-field': ([], [('sd_dev_alloc', ['ctx', 1536, '&'])]),
 'rolling-context-out': ([],
                         [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                          ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'rule_regrid_apply-context-out': ([],
                                   [('sd_dev_alloc', ['ctx', 384, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('SRC', 0), 384]),
                                    ('sd_dev_free', ['ctx', ('block0', 0)])]),
 'rule_regrid_apply-context-src': ([], [('sd_dev_alloc', ['ctx', 960, '&'])]),
 'skill-context-a': ([],
                     [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                      ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'skill-context-b': ([],
                     [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                      ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'skill-context-out': ([],
                       [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                        ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]),
                        ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'skill_groups-context-a': ([],
                            [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                             ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'skill_groups-context-b': ([],
                            [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                             ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'skill_groups-context-out': ([],
                              [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                               ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]),
                               ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'spells-context-field': ([], [('sd_dev_alloc', ['ctx', 128, '&'])]),
 'spells-context-out': ([],
                        [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                         ('sd_dev_alloc', ['ctx', 64, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('TAB1', 0), 64]),
                         ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'spells-context-threshold': ([],
                              [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                               ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample-context-a': ([],
                         [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample-context-b': ([],
                         [('sd_dev_alloc', ['ctx', 128, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                          ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample-context-out': ([],
                           [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                            ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]),
                            ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample_groups-context-a': ([],
                                [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 768, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample_groups-context-b': ([],
                                [('sd_dev_alloc', ['ctx', 192, '&']), ('sd_dev_alloc', ['ctx', 1536, '&']),
                                 ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('A', 0), 1536]), ('sd_dev_free', ['ctx', ('block1', 0)])]),
 'twosample_groups-context-out': ([],
                                  [('sd_dev_alloc', ['ctx', 1536, '&']), ('sd_memcpy_h2d', ['ctx', ('block0', 0), ('A', 0), 1536]),
                                   ('sd_dev_alloc', ['ctx', 768, '&']), ('sd_memcpy_h2d', ['ctx', ('block1', 0), ('B32', 0), 768]),
                                   ('sd_dev_free', ['ctx', ('block0', 0)]), ('sd_dev_free', ['ctx', ('block1', 0)])])}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    call, words = REFUSALS[name]
    e = Engine()
    with pytest.raises((ValueError, NotImplementedError), match=words) as caught:  # noqa: F841  (held, as in test_failure_frees)
        call(e)
    log = [entry for entry in e.lib.log if not entry[0].endswith("_info")]
    assert (log, e.lib.traffic) == REACHED.get(name, ([], []))  # (not in REACHED: nothing had reached the library)
