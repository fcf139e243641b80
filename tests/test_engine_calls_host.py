"""CPU: what every estimator wrapper of engine.py hands to the C ABI, pinned on the stand-in library of tests/_recording_lib.py (no
library, no GPU): the entry point and the full argument list of each call in its host form and in its resident form on ``.cells()``
views whose pitch (12) is larger than their cells (8); what ``info()``, ``status()``, ``export()`` and ``close()`` of the state classes
call and give back; and every refusal, after which nothing but ``*_info`` calls may have reached the library.

The call lists in ``CALLS`` are written out literally, argument by argument in the order of include/sd_downscale.h: ``(name, offset)`` is
a pointer ``offset`` elements into the registered array ``name`` (``block<n>``: the n-th device allocation of the call, offset in bytes),
``"mem"`` a temporary of the wrapper (cell status, a fresh host result), ``"&"`` an output taken with ``byref``.  They are the lists the
wrappers produced before they got their shared argument layer, so they hold on both sides of that change.  The cases whose id carries
``rule_out``, ``rule_residency``, ``rule_dtype``, ``new_status`` or ``new_order`` (a refusal that used to come after a first call into the
library) pin what that change introduced (``-k`` deselects them)."""
import numpy as np
import pytest

from _recording_lib import context

T, TQ, F, CELLS, LD, C0, K, G = 24, 6, 2, 8, 12, 2, 3, 12
INFO = {  # what the ``*_info`` entry point of each family writes here, in the order of its outputs
    "bcsd": ("sd_bcsd_state_info", (0, G, T, CELLS, 1)),
    "qm": ("sd_qm_state_info", (T, CELLS)),
    "analog": ("sd_analog_state_info", (T, F, CELLS)),
    "linreg": ("sd_linreg_state_info", (T, F, CELLS)),
    "zscore": ("sd_zscore_state_info", (5, CELLS, 3)),
    "grouped": ("sd_grouped_state_info", (4, F, CELLS, 1)),
    "arrm": ("sd_arrm_state_info", (4, CELLS, T)),
    "regrid": ("sd_regrid_info", (0, 3, 4, 5, 6)),
    "remap": ("sd_remap_info", (3, 4, 2, 2, 7, 9)),
}
HOST_SHAPES = dict(X2=(T, CELLS), Y2=(T, CELLS), XP2=(TQ, CELLS), X3=(T, F, CELLS), XQ3=(TQ, F, CELLS), OUT2=(TQ, CELLS), OUT3=(TQ, 3, CELLS))


class Engine:
    """a recording context with the arrays of the cases: host ones by their names, resident ones (``d`` + name) as the cells 2 .. 9 of
    made-up arrays 12 cells wide"""

    def __init__(self):
        self.ctx = context()
        self.lib = self.ctx.lib
        self.states = []
        for name, shape in HOST_SHAPES.items():
            setattr(self, name, self.lib.host(name, np.zeros(shape)))
            setattr(self, "d" + name, self.wide(self.ctx, "d" + name, shape))
        ints = dict(GID=np.arange(T) % G, GIDQ=np.arange(TQ) % G, GIDT=np.arange(TQ) % 2, ORDER=np.arange(T), KEY=np.arange(T) % 4,
                    KEYQ=np.arange(TQ) % 4, DAY=np.arange(T) % 5, YEAR=np.arange(T) // 5, SAMP=np.ones((TQ, CELLS)))
        for name, a in ints.items():
            setattr(self, name, self.lib.host(name, np.ascontiguousarray(a, dtype=np.int32)))
        self.OFFSETS = self.lib.host("OFFSETS", np.array([0, 12, T], dtype=np.int64))
        self.dSAMP = self.lib.resident(self.ctx, "dSAMP", (TQ, CELLS), np.int32)

    def wide(self, ctx, name, shape, dtype=np.float64):
        return self.lib.resident(ctx, name, shape[:-1] + (LD,), dtype).cells(C0, C0 + CELLS)

    def a(self, form, name):
        return None if name is None else getattr(self, name if form == "host" else "d" + name)

    def fitted(self, family):
        """a state of the family (made through its fit or create entry point, which is then forgotten)"""
        name, values = INFO[family]
        self.lib.info[name] = values
        c = self.ctx
        state = dict(bcsd=lambda: c.bcsd_fit(0, self.X2, self.Y2, self.GID, G), qm=lambda: c.qm_fit(self.X2, self.Y2),
                     analog=lambda: c.analog_fit(self.X3, self.Y2), linreg=lambda: c.linreg_fit(self.X3, self.Y2),
                     zscore=lambda: c.zscore_fit(self.X2, self.Y2, 3, self.DAY, self.YEAR, 5),
                     grouped=lambda: c.grouped_fit(self.X3, self.Y2, self.KEY, 4, 1), arrm=lambda: c.arrm_fit(self.X2, self.Y2, 1),
                     regrid=lambda: c.regrid_create(np.arange(3.0), np.arange(4.0), np.arange(5.0), np.arange(6.0)),
                     remap=lambda: c.remap_create(np.arange(4.0), np.arange(5.0), np.arange(3.0), np.arange(3.0)))[family]()
        self.lib.log.clear()
        self.states.append(state)  # (kept: a state that goes away calls its destroy entry point)
        return state

    def reached(self):
        """what reached the library apart from reading a state's sizes"""
        return [name for name, _ in self.lib.log if not name.endswith("_info")] + [name for name, _ in self.lib.traffic]


FORMS = ("host", "res")
CASES = {}


def case(name):
    def add(fn):
        CASES[name] = fn
        return fn
    return add


for form in FORMS:
    for X in ("X2", None):
        for detrend in (False, True):
            CASES[f"bcsd_fit-{form}-{X}-detrend{int(detrend)}"] = lambda e, form=form, X=X, detrend=detrend: e.ctx.bcsd_fit(
                int(X is None), e.a(form, X), e.a(form, "Y2"), e.GID, G, True, detrend)
    CASES[f"bcsd_fit_groups-{form}"] = lambda e, form=form: e.ctx.bcsd_fit_groups(0, e.a(form, "X2"), e.a(form, "Y2"), e.ORDER, e.OFFSETS, False)
    CASES[f"bcsd_predict-{form}"] = lambda e, form=form: e.ctx.bcsd_predict(e.fitted("bcsd"), e.a(form, "XP2"), e.GIDQ, out=e.a(form, "OUT2"))
    CASES[f"bcsd_predict_trend-{form}"] = lambda e, form=form: e.ctx.bcsd_predict_trend(e.fitted("bcsd"), e.a(form, "XP2"), e.GIDQ, e.GIDT, 2,
                                                                                        out=e.a(form, "OUT2"))
    for y in ("Y2", None):
        CASES[f"qm_fit-{form}-{y}"] = lambda e, form=form, y=y: e.ctx.qm_fit(e.a(form, "X2"), e.a(form, y))
    for ex in ("both", "min", "max", "1to1", None):
        CASES[f"qm_cunnane-{form}-{ex}"] = lambda e, form=form, ex=ex: e.ctx.qm_cunnane(e.fitted("qm"), 1, e.a(form, "XP2"), ex, 7)
    for ex in ("both", "min", "max", "1to1", None, True, False):
        CASES[f"qm_predict-{form}-{ex}"] = lambda e, form=form, ex=ex: e.ctx.qm_predict(e.fitted("qm"), 2, e.a(form, "XP2"), ex, 7)
    CASES[f"analog_fit-{form}"] = lambda e, form=form: e.ctx.analog_fit(e.a(form, "X3"), e.a(form, "Y2"))
    CASES[f"analog_fit_predict-{form}"] = lambda e, form=form: e.ctx.analog_fit_predict(e.a(form, "X3"), e.a(form, "Y2"), e.a(form, "XQ3"), K, 3, 0.5,
                                                                                        out=e.a(form, "OUT3"))
    for thresh in (None, 0.25):
        CASES[f"analog_predict-{form}-thresh{thresh}"] = lambda e, form=form, thresh=thresh: e.ctx.analog_predict(
            e.fitted("analog"), e.a(form, "XQ3"), K, 3, thresh)
        CASES[f"analogreg_predict-{form}-thresh{thresh}"] = lambda e, form=form, thresh=thresh: e.ctx.analogreg_predict(
            e.fitted("analog"), e.a(form, "XQ3"), K, thresh)
        CASES[f"linreg_fit-{form}-thresh{thresh}"] = lambda e, form=form, thresh=thresh: e.ctx.linreg_fit(e.a(form, "X3"), e.a(form, "Y2"), thresh)
    CASES[f"analog_predict-{form}-host_sample_inds"] = lambda e, form=form: e.ctx.analog_predict(e.fitted("analog"), e.a(form, "XQ3"), K, 1,
                                                                                                 sample_inds=e.SAMP)
    CASES[f"analog_predict-{form}-neighbors"] = lambda e, form=form: e.ctx.analog_predict(e.fitted("analog"), e.a(form, "XQ3"), K, 3,
                                                                                          want_neighbors=True)
    CASES[f"linreg_predict-{form}"] = lambda e, form=form: e.ctx.linreg_predict(e.fitted("linreg"), e.a(form, "XQ3"))
    CASES[f"zscore_fit-{form}"] = lambda e, form=form: e.ctx.zscore_fit(e.a(form, "X2"), e.a(form, "Y2"), 3, e.DAY, e.YEAR, 5)
    for stats in (False, True):
        CASES[f"zscore_predict-{form}-stats{int(stats)}"] = lambda e, form=form, stats=stats: e.ctx.zscore_predict(
            e.fitted("zscore"), e.a(form, "XP2"), with_stats=stats)
    CASES[f"grouped_fit-{form}"] = lambda e, form=form: e.ctx.grouped_fit(e.a(form, "X3"), e.a(form, "Y2"), e.KEY, 4, 1)
    CASES[f"grouped_predict-{form}"] = lambda e, form=form: e.ctx.grouped_predict(e.fitted("grouped"), e.a(form, "XQ3"), e.KEYQ, out=e.a(form, "OUT2"))
    for r2 in (False, True):
        CASES[f"arrm_fit-{form}-r2{int(r2)}"] = lambda e, form=form, r2=r2: e.ctx.arrm_fit(e.a(form, "X2"), e.a(form, "Y2"), 2, r2)
    CASES[f"arrm_predict-{form}"] = lambda e, form=form: e.ctx.arrm_predict(e.fitted("arrm"), e.a(form, "XP2"), out=e.a(form, "OUT2"))
CASES["analog_predict-res-resident_sample_inds"] = lambda e: e.ctx.analog_predict(e.fitted("analog"), e.dXQ3, K, 1, sample_inds=e.dSAMP,
                                                                                  out=e.dOUT3)
CASES["bcsd_fit_predict-X"] = lambda e: e.ctx.bcsd_fit_predict(0, e.dX2, e.dY2, e.GID, G, e.dXP2, e.GIDQ, True, e.dOUT2, True)
CASES["bcsd_fit_predict-noX"] = lambda e: e.ctx.bcsd_fit_predict(1, None, e.dY2, e.GID, G, e.dXP2, e.GIDQ, False)


def exported(e, family, **more):
    """what ``export()`` of the family gives, as registered host arrays of the right shapes"""
    shapes = dict(
        bcsd=dict(y_sorted=(CELLS, T), x_climo=(CELLS, G), y_climo=(CELLS, G), y_trend=(CELLS, G, 2)),
        linreg=dict(coef=(F, CELLS), intercept=(CELLS,), fit_error=(CELLS,), logistic_coef=(F, CELLS), logistic_intercept=(CELLS,)),
        zscore={k: (5, CELLS) for k in ("x_mean", "x_std", "y_mean", "y_std", "shift", "scale")},
        grouped=dict(coef=(4, F, CELLS), intercept=(4, CELLS)),
        arrm=dict(breaks=(4, CELLS), beta=(4, CELLS), ssr=(CELLS,)))[family]
    d = {k: e.lib.host(k, np.zeros(s)) for k, s in shapes.items()}
    d["status"] = e.lib.host("status", np.zeros(CELLS, dtype=np.int32))
    return dict(d, **more)


@case("bcsd_import-plain")
def _(e):
    d = exported(e, "bcsd", info=dict(kind=1, G=G, T=T, C=CELLS, return_anoms=True), group_offsets=e.lib.host("offs", np.arange(G + 1)))
    e.ctx.bcsd_import(d)


@case("bcsd_import-trend")
def _(e):
    d = exported(e, "bcsd", info=dict(kind=0, G=G, T=T, C=CELLS, return_anoms=False, detrend=True),
                 group_offsets=e.lib.host("offs", np.arange(G + 1)))
    e.ctx.bcsd_import(d)


@case("linreg_import-plain")
def _(e):
    d = exported(e, "linreg", T=T)
    del d["logistic_coef"], d["logistic_intercept"]
    e.ctx.linreg_import(d)


@case("linreg_import-logistic")
def _(e):
    e.ctx.linreg_import(exported(e, "linreg", T=T, thresh_dropped=e.lib.host("dropped", np.zeros(CELLS, dtype=np.int32))))


@case("zscore_import")
def _(e):
    e.ctx.zscore_import(exported(e, "zscore", window_width=3))


@case("grouped_import")
def _(e):
    e.ctx.grouped_import(exported(e, "grouped", window=1, fitted=e.lib.host("fitted", np.ones(4, dtype=np.int32))))


@case("arrm_import")
def _(e):
    e.ctx.arrm_import(exported(e, "arrm", T=T, break_index=e.lib.host("break_index", np.zeros((4, CELLS), dtype=np.int32))))


@case("regrid_create")
def _(e):
    sy, sx, dy, dx = (e.lib.host(n, np.arange(float(k))) for n, k in (("sy", 3), ("sx", 4), ("dy", 5), ("dx", 6)))
    e.ctx.regrid_create(sy, sx, dy, dx, "nearest")


@case("remap_create")
def _(e):
    syb, sxb, dyb, dxb = (e.lib.host(n, np.arange(float(k))) for n, k in (("syb", 4), ("sxb", 5), ("dyb", 3), ("dxb", 2)))
    e.ctx.remap_create(syb, sxb, dyb, dxb)


# ---- the state classes ----
for family in INFO:
    CASES[f"info-{family}"] = lambda e, family=family: e.fitted(family).info()
    CASES[f"close-{family}"] = lambda e, family=family: e.fitted(family).close()
for family in ("bcsd", "zscore", "grouped", "arrm"):
    CASES[f"status-{family}"] = lambda e, family=family: e.fitted(family).status()
for family in ("linreg", "qm"):
    CASES[f"status-{family}-new_status"] = lambda e, family=family: e.fitted(family).status()
for family in ("bcsd", "linreg", "zscore", "grouped", "arrm", "qm"):
    CASES[f"export-{family}"] = lambda e, family=family: e.fitted(family).export()
CASES["export-qm-without_y"] = lambda e: e.fitted("qm").export(with_y=False)
CASES["fitted-grouped"] = lambda e: e.fitted("grouped").fitted()

CALLS = {'analog_fit-host': [('sd_analog_fit', ['ctx', ('X3', 0), ('Y2', 0), 24, 2, 8, '&'])],
 'analog_fit-res': [('sd_analog_fit_dev', ['ctx', ('dX3', 2), ('dY2', 2), 12, 24, 2, 8, '&'])],
 'analog_fit_predict-host': [('sd_analog_fit_predict', ['ctx', ('X3', 0), ('Y2', 0), 24, 2, 8, ('XQ3', 0), 6, 3, 3, 1, 0.5, ('OUT3', 0), 'mem'])],
 'analog_fit_predict-res': [('sd_analog_fit_predict_dev',
                             ['ctx', ('dX3', 2), ('dY2', 2), 12, 24, 2, 8, ('dXQ3', 2), 12, 6, 3, 3, 1, 0.5, ('dOUT3', 2), 12, 'mem'])],
 'analog_predict-host-host_sample_inds': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                          ('sd_analog_predict',
                                           ['ctx', 'state0', ('XQ3', 0), 6, 3, 1, 0, 0.0, ('SAMP', 0), 'mem', None, None, 'mem'])],
 'analog_predict-host-neighbors': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                   ('sd_analog_predict', ['ctx', 'state0', ('XQ3', 0), 6, 3, 3, 0, 0.0, None, 'mem', 'mem', 'mem', 'mem'])],
 'analog_predict-host-thresh0.25': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                    ('sd_analog_predict', ['ctx', 'state0', ('XQ3', 0), 6, 3, 3, 1, 0.25, None, 'mem', None, None, 'mem'])],
 'analog_predict-host-threshNone': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                    ('sd_analog_predict', ['ctx', 'state0', ('XQ3', 0), 6, 3, 3, 0, 0.0, None, 'mem', None, None, 'mem'])],
 'analog_predict-res-host_sample_inds': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                         ('sd_analog_predict_dev',
                                          ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 1, 0, 0.0, ('block1', 0), ('block0', 0), 8, None, None, 'mem'])],
 'analog_predict-res-neighbors': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                  ('sd_analog_predict_dev',
                                   ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 3, 0, 0.0, None, ('block0', 0), 8, ('block1', 0), ('block2', 0), 'mem'])],
 'analog_predict-res-resident_sample_inds': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                             ('sd_analog_predict_dev',
                                              ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 1, 0, 0.0, ('dSAMP', 0), ('dOUT3', 2), 12, None, None,
                                               'mem'])],
 'analog_predict-res-thresh0.25': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                   ('sd_analog_predict_dev',
                                    ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 3, 1, 0.25, None, ('block0', 0), 8, None, None, 'mem'])],
 'analog_predict-res-threshNone': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                   ('sd_analog_predict_dev',
                                    ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 3, 0, 0.0, None, ('block0', 0), 8, None, None, 'mem'])],
 'analogreg_predict-host-thresh0.25': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                       ('sd_analogreg_predict', ['ctx', 'state0', ('XQ3', 0), 6, 3, 1, 0.25, 'mem', 'mem'])],
 'analogreg_predict-host-threshNone': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                       ('sd_analogreg_predict', ['ctx', 'state0', ('XQ3', 0), 6, 3, 0, 0.0, 'mem', 'mem'])],
 'analogreg_predict-res-thresh0.25': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                      ('sd_analogreg_predict_dev', ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 1, 0.25, ('block0', 0), 8, 'mem'])],
 'analogreg_predict-res-threshNone': [('sd_analog_state_info', ['state0', '&', '&', '&']),
                                      ('sd_analogreg_predict_dev', ['ctx', 'state0', ('dXQ3', 2), 12, 6, 3, 0, 0.0, ('block0', 0), 8, 'mem'])],
 'arrm_fit-host-r20': [('sd_arrm_fit', ['ctx', ('X2', 0), ('Y2', 0), 24, 8, 2, None, '&'])],
 'arrm_fit-host-r21': [('sd_arrm_fit', ['ctx', ('X2', 0), ('Y2', 0), 24, 8, 2, 'mem', '&'])],
 'arrm_fit-res-r20': [('sd_arrm_fit_dev', ['ctx', ('dX2', 2), ('dY2', 2), 12, 24, 8, 2, None, '&'])],
 'arrm_fit-res-r21': [('sd_arrm_fit_dev', ['ctx', ('dX2', 2), ('dY2', 2), 12, 24, 8, 2, ('block0', 0), '&'])],
 'arrm_import': [('sd_arrm_state_import', ['ctx', 4, 8, 24, ('breaks', 0), ('break_index', 0), ('beta', 0), ('ssr', 0), ('status', 0), '&']),
                 ('sd_arrm_state_destroy', ['state0'])],
 'arrm_predict-host': [('sd_arrm_state_info', ['state0', '&', '&', '&']), ('sd_arrm_predict', ['ctx', 'state0', ('XP2', 0), 6, ('OUT2', 0), 'mem'])],
 'arrm_predict-res': [('sd_arrm_state_info', ['state0', '&', '&', '&']),
                      ('sd_arrm_predict_dev', ['ctx', 'state0', ('dXP2', 2), 12, 6, ('dOUT2', 2), 12, 'mem'])],
 'bcsd_fit-host-None-detrend0': [('sd_bcsd_fit', ['ctx', 1, None, ('Y2', 0), ('GID', 0), 12, 24, 8, 1, '&'])],
 'bcsd_fit-host-None-detrend1': [('sd_bcsd_fit', ['ctx', 1, None, ('Y2', 0), ('GID', 0), 12, 24, 8, 3, '&'])],
 'bcsd_fit-host-X2-detrend0': [('sd_bcsd_fit', ['ctx', 0, ('X2', 0), ('Y2', 0), ('GID', 0), 12, 24, 8, 1, '&'])],
 'bcsd_fit-host-X2-detrend1': [('sd_bcsd_fit', ['ctx', 0, ('X2', 0), ('Y2', 0), ('GID', 0), 12, 24, 8, 3, '&'])],
 'bcsd_fit-res-None-detrend0': [('sd_bcsd_fit_dev', ['ctx', 1, None, ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 1, '&'])],
 'bcsd_fit-res-None-detrend1': [('sd_bcsd_fit_dev', ['ctx', 1, None, ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 3, '&'])],
 'bcsd_fit-res-X2-detrend0': [('sd_bcsd_fit_dev', ['ctx', 0, ('dX2', 2), ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 1, '&'])],
 'bcsd_fit-res-X2-detrend1': [('sd_bcsd_fit_dev', ['ctx', 0, ('dX2', 2), ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 3, '&'])],
 'bcsd_fit_groups-host': [('sd_bcsd_fit_groups', ['ctx', 0, ('X2', 0), ('Y2', 0), ('ORDER', 0), ('OFFSETS', 0), 2, 24, 8, 0, '&'])],
 'bcsd_fit_groups-res': [('sd_bcsd_fit_groups_dev', ['ctx', 0, ('dX2', 2), ('dY2', 2), 12, ('ORDER', 0), ('OFFSETS', 0), 2, 24, 8, 0, '&'])],
 'bcsd_fit_predict-X': [('sd_bcsd_fit_predict_dev',
                         ['ctx', 0, ('dX2', 2), ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 3, ('dXP2', 2), 12, ('GIDQ', 0), 6, ('dOUT2', 2), 12, 'mem'])],
 'bcsd_fit_predict-noX': [('sd_bcsd_fit_predict_dev',
                           ['ctx', 1, None, ('dY2', 2), 12, ('GID', 0), 12, 24, 8, 0, ('dXP2', 2), 12, ('GIDQ', 0), 6, ('block0', 0), 8, 'mem'])],
 'bcsd_import-plain': [('sd_bcsd_state_import',
                        ['ctx', 1, 12, 24, 8, 1, ('y_sorted', 0), ('x_climo', 0), ('y_climo', 0), ('status', 0), ('offs', 0), '&']),
                       ('sd_bcsd_state_destroy', ['state0'])],
 'bcsd_import-trend': [('sd_bcsd_state_import',
                        ['ctx', 0, 12, 24, 8, 2, ('y_sorted', 0), ('x_climo', 0), ('y_climo', 0), ('status', 0), ('offs', 0), '&']),
                       ('sd_bcsd_state_set_trend', ['state0', ('y_trend', 0)]), ('sd_bcsd_state_destroy', ['state0'])],
 'bcsd_predict-host': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']),
                       ('sd_bcsd_predict', ['ctx', 'state0', ('XP2', 0), ('GIDQ', 0), 6, ('OUT2', 0), 'mem'])],
 'bcsd_predict-res': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']),
                      ('sd_bcsd_predict_dev', ['ctx', 'state0', ('dXP2', 2), 12, ('GIDQ', 0), 6, ('dOUT2', 2), 12, 'mem'])],
 'bcsd_predict_trend-host': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']),
                             ('sd_bcsd_predict_trend', ['ctx', 'state0', ('XP2', 0), ('GIDQ', 0), ('GIDT', 0), 2, 6, ('OUT2', 0), 'mem'])],
 'bcsd_predict_trend-res': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']),
                            ('sd_bcsd_predict_trend_dev',
                             ['ctx', 'state0', ('dXP2', 2), 12, ('GIDQ', 0), ('GIDT', 0), 2, 6, ('dOUT2', 2), 12, 'mem'])],
 'close-analog': [('sd_analog_state_destroy', ['state0'])],
 'close-arrm': [('sd_arrm_state_destroy', ['state0'])],
 'close-bcsd': [('sd_bcsd_state_destroy', ['state0'])],
 'close-grouped': [('sd_grouped_state_destroy', ['state0'])],
 'close-linreg': [('sd_linreg_state_destroy', ['state0'])],
 'close-qm': [('sd_qm_state_destroy', ['state0'])],
 'close-regrid': [('sd_regrid_destroy', ['state0'])],
 'close-remap': [('sd_remap_destroy', ['state0'])],
 'close-zscore': [('sd_zscore_state_destroy', ['state0'])],
 'export-arrm': [('sd_arrm_state_info', ['state0', '&', '&', '&']), ('sd_arrm_state_export', ['state0', 'mem', 'mem', 'mem', 'mem', 'mem'])],
 'export-bcsd': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']),
                 ('sd_bcsd_state_export', ['state0', 'mem', 'mem', 'mem', 'mem', 'mem'])],
 'export-grouped': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&']), ('sd_grouped_state_export', ['state0', 'mem', 'mem', 'mem', 'mem'])],
 'export-linreg': [('sd_linreg_state_info', ['state0', '&', '&', '&']),
                   ('sd_linreg_state_export', ['state0', 'mem', 'mem', 'mem', 'mem', 'mem', 'mem'])],
 'export-qm': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_state_export', ['state0', 'mem', 'mem', 'mem'])],
 'export-qm-without_y': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_state_export', ['state0', 'mem', None, 'mem'])],
 'export-zscore': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                   ('sd_zscore_state_export', ['state0', 'mem', 'mem', 'mem', 'mem', 'mem', 'mem', 'mem'])],
 'fitted-grouped': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&']), ('sd_grouped_state_export', ['state0', None, None, 'mem', None])],
 'grouped_fit-host': [('sd_grouped_fit', ['ctx', ('X3', 0), ('Y2', 0), 24, 2, 8, ('KEY', 0), 4, 1, '&'])],
 'grouped_fit-res': [('sd_grouped_fit_dev', ['ctx', ('dX3', 2), ('dY2', 2), 12, 24, 2, 8, ('KEY', 0), 4, 1, '&'])],
 'grouped_import': [('sd_grouped_state_import', ['ctx', 4, 2, 8, 1, ('coef', 0), ('intercept', 0), ('fitted', 0), ('status', 0), '&']),
                    ('sd_grouped_state_destroy', ['state0'])],
 'grouped_predict-host': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&']),
                          ('sd_grouped_predict', ['ctx', 'state0', ('XQ3', 0), 6, ('KEYQ', 0), ('OUT2', 0), 'mem'])],
 'grouped_predict-res': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&']),
                         ('sd_grouped_predict_dev', ['ctx', 'state0', ('dXQ3', 2), 12, 6, ('KEYQ', 0), ('dOUT2', 2), 12, 'mem'])],
 'info-analog': [('sd_analog_state_info', ['state0', '&', '&', '&'])],
 'info-arrm': [('sd_arrm_state_info', ['state0', '&', '&', '&'])],
 'info-bcsd': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&'])],
 'info-grouped': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&'])],
 'info-linreg': [('sd_linreg_state_info', ['state0', '&', '&', '&'])],
 'info-qm': [('sd_qm_state_info', ['state0', '&', '&'])],
 'info-regrid': [('sd_regrid_info', ['state0', '&', '&', '&', '&', '&'])],
 'info-remap': [('sd_remap_info', ['state0', '&', '&', '&', '&', '&', '&'])],
 'info-zscore': [('sd_zscore_state_info', ['state0', '&', '&', '&'])],
 'linreg_fit-host-thresh0.25': [('sd_linreg_fit', ['ctx', ('X3', 0), ('Y2', 0), 24, 2, 8, 1, 0.25, '&'])],
 'linreg_fit-host-threshNone': [('sd_linreg_fit', ['ctx', ('X3', 0), ('Y2', 0), 24, 2, 8, 0, 0.0, '&'])],
 'linreg_fit-res-thresh0.25': [('sd_linreg_fit_dev', ['ctx', ('dX3', 2), ('dY2', 2), 12, 24, 2, 8, 1, 0.25, '&'])],
 'linreg_fit-res-threshNone': [('sd_linreg_fit_dev', ['ctx', ('dX3', 2), ('dY2', 2), 12, 24, 2, 8, 0, 0.0, '&'])],
 'linreg_import-logistic': [('sd_linreg_state_import',
                             ['ctx', 24, 2, 8, ('coef', 0), ('intercept', 0), ('fit_error', 0), 'mem', ('dropped', 0), ('status', 0), '&']),
                            ('sd_linreg_state_destroy', ['state0'])],
 'linreg_import-plain': [('sd_linreg_state_import',
                          ['ctx', 24, 2, 8, ('coef', 0), ('intercept', 0), ('fit_error', 0), None, None, ('status', 0), '&']),
                         ('sd_linreg_state_destroy', ['state0'])],
 'linreg_predict-host': [('sd_linreg_state_info', ['state0', '&', '&', '&']), ('sd_linreg_predict', ['ctx', 'state0', ('XQ3', 0), 6, 'mem', 'mem'])],
 'linreg_predict-res': [('sd_linreg_state_info', ['state0', '&', '&', '&']),
                        ('sd_linreg_predict_dev', ['ctx', 'state0', ('dXQ3', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_cunnane-host-1to1': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_cunnane', ['ctx', 'state0', 1, 0, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_cunnane-host-None': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_cunnane', ['ctx', 'state0', 1, 0, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_cunnane-host-both': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_cunnane', ['ctx', 'state0', 1, 3, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_cunnane-host-max': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_cunnane', ['ctx', 'state0', 1, 2, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_cunnane-host-min': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_cunnane', ['ctx', 'state0', 1, 1, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_cunnane-res-1to1': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_cunnane_dev', ['ctx', 'state0', 1, 0, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_cunnane-res-None': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_cunnane_dev', ['ctx', 'state0', 1, 0, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_cunnane-res-both': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_cunnane_dev', ['ctx', 'state0', 1, 3, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_cunnane-res-max': [('sd_qm_state_info', ['state0', '&', '&']),
                        ('sd_qm_cunnane_dev', ['ctx', 'state0', 1, 2, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_cunnane-res-min': [('sd_qm_state_info', ['state0', '&', '&']),
                        ('sd_qm_cunnane_dev', ['ctx', 'state0', 1, 1, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_fit-host-None': [('sd_qm_fit', ['ctx', ('X2', 0), None, 24, 8, '&'])],
 'qm_fit-host-Y2': [('sd_qm_fit', ['ctx', ('X2', 0), ('Y2', 0), 24, 8, '&'])],
 'qm_fit-res-None': [('sd_qm_fit_dev', ['ctx', ('dX2', 2), None, 12, 24, 8, '&'])],
 'qm_fit-res-Y2': [('sd_qm_fit_dev', ['ctx', ('dX2', 2), ('dY2', 2), 12, 24, 8, '&'])],
 'qm_predict-host-1to1': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 4, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-False': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 0, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-None': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 0, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-True': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 4, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-both': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 3, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-max': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 2, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-host-min': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_predict', ['ctx', 'state0', 2, 1, 7, ('XP2', 0), 6, 'mem', 'mem'])],
 'qm_predict-res-1to1': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_predict_dev', ['ctx', 'state0', 2, 4, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-False': [('sd_qm_state_info', ['state0', '&', '&']),
                          ('sd_qm_predict_dev', ['ctx', 'state0', 2, 0, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-None': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_predict_dev', ['ctx', 'state0', 2, 0, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-True': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_predict_dev', ['ctx', 'state0', 2, 4, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-both': [('sd_qm_state_info', ['state0', '&', '&']),
                         ('sd_qm_predict_dev', ['ctx', 'state0', 2, 3, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-max': [('sd_qm_state_info', ['state0', '&', '&']),
                        ('sd_qm_predict_dev', ['ctx', 'state0', 2, 2, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'qm_predict-res-min': [('sd_qm_state_info', ['state0', '&', '&']),
                        ('sd_qm_predict_dev', ['ctx', 'state0', 2, 1, 7, ('dXP2', 2), 12, 6, ('block0', 0), 8, 'mem'])],
 'regrid_create': [('sd_regrid_create', ['ctx', 1, 3, 4, ('sy', 0), ('sx', 0), 5, 6, ('dy', 0), ('dx', 0), '&']), ('sd_regrid_destroy', ['state0'])],
 'remap_create': [('sd_remap_create', ['ctx', 3, 4, ('syb', 0), ('sxb', 0), 2, 1, ('dyb', 0), ('dxb', 0), '&']), ('sd_remap_destroy', ['state0'])],
 'status-arrm': [('sd_arrm_state_info', ['state0', '&', '&', '&']), ('sd_arrm_state_export', ['state0', None, None, None, None, 'mem'])],
 'status-bcsd': [('sd_bcsd_state_info', ['state0', '&', '&', '&', '&', '&']), ('sd_bcsd_state_status', ['state0', 'mem'])],
 'status-grouped': [('sd_grouped_state_info', ['state0', '&', '&', '&', '&']), ('sd_grouped_state_export', ['state0', None, None, None, 'mem'])],
 'status-linreg-new_status': [('sd_linreg_state_info', ['state0', '&', '&', '&']),
                              ('sd_linreg_state_export', ['state0', None, None, None, None, None, 'mem'])],
 'status-qm-new_status': [('sd_qm_state_info', ['state0', '&', '&']), ('sd_qm_state_export', ['state0', None, None, 'mem'])],
 'status-zscore': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                   ('sd_zscore_state_export', ['state0', None, None, None, None, None, None, 'mem'])],
 'zscore_fit-host': [('sd_zscore_fit', ['ctx', ('X2', 0), ('Y2', 0), 24, 8, 3, ('DAY', 0), ('YEAR', 0), 5, '&'])],
 'zscore_fit-res': [('sd_zscore_fit_dev', ['ctx', ('dX2', 2), ('dY2', 2), 12, 24, 8, 3, ('DAY', 0), ('YEAR', 0), 5, '&'])],
 'zscore_import': [('sd_zscore_state_import',
                    ['ctx', 5, 8, 3, ('x_mean', 0), ('x_std', 0), ('y_mean', 0), ('y_std', 0), ('shift', 0), ('scale', 0), ('status', 0), '&']),
                   ('sd_zscore_state_destroy', ['state0'])],
 'zscore_predict-host-stats0': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                                ('sd_zscore_predict', ['ctx', 'state0', ('XP2', 0), 6, 'mem', None, None, None, None, 'mem'])],
 'zscore_predict-host-stats1': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                                ('sd_zscore_predict', ['ctx', 'state0', ('XP2', 0), 6, 'mem', 'mem', 'mem', 'mem', 'mem', 'mem'])],
 'zscore_predict-res-stats0': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                               ('sd_zscore_predict_dev', ['ctx', 'state0', ('dXP2', 2), 12, 6, ('block0', 0), 8, None, None, None, None, 'mem'])],
 'zscore_predict-res-stats1': [('sd_zscore_state_info', ['state0', '&', '&', '&']),
                               ('sd_zscore_predict_dev',
                                ['ctx', 'state0', ('dXP2', 2), 12, 6, ('block0', 0), 8, ('block1', 0), ('block2', 0), ('block3', 0), ('block4', 0),
                                 'mem'])]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls(name):
    e = Engine()
    kept = CASES[name](e)  # noqa: F841  (a state that goes away calls its destroy entry point)
    assert e.lib.log == CALLS[name]


INFOS = {
    "bcsd": dict(kind=0, G=G, T=T, C=CELLS, return_anoms=True, detrend=False),
    "qm": dict(T=T, C=CELLS),
    "analog": dict(T=T, F=F, C=CELLS),
    "linreg": dict(T=T, F=F, C=CELLS),
    "zscore": dict(K=5, C=CELLS, window_width=3),
    "grouped": dict(n=4, F=F, C=CELLS, window=1),
    "arrm": dict(B=4, C=CELLS, T=T),
    "regrid": dict(method=0, ny=3, nx=4, Ny=5, Nx=6),
    "remap": dict(ny=3, nx=4, Ny=2, Nx=2, y_entries=7, x_entries=9),
}


@pytest.mark.parametrize("family", sorted(INFOS))
def test_info_decoding(family):
    assert Engine().fitted(family).info() == INFOS[family]


@pytest.mark.parametrize("flags", range(4))
def test_bcsd_info_flags(flags):
    e = Engine()
    state = e.fitted("bcsd")
    e.lib.info["sd_bcsd_state_info"] = (1, G, T, CELLS, flags)
    assert state.info() == dict(kind=1, G=G, T=T, C=CELLS, return_anoms=bool(flags & 1), detrend=bool(flags & 2))


EXPORTS = {  # key -> (shape, dtype) of the arrays of ``export()``; the other entries are plain values
    "bcsd": dict(y_sorted=((CELLS, T), "f8"), x_climo=((CELLS, G), "f8"), y_climo=((CELLS, G), "f8"), status=((CELLS,), "i4"),
                 group_offsets=((G + 1,), "i8")),
    "linreg": dict(coef=((F, CELLS), "f8"), intercept=((CELLS,), "f8"), fit_error=((CELLS,), "f8"), status=((CELLS,), "i4")),
    "zscore": dict({k: ((5, CELLS), "f8") for k in ("x_mean", "x_std", "y_mean", "y_std", "shift", "scale")}, status=((CELLS,), "i4")),
    "grouped": dict(coef=((4, F, CELLS), "f8"), intercept=((4, CELLS), "f8"), fitted=((4,), "?"), status=((CELLS,), "i4")),
    "arrm": dict(breaks=((4, CELLS), "f8"), break_index=((4, CELLS), "i4"), beta=((4, CELLS), "f8"), ssr=((CELLS,), "f8"), status=((CELLS,), "i4")),
    "qm": dict(x_sorted=((CELLS, T), "f8"), y_sorted=((CELLS, T), "f8"), status=((CELLS,), "i4")),
}
PLAIN = dict(bcsd=dict(info=INFOS["bcsd"]), linreg=dict(T=T), zscore=dict(window_width=3), grouped=dict(window=1), arrm=dict(T=T), qm={})


@pytest.mark.parametrize("family", sorted(EXPORTS))
def test_export_keys_shapes_dtypes(family):
    got = Engine().fitted(family).export()
    assert set(got) == set(EXPORTS[family]) | set(PLAIN[family])
    for key, (shape, dtype) in EXPORTS[family].items():
        assert got[key].shape == shape and got[key].dtype == np.dtype(dtype), key
    for key, value in PLAIN[family].items():
        assert got[key] == value, key


@pytest.mark.parametrize("family", ["bcsd", "zscore", "grouped", "arrm", "linreg-new_status", "qm-new_status"])
def test_status_shape(family):
    status = Engine().fitted(family.split("-")[0]).status()
    assert status.shape == (CELLS,) and status.dtype == np.int32


@pytest.mark.parametrize("family", sorted(INFO))
def test_close_once(family):
    e = Engine()
    state = e.fitted(family)
    state.close()
    once = list(e.lib.log)
    state.close()
    assert e.lib.log == once and len(once) == 1 and once[0][1] == ["state0"]
    with pytest.raises(ValueError, match="destroyed"):
        state.vptr


# ---- refusals: (what is called, the words of the refusal) ----
REFUSALS = {}


def refusal(name, words):
    def add(fn):
        REFUSALS[name] = (fn, words)
        return fn
    return add


def other(e):
    """an Engine of another context whose arrays decode in e's library as well (nothing of it may get that far)"""
    return Engine()


PITCH = "X and y: expected two DeviceArrays with the same row pitch"
BOTH = "X and y must both be host arrays or both be DeviceArrays"
ANOTHER = "sd_downscale: {}: `{}` belongs to another context"


def narrow(e, name, shape):
    """a resident [.., C] field of pitch 10, not the 12 of the others"""
    return e.lib.resident(e.ctx, name, shape[:-1] + (10,)).cells(0, CELLS)


def f32(e, name, shape):
    return e.wide(e.ctx, name, shape, np.float32)


# fits of a [T, C] pair
PAIR_FITS = {
    "bcsd_fit": lambda e, X, y: e.ctx.bcsd_fit(0, X, y, e.GID, G),
    "bcsd_fit_groups": lambda e, X, y: e.ctx.bcsd_fit_groups(0, X, y, e.ORDER, e.OFFSETS),
    "bcsd_fit_predict": lambda e, X, y: e.ctx.bcsd_fit_predict(0, X, y, e.GID, G, e.dXP2, e.GIDQ),
    "qm_fit": lambda e, X, y: e.ctx.qm_fit(X, y),
    "zscore_fit": lambda e, X, y: e.ctx.zscore_fit(X, y, 3, e.DAY, e.YEAR, 5),
    "arrm_fit": lambda e, X, y: e.ctx.arrm_fit(X, y, 2),
}
# fits of X [T, F, C] with y [T, C]
TRAIN_FITS = {
    "analog_fit": lambda e, X, y: e.ctx.analog_fit(X, y),
    "analog_fit_predict": lambda e, X, y: e.ctx.analog_fit_predict(X, y, e.dXQ3 if hasattr(X, "vptr") else e.XQ3, K, 3),
    "linreg_fit": lambda e, X, y: e.ctx.linreg_fit(X, y),
    "grouped_fit": lambda e, X, y: e.ctx.grouped_fit(X, y, e.KEY, 4, 1),
}
# predictions: family of the state, the query's name, result's name, call(e, state, Xq, out)
PREDICTS = {
    "bcsd_predict": ("bcsd", "XP2", "OUT2", lambda e, s, X, out: e.ctx.bcsd_predict(s, X, e.GIDQ, out=out)),
    "bcsd_predict_trend": ("bcsd", "XP2", "OUT2", lambda e, s, X, out: e.ctx.bcsd_predict_trend(s, X, e.GIDQ, e.GIDT, 2, out=out)),
    "qm_cunnane": ("qm", "XP2", "OUT2", lambda e, s, X, out: e.ctx.qm_cunnane(s, 0, X, out=out)),
    "qm_predict": ("qm", "XP2", "OUT2", lambda e, s, X, out: e.ctx.qm_predict(s, 0, X, out=out)),
    "analog_predict": ("analog", "XQ3", "OUT3", lambda e, s, X, out: e.ctx.analog_predict(s, X, K, 3, out=out)),
    "analogreg_predict": ("analog", "XQ3", "OUT3", lambda e, s, X, out: e.ctx.analogreg_predict(s, X, K, out=out)),
    "linreg_predict": ("linreg", "XQ3", "OUT3", lambda e, s, X, out: e.ctx.linreg_predict(s, X, out=out)),
    "zscore_predict": ("zscore", "XP2", "OUT2", lambda e, s, X, out: e.ctx.zscore_predict(s, X, out=out)),
    "grouped_predict": ("grouped", "XQ3", "OUT2", lambda e, s, X, out: e.ctx.grouped_predict(s, X, e.KEYQ, out=out)),
    "arrm_predict": ("arrm", "XP2", "OUT2", lambda e, s, X, out: e.ctx.arrm_predict(s, X, out=out)),
}
ROWS = dict(XP2="T", XQ3="Tq")
SIZES = dict(XP2=f"{CELLS}", XQ3=f"{F}, {CELLS}")
QUERY_NAME = dict(bcsd_predict="X", bcsd_predict_trend="X", qm_cunnane="X", qm_predict="X", zscore_predict="Xp", arrm_predict="Xq")

for name, call in PAIR_FITS.items():
    REFUSALS[f"{name}-rule_dtype-X"] = (lambda e, call=call: call(e, f32(e, "X32", (T, CELLS)), e.dY2), r"X: expected a float64 \[.*\] field, got shape \(24, 8\) of float32")
    REFUSALS[f"{name}-rule_dtype-y"] = (lambda e, call=call: call(e, e.dX2, f32(e, "y32", (T, CELLS))), r"y: expected a float64 \[.*\] field, got shape \(24, 8\) of float32")
    REFUSALS[f"{name}-rule_residency-pitch"] = (lambda e, call=call: call(e, narrow(e, "Xn", (T, CELLS)), e.dY2), PITCH)
    REFUSALS[f"{name}-rule_residency-context"] = (lambda e, call=call: call(e, other(e).dX2, e.dY2), ANOTHER.format("sd_" + name, "X"))
    REFUSALS[f"{name}-y_rows"] = (lambda e, call=call: call(e, e.X2, np.zeros((T - 1, CELLS))),
                                  r"X: expected a \[23, 8\] field" if name.startswith("bcsd") else r"y: expected a \[24, 8\] field")
for name in ("bcsd_fit", "qm_fit"):
    REFUSALS[f"{name}-mixed-resident_X"] = (lambda e, call=PAIR_FITS[name]: call(e, e.dX2, e.Y2), BOTH)
    REFUSALS[f"{name}-mixed-resident_y"] = (lambda e, call=PAIR_FITS[name]: call(e, e.X2, e.dY2), BOTH)
REFUSALS["bcsd_fit_groups-rule_residency-mixed-resident_X"] = (lambda e: PAIR_FITS["bcsd_fit_groups"](e, e.dX2, e.Y2), BOTH)
REFUSALS["bcsd_fit_groups-rule_residency-mixed-resident_y"] = (lambda e: PAIR_FITS["bcsd_fit_groups"](e, e.X2, e.dY2), BOTH)
for name in ("zscore_fit", "arrm_fit", "grouped_fit"):
    call = PAIR_FITS.get(name) or TRAIN_FITS[name]
    X = "X3" if name == "grouped_fit" else "X2"
    REFUSALS[f"{name}-mixed-resident_X"] = (lambda e, call=call, X=X: call(e, e.a("res", X), e.Y2), PITCH)
for form, X, y in (("host", "X2", "Y2"), ("resident_X", "dX2", "Y2"), ("resident_y", "X2", "dY2")):
    REFUSALS[f"bcsd_fit_predict-rule_residency-{form}"] = (lambda e, X=X, y=y: PAIR_FITS["bcsd_fit_predict"](e, getattr(e, X), getattr(e, y)),
                                                           "bcsd_fit_predict takes resident fields")
for name, call in TRAIN_FITS.items():
    REFUSALS[f"{name}-rule_dtype-X"] = (lambda e, call=call: call(e, f32(e, "X32", (T, F, CELLS)), e.dY2),
                                        r"X: expected a float64 \[T, F, C\] field, got .* of float32")
    REFUSALS[f"{name}-rule_residency-pitch"] = (lambda e, call=call: call(e, narrow(e, "Xn", (T, F, CELLS)), e.dY2), PITCH)
    REFUSALS[f"{name}-rule_residency-context"] = (lambda e, call=call: call(e, other(e).dX3, e.dY2), ANOTHER.format("sd_" + name, "X"))
    words = dict(grouped_fit=r"y: expected a \[24, 8\] field", analog_fit_predict=r"expected X \[T, F, C\] and y \[T, C\], got")
    REFUSALS[f"{name}-y_rows"] = (lambda e, call=call: call(e, e.X3, np.zeros((T - 1, CELLS))),
                                  words.get(name, r"expected X \[T, F, C\] and y \[T, C\] of the same kind, got \(24, 2, 8\) and \(23, 8\)"))
for name in ("analog_fit", "linreg_fit"):
    REFUSALS[f"{name}-mixed-resident_X"] = (lambda e, call=TRAIN_FITS[name]: call(e, e.dX3, e.Y2),
                                            r"expected X \[T, F, C\] and y \[T, C\] of the same kind, got \(24, 2, 8\) and \(24, 8\)")
REFUSALS["analog_fit_predict-mixed-resident_X"] = (lambda e: e.ctx.analog_fit_predict(e.dX3, e.Y2, e.XQ3, K, 3),
                                                   "X, y and Xq must all be numpy arrays or all DeviceArrays")
REFUSALS["analog_fit_predict-rule_residency-mixed-resident_Xq"] = (lambda e: e.ctx.analog_fit_predict(e.X3, e.Y2, e.dXQ3, K, 3),
                                                    "X, y and Xq must all be numpy arrays or all DeviceArrays")
REFUSALS["analog_fit_predict-Xq"] = (lambda e: e.ctx.analog_fit_predict(e.X3, e.Y2, np.zeros((TQ, F + 1, CELLS)), K, 3),
                                     r"Xq: expected a \[Tq, 2, 8\] field, got shape \(6, 3, 8\)")
REFUSALS["analog_fit_predict-k"] = (lambda e: e.ctx.analog_fit_predict(e.X3, e.Y2, e.XQ3, T + 1, 3), "k=25: expected 1 <= k <= 24")
REFUSALS["grouped_fit-X_rank"] = (lambda e: e.ctx.grouped_fit(e.X2, e.Y2, e.KEY, 4, 1), r"X: expected a \[T, F, C\] field, got shape \(24, 8\)")
REFUSALS["grouped_fit-key"] = (lambda e: e.ctx.grouped_fit(e.X3, e.Y2, e.KEYQ, 4, 1), "key: expected 24 entries")
REFUSALS["zscore_fit-day_idx"] = (lambda e: e.ctx.zscore_fit(e.X2, e.Y2, 3, e.KEYQ, e.YEAR, 5), "day_idx and year: expected 24 entries")
REFUSALS["bcsd_fit-group_ids"] = (lambda e: e.ctx.bcsd_fit(0, e.X2, e.Y2, e.GID, 3), r"group_id: group ids must lie in \[0, 3\)")
REFUSALS["bcsd_fit-group_id_count"] = (lambda e: e.ctx.bcsd_fit(0, e.X2, e.Y2, e.GIDQ, G), "group_id: expected 24 group ids")
REFUSALS["bcsd_fit_groups-offsets"] = (lambda e: e.ctx.bcsd_fit_groups(0, e.X2, e.Y2, e.ORDER, [0, 30]), "group offsets must start at 0")
REFUSALS["bcsd_fit_groups-order"] = (lambda e: e.ctx.bcsd_fit_groups(0, e.X2, e.Y2, e.ORDER + 1, e.OFFSETS), r"group order entries must lie in \[0, 24\)")

for name, (family, q, o, call) in PREDICTS.items():
    qname = QUERY_NAME.get(name, "Xq")
    who = "sd_" + name
    wrong = HOST_SHAPES[q][:-1] + (CELLS + 1,)
    REFUSALS[f"{name}-query_shape"] = (lambda e, call=call, family=family, wrong=wrong: call(e, e.fitted(family), np.zeros(wrong), None),
                                       rf"{qname}: expected a \[{ROWS[q]}, {SIZES[q]}\] field, got shape")
    REFUSALS[f"{name}-rule_dtype"] = (lambda e, call=call, family=family, q=q: call(e, e.fitted(family), f32(e, "q32", HOST_SHAPES[q]), None),
                                      rf"{qname}: expected a float64 \[{ROWS[q]}, {SIZES[q]}\] field, got .* of float32")
    REFUSALS[f"{name}-rule_residency-array_context"] = (lambda e, call=call, family=family, q=q: call(e, e.fitted(family), other(e).a("res", q), None),
                                                        ANOTHER.format(who, qname))
    REFUSALS[f"{name}-rule_residency-state_context"] = (lambda e, call=call, family=family, q=q: call(e, other(e).fitted(family), e.a("res", q), None),
                                                        ANOTHER.format(who, "state"))
    REFUSALS[f"{name}-rule_residency-out_context"] = (lambda e, call=call, family=family, q=q, o=o: call(e, e.fitted(family), e.a("res", q), other(e).a("res", o)),
                                                      ANOTHER.format(who, "out"))
    shape = HOST_SHAPES[o]
    res_words = rf"out: expected a float64 DeviceArray of shape \({', '.join(map(str, shape))}\)"
    host_words = rf"out: expected a C-contiguous float64 array of shape \({', '.join(map(str, shape))}\)"
    bad_res = dict(type=lambda e: np.zeros(shape), dtype=lambda e: f32(e, "o32", shape), shape=lambda e: e.wide(e.ctx, "os", (TQ + 1,) + shape[1:]),
                   pitch=lambda e: DeviceView(e, shape))
    bad_host = dict(type=lambda e: e.a("res", o), dtype=lambda e: np.zeros(shape, dtype=np.float32), shape=lambda e: np.zeros((1, 1)),
                    pitch=lambda e: np.zeros(shape[:-1] + (LD,))[..., :CELLS])
    for what in bad_res:
        REFUSALS[f"{name}-rule_out-resident-{what}"] = (lambda e, call=call, family=family, q=q, bad=bad_res[what]: call(e, e.fitted(family), e.a("res", q), bad(e)),
                                                        res_words)
        REFUSALS[f"{name}-rule_out-host-{what}"] = (lambda e, call=call, family=family, q=q, bad=bad_host[what]: call(e, e.fitted(family), e.a("host", q), bad(e)),
                                                    host_words)


def DeviceView(e, shape):
    """a resident result whose pitch (7) is below its cells: rows that overlap"""
    from skdownscale_amd.engine import DeviceArray

    return DeviceArray(e.ctx, shape, dptr=e.lib.resident(e.ctx, "op", shape).ptr, owner=False, ld=CELLS - 1)


for what, bad, words in (("type", lambda e: np.zeros((TQ, CELLS)), "out: expected a float64 DeviceArray"),
                         ("dtype", lambda e: f32(e, "o32", (TQ, CELLS)), "out: expected a float64 DeviceArray"),
                         ("shape", lambda e: e.wide(e.ctx, "os", (TQ + 1, CELLS)), "out: expected a float64 DeviceArray"),
                         ("pitch", lambda e: DeviceView(e, (TQ, CELLS)), "out: expected a float64 DeviceArray"),
                         ("context", lambda e: other(e).dOUT2, ANOTHER.format("sd_bcsd_fit_predict", "out"))):
    REFUSALS[f"bcsd_fit_predict-rule_out-{what}"] = (lambda e, bad=bad: e.ctx.bcsd_fit_predict(0, e.dX2, e.dY2, e.GID, G, e.dXP2, e.GIDQ, out=bad(e)), words)
for what, bad, words in (("resident-type", lambda e: np.zeros((TQ, 3, CELLS)), "out: expected a float64 DeviceArray"),
                         ("resident-pitch", lambda e: DeviceView(e, (TQ, 3, CELLS)), "out: expected a float64 DeviceArray"),
                         ("resident-context", lambda e: other(e).dOUT3, ANOTHER.format("sd_analog_fit_predict", "out"))):
    REFUSALS[f"analog_fit_predict-rule_out-{what}"] = (lambda e, bad=bad: e.ctx.analog_fit_predict(e.dX3, e.dY2, e.dXQ3, K, 3, out=bad(e)), words)
REFUSALS["analog_fit_predict-host_out"] = (lambda e: e.ctx.analog_fit_predict(e.X3, e.Y2, e.XQ3, K, 3, out=np.zeros((1, 1))),
                                           r"out: expected a C-contiguous float64 array of shape \(6, 3, 8\)")
REFUSALS["bcsd_predict-out_dtype"] = (lambda e: e.ctx.bcsd_predict(e.fitted("bcsd"), e.XP2, e.GIDQ, out_dtype=np.int32), "out_dtype must be float64 or float32")
REFUSALS["bcsd_predict-out_dtype_with_out"] = (lambda e: e.ctx.bcsd_predict(e.fitted("bcsd"), e.XP2, e.GIDQ, out=e.OUT2, out_dtype=np.float32),
                                               "does not combine with a float64 `out` buffer")
REFUSALS["bcsd_predict-group_ids"] = (lambda e: e.ctx.bcsd_predict(e.fitted("bcsd"), e.XP2, e.GIDQ + G), r"group ids must lie in \[0, 12\)")
REFUSALS["bcsd_predict_trend-trend_ids"] = (lambda e: e.ctx.bcsd_predict_trend(e.fitted("bcsd"), e.XP2, e.GIDQ, e.GIDT, 1),
                                            r"trend_group_id: group ids must lie in \[0, 1\)")
REFUSALS["bcsd_import-new_order-trend_shape"] = (lambda e: e.ctx.bcsd_import(dict(exported(e, "bcsd", info=dict(kind=0, G=G, T=T, C=CELLS, return_anoms=True, detrend=True),
                                                                                 group_offsets=np.arange(G + 1)), y_trend=np.zeros((CELLS, G)))),
                                       "y_trend: expected shape")
for name in ("qm_cunnane", "qm_predict"):
    REFUSALS[f"{name}-extrapolate"] = (lambda e, name=name: getattr(e.ctx, name)(e.fitted("qm"), 0, e.XP2, "sideways"), "unknown value for extrapolate: sideways")
for k in (0, T + 1):
    REFUSALS[f"analog_predict-k{k}"] = (lambda e, k=k: e.ctx.analog_predict(e.fitted("analog"), e.XQ3, k, 3), rf"k={k}: expected 1 <= k <= 24")
REFUSALS["analog_predict-sample_inds_shape"] = (lambda e: e.ctx.analog_predict(e.fitted("analog"), e.XQ3, K, 1, sample_inds=np.zeros((3, 2), np.int32)),
                                                r"sample_inds: expected shape \(6, 8\)")
REFUSALS["analog_predict-sample_inds_range"] = (lambda e: e.ctx.analog_predict(e.fitted("analog"), e.XQ3, K, 1, sample_inds=e.SAMP + K),
                                                r"sample_inds must lie in \[0, 3\)")
REFUSALS["analog_predict-rule_residency-resident_sample_inds_host_Xq"] = (
    lambda e: e.ctx.analog_predict(e.fitted("analog"), e.XQ3, K, 1, sample_inds=e.dSAMP), "Xq and sample_inds must both be host arrays or both be DeviceArrays")
REFUSALS["analog_predict-rule_residency-sample_inds_context"] = (
    lambda e: e.ctx.analog_predict(e.fitted("analog"), e.dXQ3, K, 1, sample_inds=other(e).dSAMP), ANOTHER.format("sd_analog_predict", "sample_inds"))
REFUSALS["analog_predict-rule_dtype-sample_inds"] = (
    lambda e: e.ctx.analog_predict(e.fitted("analog"), e.dXQ3, K, 1, sample_inds=e.lib.resident(e.ctx, "s64", (TQ, CELLS), np.int64)),
    "sample_inds: expected a contiguous int32 DeviceArray")
REFUSALS["analog_predict-rule_out-neighbors_pitch"] = (lambda e: e.ctx.analog_predict(e.fitted("analog"), e.dXQ3, K, 3, want_neighbors=True, out=e.dOUT3),
                                                       "the neighbour fields share the pitch of `out`")
REFUSALS["zscore_predict-new_order-stats_pitch"] = (lambda e: e.ctx.zscore_predict(e.fitted("zscore"), e.dXP2, out=e.dOUT2, with_stats=True),
                                          "the stats fields share the pitch of `out`")
REFUSALS["grouped_predict-key"] = (lambda e: e.ctx.grouped_predict(e.fitted("grouped"), e.XQ3, e.KEY), "key: expected 6 entries")
REFUSALS["zscore_import-planes"] = (lambda e: e.ctx.zscore_import(dict(exported(e, "zscore", window_width=3), shift=np.zeros((4, CELLS)))),
                                    "the six planes must share one")
REFUSALS["grouped_import-shapes"] = (lambda e: e.ctx.grouped_import(exported(e, "grouped", window=1, fitted=np.ones(3, dtype=np.int32))),
                                     "grouped_import: expected coef")
REFUSALS["arrm_import-shapes"] = (lambda e: e.ctx.arrm_import(exported(e, "arrm", T=T, break_index=np.zeros((3, CELLS), dtype=np.int32))),
                                  "arrm_import: expected breaks")
REFUSALS["regrid_create-method"] = (lambda e: e.ctx.regrid_create(np.arange(3.0), np.arange(4.0), np.arange(5.0), np.arange(6.0), "cubic"), "regrid method 'cubic'")
REFUSALS["remap_create-bounds"] = (lambda e: e.ctx.remap_create(np.arange(4.0), np.arange(1.0), np.arange(3.0), np.arange(3.0)), "src_xb: expected the n \\+ 1 bounds")


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    call, words = REFUSALS[name]
    e = Engine()
    with pytest.raises((ValueError, NotImplementedError), match=words):
        call(e)
    assert e.reached() == []


# ---- the ``out`` rule: a valid host ``out`` is what the library writes and what the caller gets back ----
@pytest.mark.parametrize("name", sorted(PREDICTS))
def test_host_out_rule_out(name):
    family, q, o, call = PREDICTS[name]
    e = Engine()
    got = call(e, e.fitted(family), e.a("host", q), e.a("host", o))
    assert got[0] is e.a("host", o)
    assert (o, 0) in e.lib.log[-1][1]


def test_host_out_rule_out_analog_fit_predict():
    e = Engine()
    assert e.ctx.analog_fit_predict(e.X3, e.Y2, e.XQ3, K, 3, out=e.OUT3)[0] is e.OUT3
    assert ("OUT3", 0) in e.lib.log[-1][1]


@pytest.mark.parametrize("name", sorted(PREDICTS))
def test_resident_out_view_is_kept(name):
    family, q, o, call = PREDICTS[name]
    e = Engine()
    got = call(e, e.fitted(family), e.a("res", q), e.a("res", o))
    args = e.lib.log[-1][1]
    assert got[0] is e.a("res", o) and args[args.index(("d" + o, C0)) + 1] == LD
