"""What the fitted states of BCSD, the analogs, the regressor families and of quantile mapping promise their callers, whichever file
implements them (csrc/sd_bcsd.hip, sd_analog.hip, sd_linreg.hip, sd_zscore.hip, sd_grouped.hip, sd_arrm.hip, sd_qm.hip): per-cell
status out of fit, export and predict with masked before non-finite, NaN on the flagged cells (a cell that only the predict input
flags: see Family.pred_nan), the host-buffer and the resident form of every entry point bit-identical, export -> import -> predict
bit-identical to the fitted state, a second export equal to the first, close() twice harmless.  The analog state has no export,
no import and no status of its own: its fit status shows in the predict status only.

Through skdownscale_amd.engine.Context only.  C = 67 cells: one full 64-cell tile and a ragged one of three; the resident form
runs on DeviceArray.cells() views of [.., 80] parents, so the row pitch differs from C on the way in and on the way out.  Four
planted cells: MASKED (NaN as the first sample of X), MID (a NaN in the middle of the fit series), PRED (a NaN in the predict input
only) in the full tile, BOTH (masked and a NaN in the predict input) in the ragged one.  BcsdPrecipitation plants a fifth, CLIMO: one
group of its observations all dry, which fit reports as a bad climatology, and a NaN in its predict input."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

C, PITCH, C0 = 67, 80, 4
MASKED, MID, PRED, BOTH, CLIMO = 5, 17, 40, 65, 29
OK_, MASK_, NONF_, CLIMO_ = 0, 1, 2, 3  # SD_CELL_OK, SD_CELL_MASKED, SD_CELL_NONFINITE, SD_CELL_BAD_CLIMO


def expected_status(**cells):
    s = np.zeros(C, dtype=np.int32)
    for name, code in cells.items():
        s[globals()[name]] = code
    return s


FIT_STATUS = expected_status(MASKED=MASK_, MID=NONF_, BOTH=MASK_)
PREDICT_STATUS = expected_status(MASKED=MASK_, MID=NONF_, PRED=NONF_, BOTH=MASK_)


def fields(seed, T, Tq, F=None):
    """seeded Gaussian X, y of a fit and Xq of a predict call ([T, C], or [T, F, C] with F), the four cells planted"""
    rng = np.random.default_rng(seed)
    shape = (C,) if F is None else (F, C)
    X = rng.normal(0.0, 1.0, (T,) + shape)
    y = 0.8 * (X if F is None else X.sum(axis=1)) + rng.normal(0.0, 0.5, (T, C))
    Xq = rng.normal(0.0, 1.0, (Tq,) + shape)
    first = (0,) if F is None else (0, 0)
    X[first + (MASKED,)] = np.nan
    X[first + (BOTH,)] = np.nan
    X[(T // 2,) + first[1:] + (MID,)] = np.nan
    Xq[(Tq // 2,) + first[1:] + (PRED,)] = np.nan
    Xq[(Tq // 2,) + first[1:] + (BOTH,)] = np.nan
    return X, y, Xq


def resident(ctx, a):
    """a [.., C] on the device as the cells [C0, C0 + C) of a [.., PITCH] parent"""
    parent = np.full(a.shape[:-1] + (PITCH,), 7.0)
    parent[..., C0:C0 + C] = a
    return ctx.to_device(parent).cells(C0, C0 + C)


def resident_out(ctx, shape):
    return ctx.empty(shape[:-1] + (PITCH,)).cells(C0, C0 + C)


def host(a):
    return a if isinstance(a, np.ndarray) else a.to_host()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


class Family:
    """fit(ctx, X, y) -> (state, extras); predict(ctx, state, Xq, out) -> (out, status, extras); status(state); export(state);
    importer: the Context method that takes an export back"""
    importer = None
    out_shape = staticmethod(lambda Tq: (Tq, C))
    finite_everywhere = True
    fit_status, predict_status = FIT_STATUS, PREDICT_STATUS
    # What a cell whose only fault is a NaN in the predict input gets (the cells that fit flagged are NaN throughout, everywhere):
    # "sample": NaN at the non-finite sample, a prediction at every other one (the streaming predict kernels decide per sample);
    # "cell": NaN throughout.  Either way the cell is reported as non-finite.
    pred_nan = "sample"

    def status(self, state):
        return state.status()

    def export(self, state):
        return state.export()

    def more(self, ctx, st_h, st_d, out_h, status_h):
        """what a family promises beyond the common contract"""


class Bcsd(Family):
    """T = 96 in four groups of 24, Tp = 40 in groups of 10 (a detrended group needs four samples)"""
    importer = "bcsd_import"
    pred_nan = "cell"  # (nan_fill_kernel writes whole columns)
    G = 4

    def __init__(self, kind, detrend=False):
        self.kind, self.detrend = kind, detrend
        X, y, Xq = fields(16, 96, 40)
        self.gid, self.gid_q = np.repeat(np.arange(self.G), 24), np.repeat(np.arange(self.G), 10)
        if kind == 1:  # BcsdPrecipitation: zero-inflated observations, continuous wet values
            rng = np.random.default_rng(17)
            X, Xq = np.exp(X), np.exp(Xq)
            y = np.where(rng.random(y.shape) < 0.4, 0.0, np.exp(y))
            # the cell of tests/golden/make_golden.py that raises 'Invalid value in target climatology': one group all dry.  The
            # reference raises in fit first, so the NaN in its predict input does not change what the cell reports.
            y[self.gid == 2, CLIMO] = 0.0
            Xq[Xq.shape[0] // 2, CLIMO] = np.nan
            self.fit_status = expected_status(MASKED=MASK_, MID=NONF_, BOTH=MASK_, CLIMO=CLIMO_)
            self.predict_status = expected_status(MASKED=MASK_, MID=NONF_, PRED=NONF_, BOTH=MASK_, CLIMO=CLIMO_)
        self.data = X, y, Xq

    def fit(self, ctx, X, y):
        return ctx.bcsd_fit(self.kind, X, y, self.gid, self.G, True, detrend=self.detrend), {}

    def predict(self, ctx, state, Xq, out):
        o, s = ctx.bcsd_predict(state, Xq, self.gid_q, out=out)
        return o, s, {}

    def more(self, ctx, st_h, st_d, out_h, status_h):
        """fit + predict in one call on resident fields is fit followed by predict: the same status and NaN cells; bit for bit where
        the call goes through a transient state (detrend), and up to the rounding of the climatologies where the fused kernels run.
        Those sum the n = 24 samples of a group in another order than the fit kernels, and two float64 sums of n terms differ by at
        most (n - 1) eps mean|x|.  BcsdTemperature returns (rolling mean - x_climo) + q - y_climo: both climatologies differ by that,
        the three operations round by eps / 2 of an intermediate each, and every term is below max|X| + max|Xq| + max|y|, hence
        (n + 3) eps of that sum.  BcsdPrecipitation returns q / y_climo with y >= 0: (n - 1) eps relative from the sum, eps from the
        division.  (Measured on these inputs: 2 eps absolute of 2.8, and 2 eps relative.)"""
        X, y, Xq = self.data
        o, s = ctx.bcsd_fit_predict(self.kind, resident(ctx, X), resident(ctx, y), self.gid, self.G, resident(ctx, Xq), self.gid_q, True,
                                    out=resident_out(ctx, out_h.shape), detrend=self.detrend)
        assert o.ld == PITCH and np.array_equal(s, status_h)
        o = o.to_host()
        n, eps, ok = 24, np.finfo(np.float64).eps, ~np.isnan(out_h)
        if self.detrend:
            bound = np.zeros_like(out_h)
        elif self.kind == 0:
            bound = np.full_like(out_h, (n + 3) * eps * sum(np.nanmax(np.abs(a)) for a in (X, Xq, y)))
        else:
            bound = n * eps * np.abs(out_h)
        print("fit_predict against fit -> predict: largest difference %.3g, its bound %.3g" % (np.abs(o - out_h)[ok].max(), bound[ok].max()))
        assert np.array_equal(np.isnan(o), ~ok) and (np.abs(o - out_h)[ok] <= bound[ok]).all()


class Analog(Family):
    """T = 60, Tq = 9, k = 3, mean_analogs"""
    out_shape = staticmethod(lambda Tq: (Tq, 3, C))
    K, KIND = 3, 3  # SD_ANALOG_MEAN

    def __init__(self, F):
        self.data = fields(18, 60, 9, F=F)

    def fit(self, ctx, X, y):
        return ctx.analog_fit(X, y), {}

    def predict(self, ctx, state, Xq, out):
        o, s = ctx.analog_predict(state, Xq, self.K, self.KIND, out=out)
        return o, s, {}

    status = export = None

    def more(self, ctx, st_h, st_d, out_h, status_h):
        X, y, Xq = self.data
        # AnalogRegression, and fit + predict in one call: host-buffer and resident form bit-identical
        r_h, rs_h = ctx.analogreg_predict(st_h, Xq, self.K)
        r_d, rs_d = ctx.analogreg_predict(st_d, resident(ctx, Xq), self.K, out=resident_out(ctx, out_h.shape))
        assert np.array_equal(rs_h, status_h) and np.array_equal(rs_d, rs_h) and same(r_d.to_host(), r_h)
        f_h, fs_h = ctx.analog_fit_predict(X, y, Xq, self.K, self.KIND)
        f_d, fs_d = ctx.analog_fit_predict(resident(ctx, X), resident(ctx, y), resident(ctx, Xq), self.K, self.KIND,
                                           out=resident_out(ctx, out_h.shape))
        assert np.array_equal(fs_h, status_h) and np.array_equal(fs_d, fs_h) and same(f_h, out_h) and same(f_d.to_host(), f_h)
        # the neighbours (optional outputs of the host-buffer form) equal the resident form's, on the cells the call reports as OK.
        # The kernels write inds / dist of an active cell only (sd_analog_epilogue.h: `if (cell_active && pa.inds)`), so for a
        # flagged cell either form hands back what its buffer held before the call; those cells are printed, not compared.
        o_h, s_h, inds_h, dist_h = ctx.analog_predict(st_h, Xq, self.K, self.KIND, want_neighbors=True)
        o_d, s_d, inds_d, dist_d = ctx.analog_predict(st_d, resident(ctx, Xq), self.K, self.KIND, want_neighbors=True)
        assert np.array_equal(s_h, status_h) and np.array_equal(s_d, s_h) and same(o_d.to_host(), o_h)
        ok, inds_d, dist_d = status_h == 0, inds_d.to_host(), dist_d.to_host()
        print("cells whose neighbours differ between the two forms:", np.flatnonzero((inds_d != inds_h).any(axis=(0, 1))),
              np.flatnonzero(~((dist_d == dist_h) | (np.isnan(dist_d) & np.isnan(dist_h))).all(axis=(0, 1))))
        assert same(inds_d[..., ok], inds_h[..., ok]) and same(dist_d[..., ok], dist_h[..., ok])
        assert (inds_h[..., ok] >= 0).all() and (inds_h[..., ok] < X.shape[0]).all() and np.isfinite(dist_h[..., ok]).all()


class Linreg(Family):
    importer = "linreg_import"
    out_shape = staticmethod(lambda Tq: (Tq, 3, C))

    def __init__(self, thresh):
        self.thresh = thresh
        self.data = fields(11, 60, 9, F=2)

    def fit(self, ctx, X, y):
        return ctx.linreg_fit(X, y, thresh=self.thresh), {}

    def predict(self, ctx, state, Xq, out):
        o, s = ctx.linreg_predict(state, Xq, out=out)
        return o, s, {}

    def status(self, state):
        return state.export()["status"]


class Zscore(Family):
    importer = "zscore_import"
    finite_everywhere = False  # (the centred rolling window leaves the ends of the series NaN)
    pred_nan = "window"  # NaN wherever the rolling window holds the sample, and as far as the sliding sums carry it

    def __init__(self):
        from skdownscale_amd.zscore import day_grid
        from test_gpu_zscore import CALENDARS

        index = CALENDARS["days_100"]  # the shortest calendar of test_gpu_zscore.py, with its narrowest window that has a spread
        self.w = 2
        self.labels, self.day_idx, self.year = day_grid(index)
        self.data = fields(12, len(index), len(self.labels) - 2)  # one period of the kept windows

    def fit(self, ctx, X, y):
        return ctx.zscore_fit(X, y, self.w, self.day_idx, self.year, len(self.labels)), {}

    def predict(self, ctx, state, Xq, out):
        o, s, _ = ctx.zscore_predict(state, Xq, out=out)
        _, s2, stats = ctx.zscore_predict(state, Xq, with_stats=True)  # (resident: the stats share the pitch of a contiguous out)
        assert np.array_equal(s, s2)
        return o, s, {k: host(v) for k, v in stats.items()}


class Grouped(Family):
    importer = "grouped_import"

    def __init__(self):
        self.data = fields(13, 120, 24, F=2)

    def fit(self, ctx, X, y):
        return ctx.grouped_fit(X, y, np.arange(120) % 12, 12, 1), {}

    def predict(self, ctx, state, Xq, out):
        o, s = ctx.grouped_predict(state, Xq, np.arange(24) % 12, out=out)
        return o, s, {}


class Arrm(Family):
    importer = "arrm_import"

    def __init__(self):
        self.data = fields(14, 200, 9)

    def fit(self, ctx, X, y):
        state, r2 = ctx.arrm_fit(X, y, 4, with_r2=True)
        return state, {"r2": host(r2)}

    def predict(self, ctx, state, Xq, out):
        o, s = ctx.arrm_predict(state, Xq, out=out)
        return o, s, {}


class Qm(Family):
    pred_nan = "cell"  # (the result leaves the cell-major staging through the status of the call)

    def __init__(self, cunnane):
        self.cunnane = cunnane
        self.data = fields(15, 60, 9)

    def fit(self, ctx, X, y):
        return ctx.qm_fit(X, None if self.cunnane else y), {}  # (CunnaneTransformer: the optional input is absent)

    def predict(self, ctx, state, Xq, out):
        if self.cunnane:
            o, s = ctx.qm_cunnane(state, 0, Xq, extrapolate=None, out=out)
        else:
            o, s = ctx.qm_predict(state, 0, Xq, out=out)
        return o, s, {}

    def status(self, state):
        return self.export(state)["status"]

    def export(self, state):
        return state.export(with_y=not self.cunnane)


CASES = {
    "bcsd_tas": lambda: Bcsd(0),
    "bcsd_pr": lambda: Bcsd(1),
    "bcsd_tas_detrend": lambda: Bcsd(0, detrend=True),
    "analog_f1": lambda: Analog(1),
    "analog_f2": lambda: Analog(2),
    "linreg": lambda: Linreg(None),
    "linreg_thresh": lambda: Linreg(0.0),
    "zscore": Zscore,
    "grouped": Grouped,
    "arrm": Arrm,
    "qm_predict": lambda: Qm(False),
    "qm_cunnane": lambda: Qm(True),
}


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_state_contract(ctx, case):
    fam = CASES[case]()
    X, y, Xq = fam.data
    Tq = Xq.shape[0]
    flagged, fit_flagged = fam.predict_status != 0, fam.fit_status != 0
    ok_rows = np.arange(Tq) != Tq // 2  # (the planted sample of the predict input sits in row Tq // 2)

    # the host-buffer form
    st_h, fit_h = fam.fit(ctx, X, y)
    if fam.status:
        print(case, "fit status", fam.status(st_h)[[MASKED, MID, PRED, BOTH, CLIMO]], "others", np.flatnonzero(fam.status(st_h) * (fam.fit_status == 0)))
        assert np.array_equal(fam.status(st_h), fam.fit_status)
    out_h, status_h, pred_h = fam.predict(ctx, st_h, Xq, None)
    print(case, "predict status", status_h[[MASKED, MID, PRED, BOTH, CLIMO]], "others", np.flatnonzero(status_h * (fam.predict_status == 0)))
    assert np.array_equal(status_h, fam.predict_status)
    print(case, "NaN rows of the PRED cell", np.flatnonzero(np.isnan(out_h[..., PRED]).reshape(Tq, -1).any(axis=1)))
    assert out_h.shape == fam.out_shape(Tq) and np.isnan(out_h[..., fit_flagged]).all() and np.isnan(out_h[Tq // 2, ..., PRED]).all()
    if fam.pred_nan == "sample":
        assert np.isfinite(out_h[ok_rows][..., PRED]).all()
    elif fam.pred_nan == "window":
        assert np.isnan(out_h[Tq // 2 - (fam.w - 1) // 2:Tq // 2 + fam.w // 2 + 1, PRED]).all()
    else:
        assert np.isnan(out_h[..., PRED]).all()
    if fam.finite_everywhere:
        assert np.isfinite(out_h[..., ~flagged]).all()
    else:
        assert np.isfinite(out_h[..., ~flagged]).any(axis=0).all()

    # the resident form, on views whose pitch is not C
    st_d, fit_d = fam.fit(ctx, resident(ctx, X), resident(ctx, y))
    assert not fam.status or np.array_equal(fam.status(st_d), fam.fit_status)
    out_d, status_d, pred_d = fam.predict(ctx, st_d, resident(ctx, Xq), resident_out(ctx, fam.out_shape(Tq)))
    assert out_d.ld == PITCH
    assert np.array_equal(status_d, status_h) and same(host(out_d), out_h)
    for extras_h, extras_d in ((fit_h, fit_d), (pred_h, pred_d)):  # zscore: the four stats fields; arrm: r2
        assert extras_h.keys() == extras_d.keys()
        for k in extras_h:
            assert same(extras_h[k], extras_d[k]), k
    fam.more(ctx, st_h, st_d, out_h, status_h)
    e_h, e_d = (fam.export(st_h), fam.export(st_d)) if fam.export else ({}, {})
    assert e_h.keys() == e_d.keys() and all(same(np.asarray(e_h[k]), np.asarray(e_d[k])) for k in e_h if e_h[k] is not None)

    # export -> import -> predict; a second export
    if fam.importer is not None:
        st_i = getattr(ctx, fam.importer)(e_h)
        out_i, status_i, _ = fam.predict(ctx, st_i, Xq, None)
        assert np.array_equal(status_i, status_h) and same(out_i, out_h)
        again = fam.export(st_i)
        assert again.keys() == e_h.keys() and all(same(np.asarray(again[k]), np.asarray(e_h[k])) for k in e_h)
        st_i.close()
    again = fam.export(st_h) if fam.export else {}
    assert all(same(np.asarray(again[k]), np.asarray(e_h[k])) for k in e_h if e_h[k] is not None)

    for st in (st_h, st_d):
        st.close()
        st.close()
