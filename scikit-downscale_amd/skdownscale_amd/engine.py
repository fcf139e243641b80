"""Thin object layer over the C ABI: contexts, HBM-resident fields and fitted-state handles."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib
from ._lib import check, ptr


class DeviceArray:
    """A float64/int field resident in HBM (owned by the library's allocator, not torch)."""

    def __init__(self, ctx, shape, dtype=np.float64, dptr=None, owner=True, ld=None, base=None):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ld = self.shape[-1] if ld is None else int(ld)  # elements between consecutive rows (>= cells)
        self._base = base  # keeps the parent of a view alive
        self._owner = owner
        if dptr is None:
            p = C.c_void_p()
            check(ctx.lib.sd_dev_alloc(ctx.handle, self.nbytes, C.byref(p)))
            dptr = p.value
        self.ptr = dptr
        if owner:
            self._fin = weakref.finalize(self, DeviceArray._free, ctx, dptr)

    @staticmethod
    def _free(ctx, dptr):
        if ctx.handle is not None:
            ctx.lib.sd_dev_free(ctx.handle, C.c_void_p(dptr))

    def free(self):
        if self._owner and self._fin.alive:
            self._fin()

    @property
    def vptr(self):
        return C.c_void_p(self.ptr)

    @property
    def base(self):
        """the array this view was cut from (None for an array that owns its memory)"""
        return self._base

    def cells(self, c0, c1):
        """View of the cell range [c0, c1) of a [..., C] field: same rows, leading dimension of the parent
        (how a cell shard of a resident grid is handed to the engine without a copy)."""
        assert 0 <= c0 < c1 <= self.shape[-1]
        return DeviceArray(self.ctx, self.shape[:-1] + (c1 - c0,), self.dtype, dptr=self.ptr + c0 * self.dtype.itemsize,
                           owner=False, ld=self.ld, base=self)

    def rows(self, r0, r1):
        """View of the rows [r0, r1) of a [T, C] field"""
        assert len(self.shape) == 2 and 0 <= r0 < r1 <= self.shape[0]
        return DeviceArray(self.ctx, (r1 - r0, self.shape[1]), self.dtype, dptr=self.ptr + r0 * self.ld * self.dtype.itemsize, owner=False,
                           ld=self.ld, base=self)

    def to_host(self):
        if self.ld != self.shape[-1]:  # strided view: copy the parent's rows and slice on the host
            rows = int(np.prod(self.shape[:-1], dtype=np.int64))
            nbytes = ((rows - 1) * self.ld + self.shape[-1]) * self.dtype.itemsize
            flat = np.empty(nbytes // self.dtype.itemsize, dtype=self.dtype)
            check(self.ctx.lib.sd_memcpy_d2h(self.ctx.handle, ptr(flat), self.vptr, nbytes))
            full = np.zeros(rows * self.ld, dtype=self.dtype)
            full[:flat.size] = flat
            return full.reshape(rows, self.ld)[:, :self.shape[-1]].reshape(self.shape).copy()
        out = np.empty(self.shape, dtype=self.dtype)
        check(self.ctx.lib.sd_memcpy_d2h(self.ctx.handle, ptr(out), self.vptr, self.nbytes))
        return out

    def copy_from_host(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.shape == self.shape, (a.shape, self.shape)
        check(self.ctx.lib.sd_memcpy_h2d(self.ctx.handle, self.vptr, ptr(a), self.nbytes))
        return self


def vptr(a):
    """device pointer of a DeviceArray (or None)"""
    return None if a is None else a.vptr


def _f32(a):
    """the flag the ABI takes beside a float32 / float64 field: 1 for float32"""
    return int(a.dtype == np.float32)


class _State:
    """A handle of the library.  ``ABI`` is the prefix of the family's entry points (``ABI_info``, ``ABI_destroy``), ``INFO`` the
    (key, ctype) of what ``ABI_info`` gives, in the order of its arguments."""
    ABI = None
    INFO = ()

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle
        self._fin = weakref.finalize(self, _State._destroy, ctx, handle, getattr(ctx.lib, self.ABI + "_destroy"))

    @staticmethod
    def _destroy(ctx, handle, destroy):
        if ctx.handle is not None and handle:
            destroy(C.c_void_p(handle))

    def close(self):
        if self._fin.alive:
            self._fin()
        self.handle = None

    @property
    def vptr(self):
        if self.handle is None:
            raise ValueError("state has been destroyed")
        return C.c_void_p(self.handle)

    def info(self):
        v = [ctype() for _, ctype in self.INFO]
        check(getattr(self.ctx.lib, self.ABI + "_info")(self.vptr, *[C.byref(x) for x in v]))
        return {key: x.value for (key, _), x in zip(self.INFO, v)}


class _FittedState(_State):
    """A state whose ``ABI_export`` takes ``PLANES`` optional outputs (NULL: not wanted) and then the cell status [C]."""
    PLANES = 0

    def _export(self, cells, *planes):
        status = np.empty(cells, dtype=np.int32)
        check(getattr(self.ctx.lib, self.ABI + "_export")(self.vptr, *[ptr(p) for p in planes], ptr(status)))
        return status

    def status(self):
        return self._export(self.info()["C"], *[None] * self.PLANES)


class BcsdState(_State):
    ABI = "sd_bcsd_state"
    INFO = (("kind", C.c_int), ("G", C.c_int), ("T", C.c_int64), ("C", C.c_int64), ("flags", C.c_int))

    def info(self):
        i = super().info()
        flags = i.pop("flags")
        return dict(i, return_anoms=bool(flags & _lib.BCSD_RETURN_ANOMS), detrend=bool(flags & _lib.BCSD_QM_DETREND))

    def status(self):
        st = np.empty(self.info()["C"], dtype=np.int32)
        check(self.ctx.lib.sd_bcsd_state_status(self.vptr, ptr(st)))
        return st

    def set_tails(self, extrapolate="both", n_endpoints=10):
        """CunnaneTransformer(extrapolate, n_endpoints) of the fitted inverse CDFs (quantile.py:418-431, 523-545) for later
        predict calls: which tails continue along the least-squares line through the first / last ``n_endpoints`` points."""
        masks = {"both": 3, "min": _lib.QT_TAIL_LOWER, "max": _lib.QT_TAIL_UPPER, "1to1": 0, None: 0}
        if extrapolate not in masks:
            raise ValueError(f"extrapolate={extrapolate!r}: expected one of 'min', 'max', 'both', '1to1', None")
        check(self.ctx.lib.sd_bcsd_state_set_tails(self.vptr, masks[extrapolate], int(n_endpoints)))

    def export(self):
        i = self.info()
        ys = np.empty((i["C"], i["T"]))
        xc = np.empty((i["C"], i["G"]))
        yc = np.empty((i["C"], i["G"]))
        st = np.empty(i["C"], dtype=np.int32)
        off = np.empty(i["G"] + 1, dtype=np.int64)
        check(self.ctx.lib.sd_bcsd_state_export(self.vptr, ptr(ys), ptr(xc), ptr(yc), ptr(st), ptr(off)))
        e = dict(info=i, y_sorted=ys, x_climo=xc, y_climo=yc, status=st, group_offsets=off)
        if i["detrend"]:  # slope, intercept of every fitted segment's line (quantile.py:97)
            e["y_trend"] = np.empty((i["C"], i["G"], 2))
            check(self.ctx.lib.sd_bcsd_state_get_trend(self.vptr, ptr(e["y_trend"])))
        return e


class AnalogState(_State):
    ABI = "sd_analog_state"
    INFO = (("T", C.c_int64), ("F", C.c_int), ("C", C.c_int64))


class LinregState(_FittedState):
    ABI = "sd_linreg_state"
    INFO = (("T", C.c_int64), ("F", C.c_int), ("C", C.c_int64))
    PLANES = 5

    def export(self):
        """coef [F, C], intercept [C], fit_error [C], status [C]; with a threshold also logistic_coef [F, C],
        logistic_intercept [C] and thresh_dropped [C] (cells whose samples all exceed: probability 1, gard.py:426-437)"""
        i = self.info()
        coef, icpt, err = np.empty((i["F"], i["C"])), np.empty(i["C"]), np.empty(i["C"])
        logit = np.full((i["F"] + 1, i["C"]), np.nan)
        dropped = np.full(i["C"], -1, dtype=np.int32)
        status = self._export(i["C"], coef, icpt, err, logit, dropped)
        out = dict(coef=coef, intercept=icpt, fit_error=err, status=status, T=i["T"])
        if (dropped >= 0).all():  # a model with a threshold
            out.update(logistic_coef=logit[:-1], logistic_intercept=logit[-1], thresh_dropped=dropped.astype(bool))
        return out


class ZscoreState(_FittedState):
    ABI = "sd_zscore_state"
    INFO = (("K", C.c_int64), ("C", C.c_int64), ("window_width", C.c_int))
    STATS = ("x_mean", "x_std", "y_mean", "y_std", "shift", "scale")
    PLANES = len(STATS)

    def export(self):
        """x_mean, x_std, y_mean, y_std, shift, scale [K, C] (kept day windows x cells), status [C], window_width"""
        i = self.info()
        planes = {k: np.empty((i["K"], i["C"])) for k in self.STATS}
        status = self._export(i["C"], *planes.values())
        return dict(planes, status=status, window_width=i["window_width"])


class GroupedState(_FittedState):
    ABI = "sd_grouped_state"
    INFO = (("n", C.c_int), ("F", C.c_int), ("C", C.c_int64), ("window", C.c_int))
    PLANES = 3

    def fitted(self):
        fitted = np.empty(self.info()["n"], dtype=np.int32)
        check(self.ctx.lib.sd_grouped_state_export(self.vptr, None, None, ptr(fitted), None))
        return fitted.astype(bool)

    def export(self):
        """coef [n, F, C], intercept [n, C], fitted [n] (bool), status [C], window"""
        i = self.info()
        coef, icpt, fitted = np.empty((i["n"], i["F"], i["C"])), np.empty((i["n"], i["C"])), np.empty(i["n"], dtype=np.int32)
        status = self._export(i["C"], coef, icpt, fitted)
        return dict(coef=coef, intercept=icpt, fitted=fitted.astype(bool), status=status, window=i["window"])


class ArrmState(_FittedState):
    ABI = "sd_arrm_state"
    INFO = (("B", C.c_int), ("C", C.c_int64), ("T", C.c_int64))
    PLANES = 4

    def export(self):
        """breaks [B, C], break_index [B, C] (int32), beta [B, C], ssr [C], status [C], T"""
        i = self.info()
        breaks, beta = np.empty((i["B"], i["C"])), np.empty((i["B"], i["C"]))
        index, ssr = np.empty((i["B"], i["C"]), dtype=np.int32), np.empty(i["C"])
        status = self._export(i["C"], breaks, index, beta, ssr)
        return dict(breaks=breaks, break_index=index, beta=beta, ssr=ssr, status=status, T=i["T"])


class QmState(_FittedState):
    ABI = "sd_qm_state"
    INFO = (("T", C.c_int64), ("C", C.c_int64))
    PLANES = 2

    def export(self, with_y=True):
        i = self.info()
        xs = np.empty((i["C"], i["T"]))
        ys = np.empty((i["C"], i["T"])) if with_y else None
        return dict(x_sorted=xs, y_sorted=ys, status=self._export(i["C"], xs, ys))


class RegridState(_State):
    """Separable interpolation tables of one (source grid, target grid, method) on the device (sd_regrid_create)."""
    ABI = "sd_regrid"
    INFO = (("method", C.c_int), ("ny", C.c_int64), ("nx", C.c_int64), ("Ny", C.c_int64), ("Nx", C.c_int64))

    def apply(self, src, out=None):
        """src [T, ny, nx]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray -> [T, Ny * Nx]
        float64 DeviceArray, cells fastest (``out``: a [T, C] DeviceArray, possibly a cells() view of a wider one).  float32 goes to
        the device as float32 and is widened in the kernel."""
        i = self.info()
        src = self._source(src, i)
        T = src.shape[0]
        with self.ctx._uploads() as up:
            src = up(src)
            out = self.ctx._result_buffer(out, (T, i["Ny"] * i["Nx"]), True)
            self.ctx._same_context("sd_regrid", src=src, out=out)
            check(self.ctx.lib.sd_regrid_apply_dev(self.ctx.handle, self.vptr, src.vptr, _f32(src), T, out.vptr, out.ld))
        return out

    def apply_host(self, src):
        """host [T, ny, nx] -> host [T, Ny * Nx] through sd_regrid_apply (upload, run, download in one call)"""
        i = self.info()
        src = self._source(src, i)
        T = src.shape[0]
        return self.ctx._on_host("apply", self.ctx.lib.sd_regrid_apply, (T, i["Ny"] * i["Nx"]), self.vptr, src, _f32(src), T)

    @staticmethod
    def _source(src, i):
        if not isinstance(src, DeviceArray):
            src = _lib.as_field(src)
        if len(src.shape) != 3 or tuple(src.shape[1:]) != (i["ny"], i["nx"]) or src.shape[0] < 1:
            raise ValueError(f"src: expected a [T, {i['ny']}, {i['nx']}] field, got shape {tuple(src.shape)}")
        if isinstance(src, DeviceArray) and (src.dtype not in (np.float32, np.float64) or src.ld != src.shape[-1]):
            raise ValueError("src: expected a contiguous float32 or float64 DeviceArray")
        return src


class RemapState(_State):
    """Separable area-overlap tables of one (source grid, target grid) on the device (sd_remap_create)."""
    ABI = "sd_remap"
    INFO = tuple((key, C.c_int64) for key in ("ny", "nx", "Ny", "Nx", "y_entries", "x_entries"))

    def apply(self, field, min_valid=0.5, out=None):
        """field: a float32 / float64 host array [T, ny, nx] or [T, ny * nx] (any other dtype is taken as float64) or a DeviceArray
        [T, ny * nx] (rows ``ld`` apart) -> [T, Ny * Nx] float64 DeviceArray, cells fastest (``out``: a [T, C] DeviceArray, possibly a
        view of a wider or longer one).  float32 goes to the device as float32 and is widened in the kernel."""
        i = self.info()
        field, min_valid = self._args(field, i, min_valid)
        T = field.shape[0]
        with self.ctx._uploads() as up:
            field = up(field)
            out = self.ctx._result_buffer(out, (T, i["Ny"] * i["Nx"]), True)
            self.ctx._same_context("sd_remap", field=field, out=out)
            check(self.ctx.lib.sd_remap_apply_dev(self.ctx.handle, self.vptr, field.vptr, _f32(field), field.ld, T, min_valid, out.vptr, out.ld))
        return out

    def apply_host(self, field, min_valid=0.5):
        """host [T, ny, nx] -> host [T, Ny * Nx] through sd_remap_apply (upload, run, download in one call)"""
        i = self.info()
        if isinstance(field, DeviceArray):
            raise ValueError("apply_host: expected a host array")
        field, min_valid = self._args(field, i, min_valid)
        out = np.empty((field.shape[0], i["Ny"] * i["Nx"]))
        check(self.ctx.lib.sd_remap_apply(self.ctx.handle, self.vptr, ptr(field), _f32(field), field.shape[0], min_valid, ptr(out)))
        return out

    @staticmethod
    def _args(field, i, min_valid):
        cells = i["ny"] * i["nx"]
        if not isinstance(field, DeviceArray):
            field = _lib.as_field(field)
            if field.ndim == 3 and field.shape[1:] == (i["ny"], i["nx"]):
                field = field.reshape(field.shape[0], cells)
        if len(field.shape) != 2 or field.shape[1] != cells or field.shape[0] < 1 or field.dtype not in (np.float32, np.float64):
            raise ValueError(f"field: expected a float32 or float64 [T, {i['ny']}, {i['nx']}] or [T, {cells}] field, got shape "
                             f"{tuple(field.shape)} of {field.dtype}")
        min_valid = float(min_valid)
        if not 0.0 <= min_valid <= 1.0:
            raise ValueError(f"min_valid={min_valid!r}: expected a share of the covered area in [0, 1]")
        return field, min_valid


class Context:
    """One GPU + one HIP stream.  Calls on a context are serialised."""

    def __init__(self, device=0, lib_path=None):
        self.lib = _lib.load(lib_path)  # lib_path: development library with A/B switches (tests / tools only)
        h = C.c_void_p()
        check(self.lib.sd_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if self.handle is not None:
            self.lib.sd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ---- info / timing ----
    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_int64()
        check(self.lib.sd_ctx_device_info(self.handle, name, 256, C.byref(cu), C.byref(mem)))
        return dict(name=name.value.decode(), compute_units=cu.value, hbm_bytes=mem.value)

    def synchronize(self):
        check(self.lib.sd_ctx_synchronize(self.handle))

    def release_cached(self):
        """Give the context's cached device blocks (recycled state / scratch buffers) back to the driver."""
        check(self.lib.sd_ctx_release_cached(self.handle))

    def timer_start(self):
        check(self.lib.sd_timer_start(self.handle))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.sd_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def prof_enable(self, on=True):
        check(self.lib.sd_prof_enable(self.handle, 1 if on else 0))

    def prof_reset(self):
        check(self.lib.sd_prof_reset(self.handle))

    def prof(self):
        buf = C.create_string_buffer(4096)
        check(self.lib.sd_prof_names(self.handle, buf, 4096))
        out = {}
        for name in filter(None, buf.value.decode().split(";")):
            ms, n = C.c_double(), C.c_int64()
            check(self.lib.sd_prof_query(self.handle, name.encode(), C.byref(ms), C.byref(n)))
            out[name] = dict(ms=ms.value, launches=n.value)
        return out

    # ---- memory ----
    def empty(self, shape, dtype=np.float64):
        return DeviceArray(self, shape, dtype)

    def to_device(self, a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        return DeviceArray(self, a.shape, dtype).copy_from_host(a)

    # ---- float32 transport: a float32 host field crosses PCIe as float32 and is widened on the device (exact), a result
    # wanted as float32 is narrowed there (round to nearest, what ``.astype(np.float32)`` does on the host) ----
    @staticmethod
    def _is_f32_host(a):
        return isinstance(a, np.ndarray) and a.dtype == np.float32

    def widen_to_device(self, a32):
        """float32 host array -> float64 DeviceArray of the same shape (half the host-to-device bytes of an upcast on the host)"""
        a32 = np.ascontiguousarray(a32, dtype=np.float32)
        d32 = DeviceArray(self, a32.shape, np.float32).copy_from_host(a32)
        d64 = DeviceArray(self, a32.shape, np.float64)
        check(self.lib.sd_convert_f32_to_f64_dev(self.handle, d32.vptr, a32.size, d64.vptr))
        self.synchronize()
        d32.free()
        return d64

    def narrow_to_host(self, d64, out=None):
        """float64 DeviceArray (contiguous) -> float32 host array: narrowed on the device, half the device-to-host bytes"""
        if d64.ld != d64.shape[-1]:
            raise ValueError("narrow_to_host needs a contiguous DeviceArray")
        n = int(np.prod(d64.shape, dtype=np.int64))
        d32 = DeviceArray(self, d64.shape, np.float32)
        check(self.lib.sd_convert_f64_to_f32_dev(self.handle, d64.vptr, n, d32.vptr))
        res = np.empty(d64.shape, dtype=np.float32) if out is None else out
        check(self.lib.sd_memcpy_d2h(self.handle, ptr(res), d32.vptr, res.nbytes))
        d32.free()
        return res

    def wrap(self, dptr, shape, dtype=np.float64):
        """View foreign device memory (e.g. a torch tensor's data_ptr()) without owning it."""
        return DeviceArray(self, shape, dtype, dptr=int(dptr), owner=False)

    def synth_fill(self, out, kind, seed, stream, c_offset=0, c_full=None, base=None, amp=1.0, cell_scale=0.0,
                   p_dry=0.0, stream2=None, amp2=0.0):
        T, Cc = out.shape
        c_full = Cc if c_full is None else c_full
        b = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
        check(self.lib.sd_synth_fill(self.handle, out.vptr, T, Cc, out.ld, c_offset, c_full, kind, seed, stream, ptr(b), amp,
                                     cell_scale, p_dry, -1 if stream2 is None else stream2, amp2))
        return out

    # ---- the argument layer of the estimator wrappers: the C ABI takes raw pointers and cannot check them, so every field, result
    # buffer and state passes one of these before it reaches the library ----
    def _same_context(self, who, **arrays):
        for name, a in arrays.items():
            if a is not None and a.ctx is not self:
                raise ValueError(f"sd_downscale: {who}: `{name}` belongs to another context")

    def _result_buffer(self, out, shape, on_device, who=None):
        """the caller's result buffer, checked (a wrong one would be written past its end), or a fresh one; with ``who`` a resident one
        must also be this context's"""
        if out is None:
            return self.empty(shape) if on_device else np.empty(shape)
        if on_device:
            if not isinstance(out, DeviceArray) or tuple(out.shape) != tuple(shape) or out.dtype != np.float64 or out.ld < shape[-1]:
                raise ValueError(f"out: expected a float64 DeviceArray of shape {tuple(shape)}")
            if who is not None:
                self._same_context(who, out=out)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == tuple(shape) and out.flags["C_CONTIGUOUS"]):
            raise ValueError(f"out: expected a C-contiguous float64 array of shape {tuple(shape)}")
        return out

    @staticmethod
    def _float64(name, a, layout):
        """``a`` as the estimator entry points read a field: a float64 DeviceArray as it is, a host array made contiguous float64"""
        if not isinstance(a, DeviceArray):
            return _lib.as_f64(a)
        if a.dtype != np.float64:  # (it would be read to twice its length)
            raise ValueError(f"{name}: expected a float64 {layout} field, got shape {tuple(a.shape)} of {a.dtype}")
        return a

    @staticmethod
    def _field(name, a, *dims):
        """a field of rank ``len(dims)`` (numpy or DeviceArray, None stays None) with the expected sizes: a number in ``dims`` is the
        size that axis must have, a string only names the axis in the refusal"""
        if a is None:
            return None
        layout = f"[{', '.join(str(d) for d in dims)}]"
        a = Context._float64(name, a, layout)
        if len(a.shape) != len(dims) or any(not isinstance(d, str) and s != d for s, d in zip(a.shape, dims)):
            raise ValueError(f"{name}: expected a {layout} field, got shape {tuple(a.shape)}")
        return a

    @staticmethod
    def _train3(X, y, same_kind=""):
        """the training pair X [T, F, C], y [T, C] of the analog and regression fits -> (X, y, the words that refuse the pair)"""
        X, y = Context._float64("X", X, "[T, F, C]"), Context._float64("y", y, "[T, C]")
        words = f"expected X [T, F, C] and y [T, C]{same_kind}, got {tuple(X.shape)} and {tuple(y.shape)}"
        if len(X.shape) != 3 or tuple(y.shape) != (X.shape[0], X.shape[2]):
            raise ValueError(words)
        return X, y, words

    @staticmethod
    def _beside(X, y):
        """``y`` beside ``X``: a resident y that comes with a host X joins it on the host"""
        return y.to_host() if isinstance(y, DeviceArray) and not isinstance(X, DeviceArray) else y

    @staticmethod
    def _threshold(thresh):
        return (0, 0.0) if thresh is None else (1, float(thresh))

    _ONE_PITCH = "X and y: expected two DeviceArrays with the same row pitch"

    def _resident(self, who, one_ld=(), mixed=None, **arrays):
        """The residency rule, -> True for the resident form of a call: its array arguments (None: not given) are all host arrays or
        all DeviceArrays of this context, and the resident ones named in ``one_ld``, for which the ABI has one ``ld``, share their
        row pitch."""
        given = {name: a for name, a in arrays.items() if a is not None}
        on = [isinstance(a, DeviceArray) for a in given.values()]
        if any(on) != all(on):
            raise ValueError(mixed or f"{' and '.join(given)} must both be host arrays or both be DeviceArrays")
        if not any(on):
            return False
        self._same_context(who, **given)
        if len({given[name].ld for name in one_ld if name in given}) > 1:
            raise ValueError(self._ONE_PITCH)
        return True

    def _info_of(self, who, state):
        """``state.info()`` of a state of this context"""
        self._same_context(who, state=state)
        return state.info()

    def _create(self, cls, fn, *args):
        """the creating call ``fn(*args, &handle)`` -> the handle as a ``cls``"""
        h = C.c_void_p()
        check(fn(*args, C.byref(h)))
        return cls(self, h.value)

    # ---- BCSD ----
    @staticmethod
    def _group_ids(name, gid, T, G):
        gid = _lib.as_i32(gid)
        if gid.shape != (T,):
            raise ValueError(f"{name}: expected {T} group ids, got shape {gid.shape}")
        if T and (gid.min() < 0 or gid.max() >= G):
            raise ValueError(f"{name}: group ids must lie in [0, {G})")
        return gid

    @staticmethod
    def _bcsd_options(return_anoms, detrend):
        return (_lib.BCSD_RETURN_ANOMS if return_anoms else 0) | (_lib.BCSD_QM_DETREND if detrend else 0)

    def bcsd_fit(self, kind, X, y, gid, G, return_anoms=True, detrend=False):
        """X, y: numpy [T,C] (host path) or DeviceArray [T,C] (resident path); X may be None for PR.  ``detrend``:
        qm_kwargs={'detrend': True} (quantile.py:95-98,128-145)."""
        flags = self._bcsd_options(return_anoms, detrend)
        if self._is_f32_host(y) and (X is None or self._is_f32_host(X)) and y.ndim == 2 and y.size > 0:
            y = self.widen_to_device(y)  # float32 grids: 4 bytes per sample over PCIe, widened in HBM
            X = None if X is None else self.widen_to_device(X)
        y = self._field("y", y, "T", "C")
        X = self._field("X", X, *y.shape)
        dev = self._resident("sd_bcsd_fit", ("X", "y"), X=X, y=y)
        T, Cc = y.shape
        gid = self._group_ids("group_id", gid, T, G)
        if dev:
            return self._create(BcsdState, self.lib.sd_bcsd_fit_dev, self.handle, kind, vptr(X), y.vptr, y.ld, ptr(gid), G, T, Cc, flags)
        return self._create(BcsdState, self.lib.sd_bcsd_fit, self.handle, kind, ptr(X), ptr(y), ptr(gid), G, T, Cc, flags)

    def bcsd_fit_groups(self, kind, X, y, order, offsets, return_anoms=True, detrend=False):
        """Fit on explicitly listed (possibly overlapping) groups: ``order`` = time indices group by group,
        ``offsets[G+1]`` (time_grouper='daily_nasa-nex': bcsd.py:36-38,50-55)."""
        flags = self._bcsd_options(return_anoms, detrend)
        y = self._field("y", y, "T", "C")
        X = self._field("X", X, *y.shape)
        T, Cc = y.shape
        order = _lib.as_i32(order)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        G = len(offsets) - 1
        if G < 1 or offsets[0] != 0 or offsets[-1] != len(order) or (np.diff(offsets) < 0).any():
            raise ValueError("group offsets must start at 0, not decrease and end at len(order)")
        if len(order) and (order.min() < 0 or order.max() >= T):
            raise ValueError(f"group order entries must lie in [0, {T})")
        if self._resident("sd_bcsd_fit_groups", ("X", "y"), X=X, y=y):
            return self._create(BcsdState, self.lib.sd_bcsd_fit_groups_dev, self.handle, kind, vptr(X), y.vptr, y.ld, ptr(order),
                                ptr(offsets), G, T, Cc, flags)
        return self._create(BcsdState, self.lib.sd_bcsd_fit_groups, self.handle, kind, ptr(X), ptr(y), ptr(order), ptr(offsets), G, T, Cc,
                            flags)

    def bcsd_import(self, exported):
        i = exported["info"]
        detrend = i.get("detrend", False)
        if detrend:
            trend = _lib.as_f64(exported["y_trend"])
            if trend.shape != (i["C"], i["G"], 2):
                raise ValueError(f"y_trend: expected shape {(i['C'], i['G'], 2)}, got {trend.shape}")
        st = self._create(BcsdState, self.lib.sd_bcsd_state_import, self.handle, i["kind"], i["G"], i["T"], i["C"],
                          self._bcsd_options(i["return_anoms"], detrend), ptr(_lib.as_f64(exported["y_sorted"])),
                          ptr(_lib.as_f64(exported["x_climo"])), ptr(_lib.as_f64(exported["y_climo"])), ptr(_lib.as_i32(exported["status"])),
                          ptr(np.ascontiguousarray(exported["group_offsets"], dtype=np.int64)))
        if detrend:
            check(self.lib.sd_bcsd_state_set_trend(st.vptr, ptr(trend)))
        return st

    def bcsd_predict(self, state, Xp, gid_p, out=None, out_dtype=None):
        """``out_dtype=np.float32`` with a float32 host ``Xp``: the field goes in and the result comes back as float32
        (widened / narrowed on the device); everything else as before (float64 results)."""
        info = self._info_of("sd_bcsd_predict", state)
        want32 = out_dtype is not None and np.dtype(out_dtype) == np.float32
        if out_dtype is not None and not want32 and np.dtype(out_dtype) != np.float64:
            raise ValueError("bcsd_predict: out_dtype must be float64 or float32")
        if self._is_f32_host(Xp) and Xp.ndim == 2 and Xp.size > 0 and out is None:
            d_out, status = self.bcsd_predict(state, self.widen_to_device(Xp), gid_p)
            return (self.narrow_to_host(d_out) if want32 else d_out.to_host()), status
        if want32:  # (float64 or resident input: the result is narrowed where it is)
            if out is not None:
                raise ValueError("bcsd_predict: out_dtype=float32 does not combine with a float64 `out` buffer")
            res, status = self.bcsd_predict(state, Xp, gid_p)
            return (self.narrow_to_host(res) if isinstance(res, DeviceArray) else res.astype(np.float32)), status
        Cc = info["C"]
        Xp = self._field("X", Xp, "T", Cc)
        Tp = Xp.shape[0]
        gid_p = self._group_ids("group_id", gid_p, Tp, info["G"])
        dev = self._resident("sd_bcsd_predict", X=Xp)
        out = self._result_buffer(out, (Tp, Cc), dev, "sd_bcsd_predict")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_bcsd_predict_dev(self.handle, state.vptr, Xp.vptr, Xp.ld, ptr(gid_p), Tp, out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_bcsd_predict(self.handle, state.vptr, ptr(Xp), ptr(gid_p), Tp, ptr(out), ptr(status)))
        return out, status

    def bcsd_predict_trend(self, state, Xp, gid_p, gid_trend, G_trend, out=None):
        """Predict with a climate-trend grouper of its own: rolling mean over ``gid_trend`` groups, climatologies and
        quantile mapping over ``gid_p`` (groups of the state) -- bcsd.py:247-267."""
        info = self._info_of("sd_bcsd_predict_trend", state)
        Cc = info["C"]
        Xp = self._field("X", Xp, "T", Cc)
        Tp = Xp.shape[0]
        gid_p = self._group_ids("group_id", gid_p, Tp, info["G"])
        gid_trend = self._group_ids("trend_group_id", gid_trend, Tp, G_trend)
        dev = self._resident("sd_bcsd_predict_trend", X=Xp)
        out = self._result_buffer(out, (Tp, Cc), dev, "sd_bcsd_predict_trend")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_bcsd_predict_trend_dev(self.handle, state.vptr, Xp.vptr, Xp.ld, ptr(gid_p), ptr(gid_trend), G_trend, Tp,
                                                     out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_bcsd_predict_trend(self.handle, state.vptr, ptr(Xp), ptr(gid_p), ptr(gid_trend), G_trend, Tp, ptr(out),
                                                 ptr(status)))
        return out, status

    def bcsd_fit_predict(self, kind, X, y, gid, G, Xp, gid_p, return_anoms=True, out=None, detrend=False):
        """Fused resident path (DeviceArrays only)."""
        flags = self._bcsd_options(return_anoms, detrend)
        y = self._field("y", y, "T", "C")
        X = self._field("X", X, *y.shape)
        Xp = self._field("Xp", Xp, "T", y.shape[1])
        resident_only = "bcsd_fit_predict takes resident fields: X, y and Xp must be DeviceArrays"
        if not self._resident("sd_bcsd_fit_predict", ("X", "y"), resident_only, X=X, y=y, Xp=Xp):
            raise ValueError(resident_only)
        T, Cc = y.shape
        Tp = Xp.shape[0]
        gid, gid_p = self._group_ids("group_id", gid, T, G), self._group_ids("group_id_p", gid_p, Tp, G)
        out = self._result_buffer(out, (Tp, Cc), True, "sd_bcsd_fit_predict")
        status = np.empty(Cc, dtype=np.int32)
        check(self.lib.sd_bcsd_fit_predict_dev(self.handle, kind, vptr(X), y.vptr, y.ld, ptr(gid), G, T, Cc, flags, Xp.vptr, Xp.ld, ptr(gid_p),
                                               Tp, out.vptr, out.ld, ptr(status)))
        return out, status

    # ---- quantile-mapping regressors ----
    def qm_fit(self, X, y=None):
        """X, y [T, C] numpy or DeviceArray -> QmState (sorted series per cell); y=None keeps only the CDF of X
        (CunnaneTransformer)."""
        X = self._field("X", X, "T", "C")
        y = self._field("y", y, *X.shape)
        T, Cc = X.shape
        if self._resident("sd_qm_fit", ("X", "y"), X=X, y=y):
            return self._create(QmState, self.lib.sd_qm_fit_dev, self.handle, X.vptr, vptr(y), X.ld, T, Cc)
        return self._create(QmState, self.lib.sd_qm_fit, self.handle, ptr(X), ptr(y), T, Cc)

    def qm_cunnane(self, state, direction, X, extrapolate="both", n_endpoints=10, out=None):
        """CunnaneTransformer.transform (direction 0) / inverse_transform (1) of X [Tp, C] on the fitted CDFs."""
        Cc = self._info_of("sd_qm_cunnane", state)["C"]
        X = self._field("X", X, "T", Cc)
        if extrapolate not in _lib.EXTRAP_CODES:
            raise ValueError(f"unknown value for extrapolate: {extrapolate}")
        code = _lib.EXTRAP_CODES[extrapolate]
        Tp = X.shape[0]
        dev = self._resident("sd_qm_cunnane", X=X)
        out = self._result_buffer(out, (Tp, Cc), dev, "sd_qm_cunnane")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_qm_cunnane_dev(self.handle, state.vptr, int(direction), code, int(n_endpoints), X.vptr, X.ld, Tp,
                                             out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_qm_cunnane(self.handle, state.vptr, int(direction), code, int(n_endpoints), ptr(X), Tp, ptr(out), ptr(status)))
        return out, status

    def qm_predict(self, state, model, Xp, extrapolate=None, n_endpoints=10, out=None):
        """extrapolate: None, 'min', 'max', 'both' or '1to1' (``True`` is accepted for '1to1')."""
        extrapolate = "1to1" if extrapolate is True else (None if extrapolate is False else extrapolate)
        if extrapolate not in _lib.QM_EXTRAP_CODES:
            raise ValueError(f"unknown value for extrapolate: {extrapolate}")
        code = _lib.QM_EXTRAP_CODES[extrapolate]
        Cc = self._info_of("sd_qm_predict", state)["C"]
        Xp = self._field("X", Xp, "T", Cc)
        Tp = Xp.shape[0]
        dev = self._resident("sd_qm_predict", X=Xp)
        out = self._result_buffer(out, (Tp, Cc), dev, "sd_qm_predict")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_qm_predict_dev(self.handle, state.vptr, int(model), code, int(n_endpoints), Xp.vptr, Xp.ld, Tp,
                                             out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_qm_predict(self.handle, state.vptr, int(model), code, int(n_endpoints), ptr(Xp), Tp, ptr(out), ptr(status)))
        return out, status

    # ---- analogs ----
    def analog_fit(self, X, y):
        """X [T,F,C], y [T,C] numpy or DeviceArray."""
        X, y, words = self._train3(X, y, " of the same kind")
        T, F, Cc = X.shape
        if self._resident("sd_analog_fit", ("X", "y"), words, X=X, y=y):
            return self._create(AnalogState, self.lib.sd_analog_fit_dev, self.handle, X.vptr, y.vptr, y.ld, T, F, Cc)
        return self._create(AnalogState, self.lib.sd_analog_fit, self.handle, ptr(X), ptr(y), T, F, Cc)

    def _queries(self, who, state, Xq):
        """Xq [Tq, F, C] for a fitted state of F features and C cells -> (Xq, the state's info, resident?)"""
        info = self._info_of(who, state)
        Xq = self._field("Xq", Xq, "Tq", info["F"], info["C"])
        return Xq, info, self._resident(who, Xq=Xq)

    def analog_predict(self, state, Xq, k, kind, thresh=None, sample_inds=None, want_neighbors=False, out=None):
        Xq, info, dev = self._queries("sd_analog_predict", state, Xq)
        Tq, Cc = Xq.shape[0], info["C"]
        k = int(k)
        if k < 1 or k > info["T"]:
            raise ValueError(f"k={k}: expected 1 <= k <= {info['T']} (the number of training samples)")
        if sample_inds is not None:
            resident = isinstance(sample_inds, DeviceArray)
            if not resident:
                sample_inds = _lib.as_i32(sample_inds)
            if tuple(sample_inds.shape) != (Tq, Cc):
                raise ValueError(f"sample_inds: expected shape {(Tq, Cc)}, got {tuple(sample_inds.shape)}")
            if not resident and len(sample_inds) and (np.min(sample_inds) < 0 or np.max(sample_inds) >= k):
                raise ValueError(f"sample_inds must lie in [0, {k})")
            if resident:  # (host indices also go beside a resident Xq: they are uploaded below)
                if sample_inds.dtype != np.int32 or sample_inds.ld != Cc:
                    raise ValueError(f"sample_inds: expected a contiguous int32 DeviceArray, got pitch {sample_inds.ld} of {sample_inds.dtype}")
                self._resident("sd_analog_predict", Xq=Xq, sample_inds=sample_inds)
        out = self._result_buffer(out, (Tq, 3, Cc), dev, "sd_analog_predict")
        if dev and want_neighbors and out.ld != Cc:
            raise ValueError("analog_predict: the neighbour fields share the pitch of `out`, which must be contiguous here")
        has_t, tv = self._threshold(thresh)
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            samp = sample_inds if sample_inds is None or isinstance(sample_inds, DeviceArray) else self.to_device(sample_inds, np.int32)
            inds = self.empty((Tq, k, Cc), np.int64) if want_neighbors else None
            dist = self.empty((Tq, k, Cc)) if want_neighbors else None
            check(self.lib.sd_analog_predict_dev(self.handle, state.vptr, Xq.vptr, Xq.ld, Tq, k, kind, has_t, tv, vptr(samp), out.vptr, out.ld,
                                                 vptr(inds), vptr(dist), ptr(status)))
        else:
            inds = np.empty((Tq, k, Cc), dtype=np.int64) if want_neighbors else None
            dist = np.empty((Tq, k, Cc)) if want_neighbors else None
            check(self.lib.sd_analog_predict(self.handle, state.vptr, ptr(Xq), Tq, k, kind, has_t, tv, ptr(sample_inds), ptr(out),
                                             ptr(inds), ptr(dist), ptr(status)))
        return (out, status, inds, dist) if want_neighbors else (out, status)

    def analogreg_predict(self, state, Xq, k, thresh=None, out=None):
        """AnalogRegression.predict for every cell; ``thresh``: exceedance probability by logistic regression on the analogs
        (gard.py:201-212), linear model on the exceeding analogs."""
        Xq, info, dev = self._queries("sd_analogreg_predict", state, Xq)
        Tq, Cc = Xq.shape[0], info["C"]
        out = self._result_buffer(out, (Tq, 3, Cc), dev, "sd_analogreg_predict")
        has, thr = self._threshold(thresh)
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_analogreg_predict_dev(self.handle, state.vptr, Xq.vptr, Xq.ld, Tq, int(k), has, thr, out.vptr, out.ld,
                                                    ptr(status)))
        else:
            check(self.lib.sd_analogreg_predict(self.handle, state.vptr, ptr(Xq), Tq, int(k), has, thr, ptr(out), ptr(status)))
        return out, status

    def analog_fit_predict(self, X, y, Xq, k, kind, thresh=None, out=None):
        """AnalogBase.fit + PureAnalog.predict in one call without a fitted state (sd_analog_fit_predict*): X [T,F,C], y [T,C],
        Xq [Tq,F,C], all numpy or all DeviceArray -> (out [Tq,3,C], status [C]); bit-identical to analog_fit -> analog_predict."""
        dev = self._resident("sd_analog_fit_predict", ("X", "y"), "X, y and Xq must all be numpy arrays or all DeviceArrays", X=X, y=y, Xq=Xq)
        X, y, _ = self._train3(X, y)
        T, F, Cc = X.shape
        Xq = self._field("Xq", Xq, "Tq", F, Cc)
        Tq = Xq.shape[0]
        k = int(k)
        if k < 1 or k > T:
            raise ValueError(f"k={k}: expected 1 <= k <= {T} (the number of training samples)")
        out = self._result_buffer(out, (Tq, 3, Cc), dev, "sd_analog_fit_predict")
        has_t, tv = self._threshold(thresh)
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_analog_fit_predict_dev(self.handle, X.vptr, y.vptr, y.ld, T, F, Cc, Xq.vptr, Xq.ld, Tq, k, kind, has_t, tv,
                                                     out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_analog_fit_predict(self.handle, ptr(X), ptr(y), T, F, Cc, ptr(Xq), Tq, k, kind, has_t, tv, ptr(out), ptr(status)))
        return out, status

    # ---- PureRegression (thresh=None) ----
    def linreg_fit(self, X, y, thresh=None):
        """X [T,F,C], y [T,C] numpy or DeviceArray -> LinregState (coefficients, intercept, fit error per cell; with ``thresh``
        also the logistic model of the exceedance probability, gard.py:416-437)."""
        X, y, words = self._train3(X, y, " of the same kind")
        T, F, Cc = X.shape
        has, thr = self._threshold(thresh)
        if self._resident("sd_linreg_fit", ("X", "y"), words, X=X, y=y):
            return self._create(LinregState, self.lib.sd_linreg_fit_dev, self.handle, X.vptr, y.vptr, y.ld, T, F, Cc, has, thr)
        return self._create(LinregState, self.lib.sd_linreg_fit, self.handle, ptr(X), ptr(y), T, F, Cc, has, thr)

    def linreg_import(self, exported):
        """device state from ``LinregState.export()`` (pickling, checkpoint / resume)"""
        coef = _lib.as_f64(exported["coef"])
        F, Cc = coef.shape
        logit = dropped = None
        if "logistic_coef" in exported:
            logit = _lib.as_f64(np.vstack([exported["logistic_coef"], np.asarray(exported["logistic_intercept"]).reshape(1, Cc)]))
            dropped = _lib.as_i32(exported["thresh_dropped"])
        return self._create(LinregState, self.lib.sd_linreg_state_import, self.handle, int(exported["T"]), F, Cc, ptr(coef),
                            ptr(_lib.as_f64(exported["intercept"])), ptr(_lib.as_f64(exported["fit_error"])), ptr(logit), ptr(dropped),
                            ptr(_lib.as_i32(exported["status"])))

    def linreg_predict(self, state, Xq, out=None):
        Xq, info, dev = self._queries("sd_linreg_predict", state, Xq)
        Tq, Cc = Xq.shape[0], info["C"]
        out = self._result_buffer(out, (Tq, 3, Cc), dev, "sd_linreg_predict")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_linreg_predict_dev(self.handle, state.vptr, Xq.vptr, Xq.ld, Tq, out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_linreg_predict(self.handle, state.vptr, ptr(Xq), Tq, ptr(out), ptr(status)))
        return out, status

    # ---- ZScoreRegressor ----
    def zscore_fit(self, X, y, window_width, day_idx, year, D):
        """X, y [T, C] (numpy or DeviceArray); day_idx / year: host [T] (sd_zscore_fit) -> ZscoreState"""
        X = self._field("X", X, "T", "C")
        y = self._field("y", self._beside(X, y), *X.shape)
        T, Cc = X.shape
        day_idx, year = _lib.as_i32(day_idx), _lib.as_i32(year)
        if day_idx.shape != (T,) or year.shape != (T,):
            raise ValueError(f"day_idx and year: expected {T} entries, got {day_idx.shape} and {year.shape}")
        if self._resident("sd_zscore_fit", ("X", "y"), self._ONE_PITCH, X=X, y=y):
            return self._create(ZscoreState, self.lib.sd_zscore_fit_dev, self.handle, X.vptr, y.vptr, X.ld, T, Cc, int(window_width),
                                ptr(day_idx), ptr(year), int(D))
        return self._create(ZscoreState, self.lib.sd_zscore_fit, self.handle, ptr(X), ptr(y), T, Cc, int(window_width), ptr(day_idx),
                            ptr(year), int(D))

    def zscore_import(self, exported):
        """device state from ``ZscoreState.export()`` (pickling)"""
        planes = [_lib.as_f64(exported[k]) for k in ZscoreState.STATS]
        K, Cc = planes[0].shape
        if any(p.shape != (K, Cc) for p in planes):
            raise ValueError("zscore_import: the six planes must share one [K, C] shape")
        return self._create(ZscoreState, self.lib.sd_zscore_state_import, self.handle, K, Cc, int(exported["window_width"]),
                            *[ptr(p) for p in planes], ptr(_lib.as_i32(exported["status"])))

    def zscore_predict(self, state, Xp, out=None, with_stats=False):
        """Xp [Tp, C] -> (out [Tp, C], cell status [C], stats): stats = dict(meani, stdi, meanf, stdf) of [Tp, C] fields (on the
        device for a DeviceArray input) when ``with_stats``, else None"""
        Cc = self._info_of("sd_zscore_predict", state)["C"]
        Xp = self._field("Xp", Xp, "T", Cc)
        Tp = Xp.shape[0]
        dev = self._resident("sd_zscore_predict", Xp=Xp)
        out = self._result_buffer(out, (Tp, Cc), dev, "sd_zscore_predict")
        if dev and with_stats and out.ld != Cc:
            raise ValueError("zscore_predict: the stats fields share the pitch of `out`, which must be contiguous here")
        stats = {k: (self.empty((Tp, Cc)) if dev else np.empty((Tp, Cc))) for k in ("meani", "stdi", "meanf", "stdf")} if with_stats else None
        sp = [None] * 4 if stats is None else [s.vptr if dev else ptr(s) for s in stats.values()]
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_zscore_predict_dev(self.handle, state.vptr, Xp.vptr, Xp.ld, Tp, out.vptr, out.ld, *sp, ptr(status)))
        else:
            check(self.lib.sd_zscore_predict(self.handle, state.vptr, ptr(Xp), Tp, ptr(out), *sp, ptr(status)))
        return out, status, stats

    # ---- GroupedRegressor ----
    def grouped_fit(self, X, y, key, n, window):
        """X [T, F, C], y [T, C] (numpy or DeviceArray); key: host [T] in [0, n) (sd_grouped_fit) -> GroupedState"""
        X = self._field("X", X, "T", "F", "C")
        T, F, Cc = X.shape
        y = self._field("y", self._beside(X, y), T, Cc)
        key = _lib.as_i32(key)
        if key.shape != (T,):
            raise ValueError(f"key: expected {T} entries, got shape {key.shape}")
        if self._resident("sd_grouped_fit", ("X", "y"), self._ONE_PITCH, X=X, y=y):
            return self._create(GroupedState, self.lib.sd_grouped_fit_dev, self.handle, X.vptr, y.vptr, X.ld, T, F, Cc, ptr(key), int(n),
                                int(window))
        return self._create(GroupedState, self.lib.sd_grouped_fit, self.handle, ptr(X), ptr(y), T, F, Cc, ptr(key), int(n), int(window))

    def grouped_import(self, exported):
        """device state from ``GroupedState.export()`` (pickling)"""
        coef, icpt = _lib.as_f64(exported["coef"]), _lib.as_f64(exported["intercept"])
        n, F, Cc = coef.shape
        fitted = _lib.as_i32(exported["fitted"])
        if icpt.shape != (n, Cc) or fitted.shape != (n,):
            raise ValueError("grouped_import: expected coef [n, F, C], intercept [n, C] and fitted [n]")
        return self._create(GroupedState, self.lib.sd_grouped_state_import, self.handle, n, F, Cc, int(exported["window"]), ptr(coef),
                            ptr(icpt), ptr(fitted), ptr(_lib.as_i32(exported["status"])))

    def grouped_predict(self, state, Xq, key, out=None):
        """Xq [Tq, F, C], key: host [Tq] -> (out [Tq, C], cell status [C]); a key without a fitted model is a ValueError"""
        Xq, info, dev = self._queries("sd_grouped_predict", state, Xq)
        Tq, Cc = Xq.shape[0], info["C"]
        key = _lib.as_i32(key)
        if key.shape != (Tq,):
            raise ValueError(f"key: expected {Tq} entries, got shape {key.shape}")
        out = self._result_buffer(out, (Tq, Cc), dev, "sd_grouped_predict")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_grouped_predict_dev(self.handle, state.vptr, Xq.vptr, Xq.ld, Tq, ptr(key), out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_grouped_predict(self.handle, state.vptr, ptr(Xq), Tq, ptr(key), ptr(out), ptr(status)))
        return out, status

    # ---- PiecewiseLinearRegression(fit_option='arrm') ----
    def arrm_fit(self, X, y, max_breakpoints, with_r2=False):
        """X, y [T, C] (numpy or DeviceArray) -> ArrmState, or (ArrmState, r2 [T, C]) with ``with_r2`` (sd_arrm_fit)"""
        X = self._field("X", X, "T", "C")
        y = self._field("y", self._beside(X, y), *X.shape)
        T, Cc = X.shape
        if self._resident("sd_arrm_fit", ("X", "y"), self._ONE_PITCH, X=X, y=y):
            r2 = self.empty((T, Cc)) if with_r2 else None
            state = self._create(ArrmState, self.lib.sd_arrm_fit_dev, self.handle, X.vptr, y.vptr, X.ld, T, Cc, int(max_breakpoints), vptr(r2))
        else:
            r2 = np.empty((T, Cc)) if with_r2 else None
            state = self._create(ArrmState, self.lib.sd_arrm_fit, self.handle, ptr(X), ptr(y), T, Cc, int(max_breakpoints), ptr(r2))
        return (state, r2) if with_r2 else state

    def arrm_import(self, exported):
        """device state from ``ArrmState.export()`` (pickling)"""
        breaks, beta = _lib.as_f64(exported["breaks"]), _lib.as_f64(exported["beta"])
        B, Cc = breaks.shape
        index, ssr = _lib.as_i32(exported["break_index"]), _lib.as_f64(exported["ssr"])
        if beta.shape != (B, Cc) or index.shape != (B, Cc) or ssr.shape != (Cc,):
            raise ValueError("arrm_import: expected breaks, break_index and beta [B, C] and ssr [C]")
        return self._create(ArrmState, self.lib.sd_arrm_state_import, self.handle, B, Cc, int(exported["T"]), ptr(breaks), ptr(index),
                            ptr(beta), ptr(ssr), ptr(_lib.as_i32(exported["status"])))

    def arrm_predict(self, state, Xq, out=None):
        """Xq [Tq, C] -> (out [Tq, C], cell status [C])"""
        Cc = self._info_of("sd_arrm_predict", state)["C"]
        Xq = self._field("Xq", Xq, "T", Cc)
        Tq = Xq.shape[0]
        dev = self._resident("sd_arrm_predict", Xq=Xq)
        out = self._result_buffer(out, (Tq, Cc), dev, "sd_arrm_predict")
        status = np.empty(Cc, dtype=np.int32)
        if dev:
            check(self.lib.sd_arrm_predict_dev(self.handle, state.vptr, Xq.vptr, Xq.ld, Tq, out.vptr, out.ld, ptr(status)))
        else:
            check(self.lib.sd_arrm_predict(self.handle, state.vptr, ptr(Xq), Tq, ptr(out), ptr(status)))
        return out, status

    # ---- regridding (GridArray.interp_like) ----
    def regrid_create(self, src_y, src_x, dst_y, dst_x, method="linear"):
        """Tables that take a [T, len(src_y), len(src_x)] field onto the (dst_y, dst_x) grid -> RegridState"""
        if method not in _lib.REGRID_METHODS:
            raise NotImplementedError(f"regrid method {method!r}: expected 'linear' or 'nearest'")
        sy, sx, dy, dx = (_lib.as_f64(np.ravel(a)) for a in (src_y, src_x, dst_y, dst_x))
        return self._create(RegridState, self.lib.sd_regrid_create, self.handle, _lib.REGRID_METHODS[method], len(sy), len(sx), ptr(sy),
                            ptr(sx), len(dy), len(dx), ptr(dy), ptr(dx))

    # ---- conservative remapping (GridArray.remap_like) ----
    def remap_create(self, src_yb, src_xb, dst_yb, dst_xb):
        """Area-overlap tables that take a [T, len(src_yb) - 1, len(src_xb) - 1] field onto the grid whose cell bounds are
        (dst_yb, dst_xb); every bounds array is strictly ascending or descending, in the units whose differences are the weights
        -> RemapState"""
        b = {}
        for name, a in (("src_yb", src_yb), ("src_xb", src_xb), ("dst_yb", dst_yb), ("dst_xb", dst_xb)):
            a = np.asarray(a)
            if a.ndim != 1 or len(a) < 2:
                raise ValueError(f"{name}: expected the n + 1 bounds of n >= 1 cells, got shape {a.shape}")
            b[name] = _lib.as_f64(a)
        return self._create(RemapState, self.lib.sd_remap_create, self.handle, len(b["src_yb"]) - 1, len(b["src_xb"]) - 1, ptr(b["src_yb"]),
                            ptr(b["src_xb"]), len(b["dst_yb"]) - 1, len(b["dst_xb"]) - 1, ptr(b["dst_yb"]), ptr(b["dst_xb"]))

    def remap_host(self, field, src_yb, src_xb, dst_yb, dst_xb, min_valid=0.5):
        """host [T, ny, nx] -> host [T, Ny * Nx]: tables, upload, run, download (sd_remap_create + sd_remap_apply)"""
        state = self.remap_create(src_yb, src_xb, dst_yb, dst_xb)
        try:
            return state.apply_host(field, min_valid)
        finally:
            state.close()

    # ---- the argument layer of the time-axis and analog-library wrappers, on top of the one above (_field, _result_buffer,
    # _same_context) ----
    @staticmethod
    def _time_field(field, name="field", rows="T"):
        """a [T, C] field as the time-axis kernels take it: a DeviceArray, or a host array as float32 / float64"""
        if not isinstance(field, DeviceArray):
            field = _lib.as_field(field)
        if len(field.shape) != 2 or field.dtype not in (np.float32, np.float64):
            raise ValueError(f"{name}: expected a float32 or float64 [{rows}, C] field, got shape {tuple(field.shape)} of {field.dtype}")
        return field

    @staticmethod
    def _pair(a, b):
        """the two fields of a paired call, checked alike"""
        a, b = Context._time_field(a, "a"), Context._time_field(b, "b")
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"b: expected a [T, C] field of shape {tuple(a.shape)} like a, got shape {tuple(b.shape)}")
        return a, b

    @staticmethod
    def _stat_codes(who, stats, table, noun):
        """one name or a list of names of ``table`` -> their codes [nstat] as the ABI reads them"""
        stats = [stats] if isinstance(stats, str) else list(stats)
        for s in stats:
            if s not in table:
                raise ValueError(f"{noun} {s!r}: expected one of {', '.join(repr(k) for k in table)}")
        if not 1 <= len(stats) <= len(table):
            raise ValueError(f"sd_downscale: {who}: nstat = {len(stats)}, expected 1 to {len(table)} statistics")
        return np.ascontiguousarray([table[s] for s in stats], dtype=np.intc)

    @staticmethod
    def _sizes(who, **sizes):
        """a size below 1 leaves nothing to allocate a result for: refused here, in the words of the plan's refusal"""
        if min(sizes.values()) < 1:
            raise ValueError(f"sd_downscale: {who}: bad sizes ({', '.join(f'{name}={n}' for name, n in sizes.items())})")

    @staticmethod
    def _offsets(offsets):
        """the bin table [M + 1] -> (offsets as host int64, M)"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError(f"offsets: expected a table of M + 1 entries, got shape {offsets.shape}")
        return offsets, len(offsets) - 1

    @staticmethod
    def _bins(who, offsets, T, Cc):
        """the bin table [M + 1] of a [T, C] field that gives a result per bin -> (offsets, M)"""
        offsets, M = Context._offsets(offsets)
        Context._sizes(who, T=T, C=Cc, M=M)
        return offsets, M

    @staticmethod
    def _row_groups(group, T):
        """one group id per row of a [T, C] field, as host int32"""
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.shape != (T,):
            raise ValueError(f"group: expected one group id per row ({T}), got shape {group.shape}")
        return group

    @staticmethod
    def _groups(who, group, G, T, Cc):
        """the group ids [T] and G of a [T, C] field that gives a result per group -> (group, G)"""
        group = Context._row_groups(group, T)
        Context._sizes(who, T=T, C=Cc)
        Context._sizes(who, G=int(G))
        return group, int(G)

    @contextlib.contextmanager
    def _uploads(self):
        """``up(a)``: ``a`` on the device -- a DeviceArray (or None) as it is, a host array uploaded as it is for the length of the
        ``with`` block and freed when it ends"""
        mine = []

        def up(a):
            if a is None or isinstance(a, DeviceArray):
                return a
            mine.append(self.to_device(a, a.dtype))
            return mine[-1]

        try:
            yield up
        finally:
            for a in mine:
                a.free()

    @contextlib.contextmanager
    def _fresh(self, *kinds):
        """fresh DeviceArrays, one per (shape, dtype), for the results of the call made in the ``with`` block: freed if it raises, the
        caller's otherwise"""
        made = [self.empty(shape, dtype) for shape, dtype in kinds]
        try:
            yield made
        except BaseException:
            for a in made:
                a.free()
            raise

    def _stat_planes(self, out, nstat, M, Cc, plane_rows):
        """the output of a call that gives nstat statistics of M bins -> (out, elements between two statistics): the [nstat * M, C]
        result, or with ``plane_rows`` the [M, C] view of this call's bins inside the first of nstat planes of a longer DeviceArray"""
        if plane_rows is None:
            out = self._result_buffer(out, (nstat * M, Cc), True)
            stride = M * out.ld
        else:
            out = self._result_buffer(out, (M, Cc), True)
            base = out.base
            first = None if base is None or out.ld != base.ld else (out.ptr - base.ptr) // (base.ld * 8)
            if first is None or plane_rows < M or first + (nstat - 1) * plane_rows + M > base.shape[0]:
                raise ValueError(f"out: expected the rows of {M} bins inside the first of {nstat} planes of {plane_rows} rows of a DeviceArray")
            stride = int(plane_rows) * out.ld
        return out, stride

    def _on_host(self, name, fn, shape, *args, fields="a host array"):
        """the tail of the ``_host`` twin ``name``: none of ``args`` may be resident; ``fn(ctx, *args, out)``, every host array as its
        pointer, fills a fresh host result of ``shape`` (upload, run, download in one call of the library)"""
        if any(isinstance(a, DeviceArray) for a in args):
            raise ValueError(f"{name}_host: expected {fields}")
        out = np.empty(shape)
        check(fn(self.handle, *[ptr(a) if isinstance(a, np.ndarray) else a for a in args], ptr(out)))
        return out

    def _paired(self, who, a, b, bins, out, plane_rows):
        """the resident form of the paired call ``who``.  ``bins``: what its ABI takes between C and the result -- the table of the bins
        (offsets [M + 1] or group ids [T]), their number, the codes of the statistics and, after nstat, what the family adds"""
        table, n, codes, *more = bins
        T, Cc = a.shape
        out, stride = self._stat_planes(out, len(codes), n, Cc, plane_rows)
        with self._uploads() as up:
            same = b is a
            a = up(a)
            b = a if same else up(b)
            self._same_context(who, a=a, b=b, out=out)
            check(getattr(self.lib, who + "_dev")(self.handle, a.vptr, _f32(a), a.ld, b.vptr, _f32(b), b.ld, T, Cc, ptr(table), n, ptr(codes),
                                                  len(codes), *more, out.vptr, out.ld, stride))
        return out

    def _paired_host(self, who, a, b, bins):
        """the host form of the paired call ``who``; ``bins`` as for ``_paired``"""
        table, n, codes, *more = bins
        T, Cc = a.shape
        return self._on_host(who[len("sd_"):], getattr(self.lib, who), (len(codes) * n, Cc), a, _f32(a), b, _f32(b), T, Cc, table, n, codes,
                             len(codes), *more, fields="host arrays")

    # ---- resampling of the time axis (GridArray.resample) ----
    @staticmethod
    def _resample_args(field, offsets, op):
        if op not in _lib.RESAMPLE_OPS:
            raise NotImplementedError(f"resample reduction {op!r}: only 'mean' and 'sum' are implemented")
        field = Context._time_field(field)
        return (field, *Context._offsets(offsets), _lib.RESAMPLE_OPS[op])

    def resample(self, field, offsets, op="mean", out=None):
        """field [T, C]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray (rows ``ld`` apart);
        offsets: host int64 [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1 -> [M, C] float64 DeviceArray (``out``: a [M, C]
        DeviceArray, possibly a view of a wider or longer one).  op 'mean' | 'sum', NaN samples skipped (sd_resample_dev)."""
        field, offsets, M, code = self._resample_args(field, offsets, op)
        T, Cc = field.shape
        self._sizes("sd_resample", T=T, C=Cc, M=M)
        out = self._result_buffer(out, (M, Cc), True)
        with self._uploads() as up:
            field = up(field)
            self._same_context("sd_resample", field=field, out=out)
            check(self.lib.sd_resample_dev(self.handle, code, field.vptr, _f32(field), field.ld, T, Cc, ptr(offsets), M, out.vptr, out.ld))
        return out

    def resample_host(self, field, offsets, op="mean"):
        """host [T, C] -> host [M, C] through sd_resample (upload, run, download in one call)"""
        field, offsets, M, code = self._resample_args(field, offsets, op)
        T, Cc = field.shape
        return self._on_host("resample", self.lib.sd_resample, (M, Cc), code, field, _f32(field), T, Cc, offsets, M)

    # ---- threshold and spell indices per bin of the time axis (GridArray.where) ----
    @staticmethod
    def _spells_args(field, op, threshold, offsets, stats, min_length, group):
        """-> the field and, in the order of the ABI, what follows its sizes"""
        if op not in _lib.SPELL_OPS:
            raise ValueError(f"where op {op!r}: expected one of {', '.join(repr(k) for k in _lib.SPELL_OPS)}")
        codes = Context._stat_codes("sd_spells", stats, _lib.SPELL_STATS, "spell statistic")
        field = Context._time_field(field)
        T, Cc = field.shape
        offsets, M = Context._bins("sd_spells", offsets, T, Cc)
        table = None
        if isinstance(threshold, DeviceArray) or np.ndim(threshold) > 0:
            table = threshold if isinstance(threshold, DeviceArray) else np.ascontiguousarray(threshold, dtype=np.float64)
            if len(table.shape) != 2 or table.dtype != np.float64 or table.shape[1] != Cc or table.shape[0] < 1:
                raise ValueError(f"threshold: expected a number or a float64 [G, {Cc}] table, got shape {tuple(table.shape)} of {table.dtype}")
            threshold = 0.0
            if group is not None:
                group = Context._row_groups(group, T)
        elif group is not None:
            raise ValueError("group: a scalar threshold takes no group ids")
        G = 1 if table is None else table.shape[0]
        return field, _lib.SPELL_OPS[op], float(threshold), table, group, G, offsets, M, int(min_length), codes

    def spells(self, field, op, threshold, offsets, stats, min_length=1, group=None, out=None, plane_rows=None):
        """field [T, C]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray (rows ``ld`` apart); op
        '>' | '>=' | '<' | '<='; threshold: a number, or a [G, C] float64 table (host array or DeviceArray) whose row ``group[r]``
        (host int32 [T]; None with G == 1: a per-cell threshold) holds the thresholds of row r; offsets: host int64 [M + 1], bin m =
        rows offsets[m] .. offsets[m + 1] - 1; stats: one name or a list of 'valid' | 'count' | 'fraction' | 'longest_spell' |
        'spell_days' | 'spell_count' -> [nstat * M, C] float64 DeviceArray, row ``s * M + m`` the statistic s of bin m, all from one
        pass over the field (sd_spells_dev; the rule is in include/sd_downscale.h).  ``out``: that DeviceArray, possibly a view of a
        wider one.  With ``plane_rows`` ``out`` is instead the [M, C] view of this call's bins inside the first of nstat planes of
        ``plane_rows`` rows each of a longer DeviceArray (how a caller fills the bins block by block)."""
        field, code, thr, table, group, G, offsets, M, L, codes = self._spells_args(field, op, threshold, offsets, stats, min_length, group)
        T, Cc = field.shape
        out, stride = self._stat_planes(out, len(codes), M, Cc, plane_rows)
        with self._uploads() as up:
            field, table = up(field), up(table)
            self._same_context("sd_spells", field=field, threshold=table, out=out)
            check(self.lib.sd_spells_dev(self.handle, field.vptr, _f32(field), field.ld, T, Cc, code, thr, vptr(table),
                                         0 if table is None else table.ld, ptr(group), G, ptr(offsets), M, L, ptr(codes), len(codes), out.vptr,
                                         out.ld, stride))
        return out

    def spells_host(self, field, op, threshold, offsets, stats, min_length=1, group=None):
        """host [T, C] -> host [nstat * M, C] through sd_spells (upload, run, download in one call)"""
        field, code, thr, table, group, G, offsets, M, L, codes = self._spells_args(field, op, threshold, offsets, stats, min_length, group)
        T, Cc = field.shape
        return self._on_host("spells", self.lib.sd_spells, (len(codes) * M, Cc), field, _f32(field), T, Cc, code, thr, table, group, G, offsets, M,
                             L, codes, len(codes), fields="host arrays")

    # ---- paired skill statistics per bin of the time axis (GridArray.compare) ----
    @staticmethod
    def _skill_fields(who, a, b, stats):
        """the statistics and the two fields of a paired call -> (a, b, codes)"""
        codes = Context._stat_codes(who, stats, _lib.SKILL_STATS, "skill statistic")
        return (*Context._pair(a, b), codes)

    def skill(self, a, b, offsets, stats, out=None, plane_rows=None):
        """a, b [T, C]: float32 / float64 host arrays (any other dtype is taken as float64) or DeviceArrays (rows ``ld`` apart; they
        may be the same array), paired row by row; offsets: host int64 [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; stats:
        one name or a list of 'count' | 'bias' | 'ratio' | 'mae' | 'rmse' | 'corr' | 'std_ratio' -> [nstat * M, C] float64 DeviceArray,
        row ``s * M + m`` the statistic s of bin m; both fields are read once, or twice where 'corr' or 'std_ratio' is among them
        (sd_skill_dev; the rule is in include/sd_downscale.h).  ``out`` and ``plane_rows``: as for ``spells``."""
        a, b, codes = self._skill_fields("sd_skill", a, b, stats)
        return self._paired("sd_skill", a, b, (*self._bins("sd_skill", offsets, *a.shape), codes), out, plane_rows)

    def skill_host(self, a, b, offsets, stats):
        """host [T, C] twice -> host [nstat * M, C] through sd_skill (upload, run, download in one call)"""
        a, b, codes = self._skill_fields("sd_skill", a, b, stats)
        return self._paired_host("sd_skill", a, b, (*self._bins("sd_skill", offsets, *a.shape), codes))

    def skill_groups(self, a, b, group, G, stats, out=None, plane_rows=None):
        """``skill`` over groups of steps in place of bins: group: host int32 [T], every id in [0, G) -> [nstat * G, C] float64
        DeviceArray, row ``s * G + g`` the statistic s of group g, evaluated as ``skill`` evaluates one bin whose steps are the rows
        with ``group == g`` in ascending order: the bits of ``skill`` on the fields gathered group by group.  An id that never occurs
        gives count 0 and NaN.  Both fields are whole on the device for the call (sd_skill_groups_dev).  ``out`` and ``plane_rows``:
        as for ``spells``."""
        a, b, codes = self._skill_fields("sd_skill_groups", a, b, stats)
        return self._paired("sd_skill_groups", a, b, (*self._groups("sd_skill_groups", group, G, *a.shape), codes), out, plane_rows)

    def skill_groups_host(self, a, b, group, G, stats):
        """host [T, C] twice -> host [nstat * G, C] through sd_skill_groups (upload, run, download in one call)"""
        a, b, codes = self._skill_fields("sd_skill_groups", a, b, stats)
        return self._paired_host("sd_skill_groups", a, b, (*self._groups("sd_skill_groups", group, G, *a.shape), codes))

    # ---- distribution scores per bin of the time axis (GridArray.compare(...).ks() / .perkins()) ----
    @staticmethod
    def _twosample_fields(who, a, b, stats, width, origin):
        """the statistics, the histogram and the two fields of a two-sample call -> (a, b, (codes, width, origin))"""
        codes = Context._stat_codes(who, stats, _lib.TWOSAMPLE_STATS, "distribution statistic")
        perkins = _lib.TWOSAMPLE_STATS["perkins"] in codes
        if perkins:
            if width is None:
                raise ValueError("perkins needs the width of the histogram bins (width=...)")
            number = (int, float, np.integer, np.floating)
            if not (isinstance(width, number) and not isinstance(width, bool) and np.isfinite(width) and width > 0):
                raise ValueError(f"width: expected a positive finite number, got {width!r}")
            if not (isinstance(origin, number) and not isinstance(origin, bool) and np.isfinite(origin)):
                raise ValueError(f"origin: expected a finite number, got {origin!r}")
        return (*Context._pair(a, b), (codes, float(width) if perkins else 0.0, float(origin) if perkins else 0.0))

    def twosample(self, a, b, offsets, stats, width=None, origin=0.0, out=None, plane_rows=None):
        """a, b [T, C]: float32 / float64 host arrays (any other dtype is taken as float64) or DeviceArrays (rows ``ld`` apart; they
        may be the same array); offsets: host int64 [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; stats: one name or a list
        of 'ks' | 'perkins' | 'na' | 'nb' -> [nstat * M, C] float64 DeviceArray, row ``s * M + m`` the statistic s of bin m
        (sd_twosample_dev; the rule is in include/sd_downscale.h).  Unlike ``skill``, each field contributes its own non-NaN samples of
        a bin: a NaN in ``a`` does not remove the sample of ``b`` at that step.  ``width`` (> 0) and ``origin``: the histogram bins
        floor((x - origin) / width) of 'perkins', read only where it is asked for.  A bin holds at most 19 456 rows
        (NotImplementedError beyond).  ``out`` and ``plane_rows``: as for ``spells``."""
        a, b, scores = self._twosample_fields("sd_twosample", a, b, stats, width, origin)
        return self._paired("sd_twosample", a, b, (*self._bins("sd_twosample", offsets, *a.shape), *scores), out, plane_rows)

    def twosample_host(self, a, b, offsets, stats, width=None, origin=0.0):
        """host [T, C] twice -> host [nstat * M, C] through sd_twosample (upload, run, download in one call)"""
        a, b, scores = self._twosample_fields("sd_twosample", a, b, stats, width, origin)
        return self._paired_host("sd_twosample", a, b, (*self._bins("sd_twosample", offsets, *a.shape), *scores))

    def twosample_groups(self, a, b, group, G, stats, width=None, origin=0.0, out=None, plane_rows=None):
        """``twosample`` over groups of steps in place of bins: group: host int32 [T], every id in [0, G) -> [nstat * G, C] float64
        DeviceArray, row ``s * G + g`` the statistic s of group g, evaluated as ``twosample`` evaluates one bin whose steps are the
        rows with ``group == g``: the bits of ``twosample`` on the fields gathered group by group.  An id that never occurs gives na =
        nb = 0 and NaN.  A group holds at most 19 456 rows (NotImplementedError beyond); both fields are whole on the device for the
        call (sd_twosample_groups_dev).  ``out`` and ``plane_rows``: as for ``spells``."""
        a, b, scores = self._twosample_fields("sd_twosample_groups", a, b, stats, width, origin)
        return self._paired("sd_twosample_groups", a, b, (*self._groups("sd_twosample_groups", group, G, *a.shape), *scores), out, plane_rows)

    def twosample_groups_host(self, a, b, group, G, stats, width=None, origin=0.0):
        """host [T, C] twice -> host [nstat * G, C] through sd_twosample_groups (upload, run, download in one call)"""
        a, b, scores = self._twosample_fields("sd_twosample_groups", a, b, stats, width, origin)
        return self._paired_host("sd_twosample_groups", a, b, (*self._groups("sd_twosample_groups", group, G, *a.shape), *scores))

    # ---- temporal disaggregation (GridArray.disaggregate) ----
    @staticmethod
    def _disagg_args(target, obs, src_row, offsets, op, climo, group):
        if op not in _lib.DISAGG_OPS:
            raise NotImplementedError(f"disaggregation op {op!r}: only 'shift', 'scale_mean' and 'scale_sum' are implemented")
        obs = Context._time_field(obs, "obs", "To")
        fields = {"target": target, "climo": climo}
        for name, a in fields.items():
            if a is None:
                continue
            if not isinstance(a, DeviceArray):
                a = fields[name] = np.ascontiguousarray(a, dtype=np.float64)
            if len(a.shape) != 2 or a.dtype != np.float64 or a.shape[1] != obs.shape[1]:
                raise ValueError(f"{name}: expected a float64 [{'M' if name == 'target' else 'G'}, {obs.shape[1]}] field, got shape "
                                 f"{tuple(a.shape)} of {a.dtype}")
        target, climo = fields["target"], fields["climo"]
        src_row = np.ascontiguousarray(src_row, dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if src_row.ndim != 1:
            raise ValueError(f"src_row: expected a table of Tout entries, got shape {src_row.shape}")
        M = target.shape[0]
        if offsets.ndim != 1 or len(offsets) != M + 1:
            raise ValueError(f"offsets: expected a table of M + 1 = {M + 1} entries, got shape {offsets.shape}")
        if (climo is None) != (group is None):
            raise ValueError(f"sd_downscale: sd_disagg: {'group without climo' if climo is None else 'climo without group'}")
        if group is not None:
            group = np.ascontiguousarray(group, dtype=np.int32)
            if group.shape != (M,):
                raise ValueError(f"group: expected one climatology row per bin ({M}), got shape {group.shape}")
        return target, obs, src_row, offsets, _lib.DISAGG_OPS[op], climo, 0 if climo is None else climo.shape[0], group

    def disaggregate(self, target, obs, src_row, offsets, op="shift", climo=None, group=None, out=None):
        """target [M, C] float64 and obs [To, C] float32 / float64: host arrays or DeviceArrays (rows ``ld`` apart); src_row: host int64
        [Tout], the row of obs every output row borrows; offsets: host int64 [M + 1], bin m = output rows offsets[m] .. offsets[m + 1]
        - 1; climo [G, C] float64 with group: host int32 [M] when the target is an anomaly -> [Tout, C] float64 DeviceArray (``out``:
        a [Tout, C] DeviceArray, possibly a view of a wider or longer one).  op 'shift' | 'scale_mean' | 'scale_sum' (sd_disagg_dev)."""
        target, obs, src_row, offsets, code, climo, G, group = self._disagg_args(target, obs, src_row, offsets, op, climo, group)
        To, Cc = obs.shape
        M, Tout = target.shape[0], len(src_row)
        self._sizes("sd_disagg", To=To, C=Cc, Tout=Tout, M=M)
        out = self._result_buffer(out, (Tout, Cc), True)
        with self._uploads() as up:
            target, obs, climo = up(target), up(obs), up(climo)
            self._same_context("sd_disagg", target=target, obs=obs, climo=climo, out=out)
            check(self.lib.sd_disagg_dev(self.handle, code, target.vptr, target.ld, obs.vptr, _f32(obs), obs.ld, To, Cc, ptr(src_row), Tout,
                                         ptr(offsets), M, vptr(climo), 0 if climo is None else climo.ld, G, ptr(group), out.vptr, out.ld))
        return out

    def disaggregate_host(self, target, obs, src_row, offsets, op="shift", climo=None, group=None):
        """host target [M, C], obs [To, C] -> host [Tout, C] through sd_disagg (upload, run, download in one call)"""
        target, obs, src_row, offsets, code, climo, G, group = self._disagg_args(target, obs, src_row, offsets, op, climo, group)
        To, Cc = obs.shape
        M, Tout = target.shape[0], len(src_row)
        return self._on_host("disaggregate", self.lib.sd_disagg, (Tout, Cc), code, target, obs, _f32(obs), To, Cc, src_row, Tout, offsets, M, climo,
                             G, group, fields="host arrays")

    # ---- grouping of the time axis (GridArray.groupby) ----
    @staticmethod
    def _groupby_args(who, field, group, G, op, ops):
        if op not in ops:
            raise NotImplementedError(f"{who} op {op!r}: only {', '.join(repr(k) for k in ops)} are implemented")
        field = Context._time_field(field)
        return (field, *Context._groups("sd_" + who, group, G, *field.shape), ops[op])

    def groupby_reduce(self, field, group, G, op="mean", acc=None, out=None, finish=True):
        """field [T, C]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray (rows ``ld`` apart); group:
        host int32 [T], every id in [0, G).  The rows are added, in row order, onto row ``group[t]`` of the accumulators ``acc`` = (sum
        [G, C] float64, count [G, C] int32, two DeviceArrays of one ``ld``): the pair an earlier call returned, which this call
        continues, or None for new ones that start from zero.  -> ``(result, acc)``: with ``finish`` the [G, C] float64 DeviceArray
        of op 'mean' | 'sum' over everything added so far (``out``: a [G, C] DeviceArray, possibly a view of a wider or longer one),
        else None; NaN samples skipped (sd_groupby_reduce_dev).  Any cut of the rows into calls gives the bits of one call."""
        field, group, G, code = self._groupby_args("groupby_reduce", field, group, G, op, _lib.GROUPBY_REDUCE_OPS)
        T, Cc = field.shape
        carry = acc is not None
        if carry:
            s, n = acc
            if (tuple(s.shape), s.dtype, tuple(n.shape), n.dtype) != ((G, Cc), np.float64, (G, Cc), np.int32) or s.ld != n.ld:
                raise ValueError(f"acc: expected the (sum float64, count int32) pair of [{G}, {Cc}] DeviceArrays of an earlier call")
        else:
            s, n = self.empty((G, Cc)), self.empty((G, Cc), np.int32)
        out = self._result_buffer(out, (G, Cc), True) if finish else None
        with self._uploads() as up:
            field = up(field)
            self._same_context("sd_groupby_reduce", field=field, sum=s, count=n, out=out)
            check(self.lib.sd_groupby_reduce_dev(self.handle, code, field.vptr, _f32(field), field.ld, T, Cc, ptr(group), G, s.vptr, n.vptr, s.ld,
                                                 int(carry), vptr(out), 0 if out is None else out.ld))
        return out, (s, n)

    def groupby_reduce_host(self, field, group, G, op="mean"):
        """host [T, C] -> host [G, C] through sd_groupby_reduce (upload, run, download in one call)"""
        field, group, G, code = self._groupby_args("groupby_reduce", field, group, G, op, _lib.GROUPBY_REDUCE_OPS)
        T, Cc = field.shape
        return self._on_host("groupby_reduce", self.lib.sd_groupby_reduce, (G, Cc), code, field, _f32(field), T, Cc, group, G)

    def groupby_apply(self, field, group, table, op, out=None):
        """field [T, C] as for ``groupby_reduce``; table [G, C] float64: a host array or DeviceArray; group: host int32 [T] in [0, G)
        -> [T, C] float64 DeviceArray ``field (op) table[group]``, op 'sub' | 'add' | 'mul' | 'div', one IEEE operation per element
        (``out``: a [T, C] DeviceArray, possibly a view of a wider or longer one) (sd_groupby_apply_dev)."""
        if not isinstance(table, DeviceArray):
            table = np.ascontiguousarray(table, dtype=np.float64)
        if len(table.shape) != 2 or table.dtype != np.float64:
            raise ValueError(f"table: expected a float64 [G, C] field, got shape {tuple(table.shape)} of {table.dtype}")
        field, group, G, code = self._groupby_args("groupby_apply", field, group, table.shape[0], op, _lib.GROUPBY_APPLY_OPS)
        if table.shape[1] != field.shape[1]:
            raise ValueError(f"table: expected a float64 [G, {field.shape[1]}] field, got shape {tuple(table.shape)}")
        T, Cc = field.shape
        out = self._result_buffer(out, (T, Cc), True)
        with self._uploads() as up:
            field, table = up(field), up(table)
            self._same_context("sd_groupby_apply", field=field, table=table, out=out)
            check(self.lib.sd_groupby_apply_dev(self.handle, code, field.vptr, _f32(field), field.ld, T, Cc, ptr(group), G, table.vptr, table.ld,
                                                out.vptr, out.ld))
        return out

    def groupby_apply_host(self, field, group, table, op):
        """host field [T, C], table [G, C] -> host [T, C] through sd_groupby_apply (upload, run, download in one call)"""
        table = np.ascontiguousarray(table, dtype=np.float64)
        field, group, G, code = self._groupby_args("groupby_apply", field, group, table.shape[0], op, _lib.GROUPBY_APPLY_OPS)
        if isinstance(field, DeviceArray) or table.ndim != 2 or table.shape[1] != field.shape[1]:
            raise ValueError("groupby_apply_host: expected a host [T, C] field and a host [G, C] table")
        T, Cc = field.shape
        return self._on_host("groupby_apply", self.lib.sd_groupby_apply, (T, Cc), code, field, _f32(field), T, Cc, group, G, table)

    # ---- order statistics over the time axis (GridArray.quantile / .median) ----
    @staticmethod
    def _quantile_args(field, q, group, G, method):
        if method not in _lib.QUANTILE_METHODS:
            raise ValueError(f"quantile method {method!r}: expected one of {', '.join(repr(k) for k in _lib.QUANTILE_METHODS)}")
        field = Context._time_field(field)
        T, Cc = field.shape
        Context._sizes("sd_quantile", T=T, C=Cc)
        if group is None:
            G = 1
        else:
            group = Context._row_groups(group, T)
            G = int(group.max()) + 1 if G is None else int(G)
        q = np.ascontiguousarray([0.5] if method == "median" else np.atleast_1d(q), dtype=np.float64)
        if q.ndim != 1 or G < 1 or len(q) < 1:
            raise ValueError(f"sd_downscale: sd_quantile: bad sizes (G={G}, Q={q.size if q.ndim == 1 else q.shape})")
        return field, q, group, G, _lib.QUANTILE_METHODS[method]

    def quantile(self, field, q, group=None, G=None, method="linear", skipna=True, out=None):
        """field [T, C]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray (rows ``ld`` apart); q: one
        quantile or [Q] of them in [0, 1]; group: host int32 [T] with every id in [0, G) (``G`` defaults to the largest id + 1), or None
        for one group -> [Q * G, C] float64 DeviceArray whose row ``q * G + g`` is np.nanquantile(method=...) of group g per cell
        (``skipna=False``: np.quantile, NaN where the group holds one); method 'linear' | 'lower' | 'higher' | 'nearest' | 'midpoint',
        or 'median' (np.nanmedian; q is not read, Q = 1).  ``out``: a [Q * G, C] DeviceArray, possibly a view of a wider or longer
        one.  Groups of more than 19 456 rows are refused (sd_quantile_dev)."""
        field, q, group, G, code = self._quantile_args(field, q, group, G, method)
        T, Cc = field.shape
        out = self._result_buffer(out, (len(q) * G, Cc), True)
        with self._uploads() as up:
            field = up(field)
            self._same_context("sd_quantile", field=field, out=out)
            check(self.lib.sd_quantile_dev(self.handle, code, int(bool(skipna)), field.vptr, _f32(field), field.ld, T, Cc, ptr(group), G, ptr(q),
                                           len(q), out.vptr, out.ld))
        return out

    def quantile_host(self, field, q, group=None, G=None, method="linear", skipna=True):
        """host [T, C] -> host [Q * G, C] through sd_quantile (upload, run, download in one call)"""
        field, q, group, G, code = self._quantile_args(field, q, group, G, method)
        T, Cc = field.shape
        return self._on_host("quantile", self.lib.sd_quantile, (len(q) * G, Cc), code, int(bool(skipna)), field, _f32(field), T, Cc, group, G, q,
                             len(q))

    # ---- rolling windows over the time axis (GridArray.rolling) ----
    @staticmethod
    def _rolling_args(field, window, op, back, min_periods, ddof):
        if op not in _lib.ROLLING_OPS:
            raise NotImplementedError(f"rolling op {op!r}: only {', '.join(repr(k) for k in _lib.ROLLING_OPS)} are implemented")
        field = Context._time_field(field)
        T, Cc = field.shape
        Context._sizes("sd_rolling", T=T, C=Cc)
        window = int(window)
        back = window - 1 if back is None else int(back)
        min_periods = window if min_periods is None else int(min_periods)
        return field, window, back, min_periods, int(ddof), _lib.ROLLING_OPS[op]

    def rolling(self, field, window, op="mean", back=None, min_periods=None, ddof=1, wrap=False, t0=0, n_out=None, out=None):
        """field [T, C]: a float32 / float64 host array (any other dtype is taken as float64) or DeviceArray (rows ``ld`` apart) ->
        [n_out, C] float64 DeviceArray: the rows ``t0 .. t0 + n_out - 1`` (default: all) of the rolling statistic op 'mean' | 'sum' |
        'var' | 'std' (``ddof`` for the last two).  The window of row t is the rows ``t - back .. t - back + window - 1`` (``back``
        defaults to ``window - 1``, pandas' trailing window; ``window // 2`` is ``center=True``), clipped to the field or, with
        ``wrap``, taken modulo T; NaN samples are skipped, fewer than ``min_periods`` (default ``window``) give NaN.  ``out``: a
        [n_out, C] DeviceArray, possibly a view of a wider or longer one.  O(window) work per output (sd_rolling_dev)."""
        field, window, back, min_periods, ddof, code = self._rolling_args(field, window, op, back, min_periods, ddof)
        T, Cc = field.shape
        t0 = int(t0)
        n_out = T - t0 if n_out is None else int(n_out)
        if n_out < 1:
            raise ValueError(f"sd_downscale: sd_rolling: the output rows {t0} .. {t0 + n_out - 1} lie outside the {T} rows of the source")
        out = self._result_buffer(out, (n_out, Cc), True)
        with self._uploads() as up:
            field = up(field)
            self._same_context("sd_rolling", field=field, out=out)
            check(self.lib.sd_rolling_dev(self.handle, code, field.vptr, _f32(field), field.ld, T, Cc, window, back, min_periods, ddof,
                                          int(bool(wrap)), t0, n_out, out.vptr, out.ld))
        return out

    def rolling_host(self, field, window, op="mean", back=None, min_periods=None, ddof=1, wrap=False):
        """host [T, C] -> host [T, C] through sd_rolling (upload, run, download in one call)"""
        field, window, back, min_periods, ddof, code = self._rolling_args(field, window, op, back, min_periods, ddof)
        T, Cc = field.shape
        return self._on_host("rolling", self.lib.sd_rolling, (T, Cc), code, field, _f32(field), T, Cc, window, back, min_periods, ddof,
                             int(bool(wrap)))

    # ---- constructed analogs (ConstructedAnalogs) ----
    @staticmethod
    def _ca_coarse(who, L, Q, wc, k):
        """the coarse side of a constructed-analog call: L [Tl, Cc] and Q [Tq, Cc] float64, wc [Cc] on the host, k"""
        L, Q = Context._field("L", L, "Tl", "Cc"), Context._field("Q", Q, "Tq", "Cc")
        if Q.shape[1] != L.shape[1]:
            raise ValueError(f"Q: expected a [Tq, {L.shape[1]}] field like L, got shape {tuple(Q.shape)}")
        Context._sizes(who, Tl=L.shape[0], Tq=Q.shape[0], Cc=L.shape[1])
        wc = _lib.as_f64(wc)
        if wc.shape != (L.shape[1],):
            raise ValueError(f"wc: expected {L.shape[1]} column weights, got shape {wc.shape}")
        k = int(k)
        if not 1 <= k <= _lib.CA_MAX_ANALOGS:
            raise ValueError(f"sd_downscale: {who}: k = {k} lies outside [1, {_lib.CA_MAX_ANALOGS}]")
        return L, Q, wc, k

    @staticmethod
    def _ca_ids(name, ids, n):
        """one int32 per day (keys, exclusion ids); None: -1 for every day"""
        ids = np.full(n, -1, dtype=np.int32) if ids is None else _lib.as_i32(ids)
        if ids.shape != (n,):
            raise ValueError(f"{name}: expected one id per day ({n}), got shape {ids.shape}")
        return ids

    @staticmethod
    def _ca_idx(idx):
        """the analogs of ``ca_select`` as far as Tq and k can be read from them -> (Tq, k); ``_ca_table`` checks the rest"""
        if not isinstance(idx, DeviceArray) or len(idx.shape) != 2:
            raise ValueError("idx: expected the int32 [Tq, k] DeviceArray of ca_select")
        return idx.shape

    @staticmethod
    def _ca_table(name, a, Tq, k, dtype):
        if not isinstance(a, DeviceArray) or tuple(a.shape) != (Tq, k) or a.dtype != dtype or a.ld != k:
            raise ValueError(f"{name}: expected a contiguous {np.dtype(dtype).name} DeviceArray of shape ({Tq}, {k})")
        return a

    @staticmethod
    def _ca_fine(F):
        """the fine library -> (Tl, Cf)"""
        if not isinstance(F, DeviceArray) or len(F.shape) != 2 or F.dtype not in (np.float32, np.float64):
            raise ValueError("F: expected a float32 or float64 [Tl, Cf] DeviceArray")
        return F.shape

    @staticmethod
    def _ca_rows(who, q0, q1, Tq):
        """the targets [q0, q1) of an applying call (q1 None: to the last)"""
        q0, q1 = int(q0), Tq if q1 is None else int(q1)
        if not 0 <= q0 < q1 <= Tq:
            raise ValueError(f"sd_downscale: {who}: rows [{q0}, {q1}) lie outside the {Tq} targets")
        return q0, q1

    def ca_select(self, L, Q, wc, k, key_l=None, key_q=None, period=1, window=-1, excl_l=None, excl_q=None):
        """L [Tl, Cc], Q [Tq, Cc]: float64 host arrays or DeviceArrays (rows ``ld`` apart); wc [Cc] host column weights; key_*, excl_*:
        host int32 per day (None: key 0 / no exclusion) -> (idx int32 [Tq, k], dist float64 [Tq, k], status int32 [Tq]) DeviceArrays:
        the k candidates of each target smallest by (distance, day) (sd_ca_select_dev; the rule is in include/sd_downscale.h).
        ``window`` < 0: every day is inside the window."""
        L, Q, wc, k = self._ca_coarse("sd_ca_select", L, Q, wc, k)
        Tl, Tq = L.shape[0], Q.shape[0]
        key_l = np.zeros(Tl, np.int32) if key_l is None else self._ca_ids("key_l", key_l, Tl)
        key_q = np.zeros(Tq, np.int32) if key_q is None else self._ca_ids("key_q", key_q, Tq)
        excl_l, excl_q = self._ca_ids("excl_l", excl_l, Tl), self._ca_ids("excl_q", excl_q, Tq)
        with self._uploads() as up:
            L, Q = up(L), up(Q)
            self._same_context("sd_ca_select", L=L, Q=Q)
            with self._fresh(((Tq, k), np.int32), ((Tq, k), np.float64), ((Tq,), np.int32)) as (idx, dist, status):
                check(self.lib.sd_ca_select_dev(self.handle, L.vptr, L.ld, Tl, Q.vptr, Q.ld, Tq, L.shape[1], ptr(wc), k, ptr(key_l), ptr(key_q),
                                                int(period), int(window), ptr(excl_l), ptr(excl_q), idx.vptr, dist.vptr, status.vptr))
        return idx, dist, status

    def ca_weights(self, L, Q, wc, idx, dist, status, kind="regression", ridge=1e-6):
        """the weights of the analogs ``idx`` of ``ca_select`` -> float64 [Tq, k] DeviceArray; ``status`` is updated, and ``idx`` /
        ``dist`` of a target with a singular Gram matrix are cleared.  kind 'regression' (ridge-regularised least squares of the target
        pattern on the k library patterns) | 'mean' (1 / k) (sd_ca_weights_dev)."""
        if kind not in _lib.CA_KINDS:
            raise ValueError(f"kind={kind!r}: expected one of {', '.join(repr(s) for s in _lib.CA_KINDS)}")
        L, Q, wc, k = self._ca_coarse("sd_ca_weights", L, Q, wc, self._ca_idx(idx)[1])
        Tl, Tq = L.shape[0], Q.shape[0]
        idx, dist = self._ca_table("idx", idx, Tq, k, np.int32), self._ca_table("dist", dist, Tq, k, np.float64)
        if not isinstance(status, DeviceArray) or tuple(status.shape) != (Tq,) or status.dtype != np.int32:
            raise ValueError(f"status: expected an int32 DeviceArray of shape ({Tq},)")
        ridge = float(ridge)
        if not (ridge >= 0.0 and np.isfinite(ridge)):
            raise ValueError(f"sd_downscale: sd_ca_weights: ridge = {ridge:g}, expected a finite factor >= 0")
        with self._uploads() as up:
            L, Q = up(L), up(Q)
            self._same_context("sd_ca_weights", L=L, Q=Q, idx=idx, dist=dist, status=status)
            with self._fresh(((Tq, k), np.float64)) as (weights,):
                check(self.lib.sd_ca_weights_dev(self.handle, L.vptr, L.ld, Tl, Q.vptr, Q.ld, Tq, L.shape[1], ptr(wc), k, _lib.CA_KINDS[kind], ridge,
                                                 idx.vptr, dist.vptr, weights.vptr, status.vptr))
        return weights

    def ca_apply(self, F, idx, weights, q0=0, q1=None, out=None):
        """F [Tl, Cf]: the fine library, a float32 / float64 DeviceArray (rows ``ld`` apart); idx, weights: the [Tq, k] tables ->
        float64 [q1 - q0, Cf] DeviceArray: rows [q0, q1) of ``out[q] = sum_i weights[q, i] * F[idx[q, i]]`` in analog order
        (sd_ca_apply_dev).  ``out``: that DeviceArray, possibly a view of a wider or longer one."""
        Tl, Cf = self._ca_fine(F)
        Tq, k = self._ca_idx(idx)
        idx, weights = self._ca_table("idx", idx, Tq, k, np.int32), self._ca_table("weights", weights, Tq, k, np.float64)
        q0, q1 = self._ca_rows("sd_ca_apply", q0, q1, Tq)
        out = self._result_buffer(out, (q1 - q0, Cf), True)
        self._same_context("sd_ca_apply", F=F, idx=idx, weights=weights, out=out)
        check(self.lib.sd_ca_apply_dev(self.handle, F.vptr, _f32(F), F.ld, Tl, Cf, idx.vptr, weights.vptr, Tq, k, q0, q1, out.vptr, out.ld))
        return out

    # ---- localized analogs (LocalizedAnalogs) ----
    def ca_local(self, L, Q, wc, grid, radius, idx):
        """L [Tl, ny * nx], Q [Tq, ny * nx], wc: as for ``ca_select``; grid (ny, nx) of the coarse cells, radius (ry, rx) in coarse
        cells; idx: the int32 [Tq, k] DeviceArray of ``ca_select`` -> (local_idx int32 [Tq, ny * nx], local_dist float64
        [Tq, ny * nx]) DeviceArrays: per coarse cell the analog whose distance over the cell's neighbourhood is smallest, ties to the
        lower slot (sd_ca_local_dev; the rule is in include/sd_downscale.h)."""
        L, Q, wc, k = self._ca_coarse("sd_ca_local", L, Q, wc, self._ca_idx(idx)[1])
        Tl, Tq, Cc = L.shape[0], Q.shape[0], L.shape[1]
        try:
            (ny, nx), (ry, rx) = (int(n) for n in grid), (int(r) for r in radius)
        except (TypeError, ValueError):
            raise ValueError(f"grid={grid!r}, radius={radius!r}: expected (ny, nx) and (ry, rx)") from None
        if ny < 1 or nx < 1 or ny * nx != Cc:
            raise ValueError(f"grid: expected (ny, nx) with ny * nx = {Cc} columns, got ({ny}, {nx})")
        if ry < 0 or rx < 0:
            raise ValueError(f"sd_downscale: sd_ca_local: radii ({ry}, {rx}), expected two numbers of coarse cells >= 0")
        idx = self._ca_table("idx", idx, Tq, k, np.int32)
        with self._uploads() as up:
            L, Q = up(L), up(Q)
            self._same_context("sd_ca_local", L=L, Q=Q, idx=idx)
            with self._fresh(((Tq, Cc), np.int32), ((Tq, Cc), np.float64)) as (local_idx, local_dist):
                check(self.lib.sd_ca_local_dev(self.handle, L.vptr, L.ld, Tl, Q.vptr, Q.ld, Tq, ny, nx, ptr(wc), k, ry, rx, idx.vptr,
                                               local_idx.vptr, local_dist.vptr))
        return local_idx, local_dist

    def ca_local_apply(self, F, cell_of, local_idx, L=None, Q=None, adjust="none", max_scale=0.0, q0=0, q1=None, out=None):
        """F [Tl, Cf]: the fine library, a float32 / float64 DeviceArray (rows ``ld`` apart); cell_of: int32 [Cf] DeviceArray, the
        coarse column of every fine cell; local_idx: the int32 [Tq, Cc] table of ``ca_local``; L [Tl, Cc], Q [Tq, Cc]: float64
        DeviceArrays, needed unless adjust is 'none' -> float64 [q1 - q0, Cf] DeviceArray: rows [q0, q1) of
        ``out[q, f] = F[local_idx[q, cell_of[f]], f]``, shifted by Q - L or scaled by Q / L (at most ``max_scale``; 0: no limit) of
        that day and coarse cell (sd_ca_local_apply_dev).  ``out``: that DeviceArray, possibly a view of a wider or longer one."""
        Tl, Cf = self._ca_fine(F)
        if not isinstance(cell_of, DeviceArray) or tuple(cell_of.shape) != (Cf,) or cell_of.dtype != np.int32:
            raise ValueError(f"cell_of: expected an int32 DeviceArray of shape ({Cf},)")
        if not isinstance(local_idx, DeviceArray) or len(local_idx.shape) != 2:
            raise ValueError("local_idx: expected the int32 [Tq, Cc] DeviceArray of ca_local")
        Tq, Cc = local_idx.shape
        local_idx = self._ca_table("local_idx", local_idx, Tq, Cc, np.int32)
        if adjust not in _lib.CA_ADJUST:
            raise ValueError(f"adjust={adjust!r}: expected one of {', '.join(repr(s) for s in _lib.CA_ADJUST)}")
        max_scale = float(max_scale)
        if not max_scale >= 0.0:
            raise ValueError(f"sd_downscale: sd_ca_local_apply: max_scale = {max_scale:g}, expected 0 (no limit) or a limit > 0")
        if adjust == "none":
            L = Q = None  # (not read)
        else:
            for name, a, rows, what in (("L", L, Tl, "Tl"), ("Q", Q, Tq, "Tq")):
                if not isinstance(a, DeviceArray) or tuple(a.shape) != (rows, Cc) or a.dtype != np.float64:
                    raise ValueError(f"{name}: adjust={adjust!r} needs a float64 DeviceArray of shape ({rows}, {Cc}) [{what}, Cc]")
        q0, q1 = self._ca_rows("sd_ca_local_apply", q0, q1, Tq)
        out = self._result_buffer(out, (q1 - q0, Cf), True)
        self._same_context("sd_ca_local_apply", F=F, cell_of=cell_of, local_idx=local_idx, L=L, Q=Q, out=out)
        check(self.lib.sd_ca_local_apply_dev(self.handle, F.vptr, _f32(F), F.ld, Tl, Cf, cell_of.vptr, local_idx.vptr, Cc, vptr(L),
                                             0 if L is None else L.ld, vptr(Q), 0 if Q is None else Q.ld, _lib.CA_ADJUST[adjust], max_scale, Tq, q0,
                                             q1, out.vptr, out.ld))
        return out


_default_ctx = None


def default_context():
    """Process-wide context on ``$SD_DEVICE`` / ``$LOCAL_RANK`` / device 0."""
    global _default_ctx
    if _default_ctx is None or _default_ctx.handle is None:
        dev = int(os.environ.get("SD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)
    return _default_ctx
