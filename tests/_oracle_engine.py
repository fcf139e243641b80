"""A stand-in for ``engine.Context`` that computes on the host with the NumPy oracles of this directory: what the lazy ``GridArray``
classes ask of a context, without the library.  It also keeps the books the host tests read:

* ``live``: the device buffers that exist -- ``empty``, ``to_device`` and every result an engine call allocates add one, ``free``
  of a buffer (not of a view) removes one;
* ``uploads``: ``(rows, dtype)`` of every host array that went up, through ``copy_from_host``, ``to_device`` or a state's ``apply``;
* ``trace``: every upload as ``("upload", rows, dtype)``, every regridding of source rows as ``("regrid", r0, r1)`` and every other
  engine call as ``(name, rows of its field, ...)`` with the rows of the buffer its result went to (0-based in a new one);
* ``fail_at``: the engine call (counted from 1, uploads not counted) that raises ``EngineFailure`` before it does anything.
"""
import numpy as np
import pytest

import _disagg_oracle as do
import _groupby_oracle as go
import _quantile_oracle as qo
import _regrid_oracle as ro
import _remap_oracle as mo
import _resample_oracle as so
import _rolling_oracle as rol
import _spells_oracle as sp


class EngineFailure(RuntimeError):
    pass


class FakeArray:
    """a DeviceArray stand-in over a NumPy buffer"""

    def __init__(self, a, ctx, base=None, row0=0):
        self.a, self.ctx, self.base, self.row0 = a, ctx, base, row0  # (row0: the first row inside ``base``)
        self._live = base is None
        ctx.live += self._live

    shape = property(lambda self: self.a.shape)
    dtype = property(lambda self: self.a.dtype)
    ld = property(lambda self: self.a.strides[0] // self.a.itemsize)

    def rows(self, r0, r1):
        assert 0 <= r0 < r1 <= self.a.shape[0]
        return FakeArray(self.a[r0:r1], self.ctx, self.base or self, self.row0 + r0)

    def copy_from_host(self, x):
        assert x.shape == self.a.shape
        self.ctx.uploaded(x)
        self.a[...] = x
        return self

    def to_host(self):
        return self.a.copy()

    def free(self):
        self.ctx.live -= self._live
        self._live = False

    def span(self):
        return self.row0, self.row0 + self.a.shape[0]


def _first_row(v):
    """the row of the array that owns ``v``'s memory at which the view ``v`` starts"""
    owner = v if v.base is None else v.base
    return (v.__array_interface__["data"][0] - owner.__array_interface__["data"][0]) // v.strides[0]


class OracleState:
    """what Context.regrid_create returns, computed by the oracle on the host"""

    created = 0

    def __init__(self, ctx, sy, sx, dy, dx, method):
        self.ctx, self.args = ctx, (np.array(sy), np.array(sx), np.array(dy), np.array(dx), method)
        OracleState.created += 1

    def apply(self, src, out=None):
        assert src.ndim == 3 and src.dtype in (np.float32, np.float64) and src.flags.c_contiguous
        r0 = _first_row(src)
        self.ctx.called("regrid", r0, r0 + src.shape[0])
        sy, sx, dy, dx, method = self.args
        fine = ro.regrid(src, sy, sx, dy, dx, method).reshape(src.shape[0], -1)
        return self.ctx.filled(out, fine)

    def close(self):
        pass


class OracleRemapState:
    def __init__(self, ctx, bounds):
        self.ctx, self.bounds = ctx, [np.array(b) for b in bounds]
        ctx.created += 1

    def apply(self, field, min_valid=0.5, out=None):
        if isinstance(field, FakeArray):
            v = field.a
        else:
            assert field.dtype in (np.float32, np.float64) and field.flags.c_contiguous
            self.ctx.uploaded(field)
            v = field
        self.ctx.called("remap", v.shape[0], *((0, v.shape[0]) if out is None else out.span()))
        ny, nx = len(self.bounds[0]) - 1, len(self.bounds[1]) - 1
        coarse = mo.remap(v.reshape(v.shape[0], ny, nx), *self.bounds, min_valid).reshape(v.shape[0], -1)
        return self.ctx.filled(out, coarse)

    def close(self):
        pass


class OracleContext:
    """what the lazy arrays ask of a Context, computed by the oracles on the host"""

    def __init__(self):
        self.created, self.uploads, self.trace, self.live, self.calls, self.fail_at = 0, [], [], 0, 0, None

    # ---- the books ----
    def uploaded(self, x):
        self.uploads.append((x.shape[0], x.dtype))
        self.trace.append(("upload", x.shape[0], x.dtype))

    def called(self, *entry):
        self.calls += 1
        if self.calls == self.fail_at:
            raise EngineFailure(f"engine call {self.calls}: {entry}")
        self.trace.append(entry)

    def filled(self, out, values):
        out = self._result_buffer(out, values.shape, True)
        out.a[...] = values
        return out

    # ---- memory ----
    def empty(self, shape, dtype=np.float64):
        return FakeArray(np.full(shape, -777, dtype=dtype), self)

    def to_device(self, a, dtype=np.float64):
        a = np.array(a, dtype=dtype)
        self.uploaded(a)
        return FakeArray(a, self)

    def _result_buffer(self, out, shape, on_device):
        assert out is None or tuple(out.shape) == tuple(shape)
        return self.empty(shape) if out is None else out

    # ---- the engine ----
    def regrid_create(self, sy, sx, dy, dx, method="linear"):
        return OracleState(self, sy, sx, dy, dx, method)

    def remap_create(self, syb, sxb, dyb, dxb):
        return OracleRemapState(self, (syb, sxb, dyb, dxb))

    def resample(self, field, offsets, op="mean", out=None):
        self.called("resample", field.shape[0], *((0, len(offsets) - 1) if out is None else out.span()))
        return self.filled(out, so.resample(field.a, offsets, op))

    def groupby_reduce(self, field, group, G, op="mean", acc=None, out=None, finish=True):
        self.called("groupby_reduce", field.shape[0], bool(finish))
        s, n = go.accumulate(field.a, group, G, None if acc is None else (acc[0].a, acc[1].a))
        if acc is None:
            acc = FakeArray(s, self), FakeArray(n, self)
        else:  # (the engine continues the pair in place)
            acc[0].a[...], acc[1].a[...] = s, n
        return (self.filled(out, go.finish((s, n), op)) if finish else None), acc

    def groupby_apply(self, field, group, table, op, out=None):
        self.called("groupby_apply", field.shape[0], *((0, field.shape[0]) if out is None else out.span()))
        return self.filled(out, go.apply(field.a, group, table.a, op))

    def rolling(self, field, window, op="mean", back=None, min_periods=None, ddof=1, wrap=False, t0=0, n_out=None, out=None):
        n_out = field.shape[0] - t0 if n_out is None else n_out
        self.called("rolling", field.shape[0], t0, *((0, n_out) if out is None else out.span()))
        return self.filled(out, rol.rolling(field.a, window, op, min_periods=min_periods, ddof=ddof, wrap=wrap, back=back)[t0:t0 + n_out])

    def quantile(self, field, q, group=None, G=None, method="linear", skipna=True, out=None):
        self.called("quantile", field.shape[0])
        return self.filled(out, qo.quantile_field(field.a, q, group, G, method, skipna))

    def spells(self, field, op, threshold, offsets, stats, min_length=1, group=None, out=None, plane_rows=None):
        M = len(offsets) - 1
        self.called("spells", field.shape[0], *((0, M) if out is None else out.span()))
        res = sp.spells(field.a, offsets, op, threshold.a if isinstance(threshold, FakeArray) else threshold, stats, min_length, group)
        if plane_rows is None:
            return self.filled(out, res)
        assert out.base is not None and out.shape[0] == M <= plane_rows and out.row0 + (len(stats) - 1) * plane_rows + M <= out.base.shape[0]
        for s in range(len(stats)):
            out.base.a[out.row0 + s * plane_rows:out.row0 + s * plane_rows + M] = res[s * M:(s + 1) * M]
        return out

    def disaggregate(self, target, obs, src_row, offsets, op="shift", climo=None, group=None, out=None):
        self.called("disaggregate", *target.span(), *((0, len(src_row)) if out is None else out.span()))
        return self.filled(out, do.disaggregate(target.a, obs.a, src_row, offsets, op, None if climo is None else climo.a, group))


@pytest.fixture
def engine(monkeypatch):
    """the package computing on an ``OracleContext``"""
    from skdownscale_amd import core, engine

    ctx = OracleContext()
    monkeypatch.setattr(engine, "default_context", lambda: ctx)
    monkeypatch.setattr(core, "default_context", lambda: ctx)
    OracleState.created = 0
    return ctx
