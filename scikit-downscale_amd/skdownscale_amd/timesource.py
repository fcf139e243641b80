"""How the source of a lazy time-axis array comes into HBM: the one place that decides it for ``resample``, ``groupby``, ``rolling``,
``quantile`` / ``median``, ``where``, ``compare``, ``remap_like`` and ``disaggregate``.

A source is one of three things.  A not yet computed lazy array of a kind the consumer accepts (``TAKEN_WHOLE``) whose
``_row_dim()`` is the walked dim gives its whole [T, C] field through its own ``device_field`` and stays uncomputed.  A lazy array
with a ``_block_producer`` (an unchunked ``coarse.interp_like(obs)``, a ``fine.remap_like(coarse)`` over a host array) is produced in
HBM, rows [r0, r1) at a time.  Anything else is a host array -- a computed lazy array is one -- whose rows are uploaded, float32 as
float32.  ``walk`` cuts the axis by the consumer's plan, fills one block of device scratch after the other and owns every buffer it
made: scratch and a lazy source's field are freed when the ``with`` block ends, the result only when it ends in an exception.
``walk_pair`` walks two sources in lock-step (``compare``): one ``walk`` each, cut at the same bins.
"""
from __future__ import annotations

import collections
import contextlib

from . import _lib
from .core import DeferredGridArray

# consumer -> the kinds (``DeferredGridArray._kind``) of lazy source it takes whole from HBM
_REDUCED = frozenset({"resample", "rolling"})
_TABLES = _REDUCED | {"group_reduced", "group_applied", "quantile"}
TAKEN_WHOLE = {
    "resample": frozenset(),
    "groupby": _REDUCED,  # the source of GroupReducedGridArray and GroupAppliedGridArray
    "rolling": _TABLES,
    "any": _TABLES | {"disagg", "remap", "constructed", "localized"},  # TimeQuantileGridArray, SpellGridArray, SkillGridArray (both sources)
    "remap": _TABLES | {"disagg"},  # dims must be (lead, *spatial)
    "table": frozenset({"group_reduced", "rolling", "quantile"}),  # GroupAppliedGridArray's other: dims must be in order
    "target": frozenset({"resample"}),  # DisaggregatedGridArray's monthly field: dims must be in order
}

# rows [r0, r1) of a [rows, cells] source of ``dtype`` into a DeviceArray: ``produce(r0, r1, out=block)``; ``uploads``: from the host
RowProducer = collections.namedtuple("RowProducer", "rows cells dtype produce uploads")


def _time_blocks(T, max_rows):
    return [(r0, min(T, r0 + max_rows)) for r0 in range(0, T, max_rows)]


def _halo_blocks(T, max_rows, halo):
    """[0, T) in consecutive runs [r0, r1) with the rows [b0, b1) = [r0 - before, r1 + after) clipped to [0, T) that a window reaching
    ``halo = (before, after)`` rows around each of its rows touches: ``(r0, r1, b0, b1)`` with at most ``max_rows`` rows in [b0, b1).
    None where ``max_rows`` has no room for one row beside its halo."""
    before, after = halo
    if max_rows >= T:
        return [(0, T, 0, T)]
    step = max_rows - before - after
    if step < 1:
        return None
    return [(r0, min(T, r0 + step), max(0, r0 - before), min(T, r0 + step + after)) for r0 in range(0, T, step)]


def _bin_blocks(offsets, max_rows):
    """the bins in consecutive runs [m0, m1) of at most ``max_rows`` samples -- at least one bin, however long, and at least one
    sample (a run of empty bins joins its neighbour)"""
    M = len(offsets) - 1
    blocks, m0 = [], 0
    for m in range(1, M + 1):
        have = offsets[m] - offsets[m0]
        if m == M or (have > 0 and offsets[m + 1] - offsets[m0] > max_rows):
            blocks.append((m0, m))
            m0 = m
    if len(blocks) > 1 and offsets[blocks[-1][1]] == offsets[blocks[-1][0]]:
        (a, _), (_, b) = blocks[-2], blocks[-1]
        blocks[-2:] = [(a, b)]
    return blocks


def host_rows(src, dim):
    """``src`` as a host [T, C] array, ``dim`` first and the other dims flattened in their order; float32 stays float32"""
    rest = tuple(d for d in src.dims if d != dim)
    v = _lib.as_field((src.transpose(dim, *rest) if src.dims[0] != dim else src).values)
    return v.reshape(v.shape[0], -1)


def upload_rows(rows):
    """the producer of a host [T, C] array"""
    return RowProducer(rows.shape[0], rows.shape[1], rows.dtype, lambda r0, r1, out: out.copy_from_host(rows[r0:r1]), True)


def producer_of(source, dim, ctx):
    """the ``RowProducer`` of a source that is not taken whole: a lazy array's own block producer, else the upload of its host rows"""
    return (source._block_producer(ctx, dim) if isinstance(source, DeferredGridArray) else None) or upload_rows(host_rows(source, dim))


def takes_whole(source, consumer, dim):
    """whether ``consumer`` takes ``source`` from HBM as [steps of ``dim``, C] through the source's own ``device_field``"""
    return (isinstance(source, DeferredGridArray) and source._kind in TAKEN_WHOLE[consumer] and not source.computed
            and source._row_dim() == dim)


class walk:
    """``with walk(source, dim, ctx, scratch_bytes, consumer, ...) as w: for i0, i1, block, b0 in w: ...``: consecutive blocks of the
    steps of ``dim`` of ``source`` (or of a ``RowProducer``) in HBM.  ``block`` is the DeviceArray of the rows b0 .. of the source (C
    = ``w.cells`` cells of the other dims in their order, the last fastest), valid until the next block.  The plan:

    * rows (the default): ``block`` holds the steps [i0, i1) = [b0, ...);
    * ``halo=(before, after)``: ``block`` holds the steps [i0, i1) and up to that many before and behind them, clipped to the array;
    * ``bins=offsets``: ``block`` holds the whole bins [i0, i1), the steps offsets[i0] .. offsets[i1] - 1;
    * ``whole=True``: one block with the whole axis, whatever ``scratch_bytes`` -- a host array goes up in one piece, a produced
      source is produced into it in pieces of ``scratch_bytes``.

    A block is at most ``scratch_bytes`` of the source's dtype (float64 for a produced source) but at least one step, or bin, with its
    halo; a lazy source the consumer takes whole is one block.  ``w.result(shape)`` allocates a float64 result.  Leaving the ``with``
    block frees the scratch or the lazy source's field, and after an exception the results as well."""

    def __init__(self, source, dim, ctx, scratch_bytes, consumer=None, halo=None, bins=None, whole=False, verb="group", row_budget=None):
        self._args = source, dim, int(scratch_bytes), consumer, halo, bins, whole, verb, row_budget
        self._ctx, self._buffer, self._results, self._producer, self._piece = ctx, None, [], None, None

    def __enter__(self):
        source, dim, scratch_bytes, consumer, halo, bins, whole, verb, row_budget = self._args
        p = None
        if isinstance(source, RowProducer):
            p = source
        elif takes_whole(source, consumer, dim):
            field = source.device_field(self._ctx)
            T, C = field.shape
            max_rows = T  # (one block)
        else:
            p = producer_of(source, dim, self._ctx)
        if p is not None:
            T, C = p.rows, p.cells
            if min(T, C) < 1:
                raise ValueError(f"nothing to {verb}: the array has sizes {source.sizes}")
            # (``row_budget``: the rows of a block as ``walk_pair`` shares them between two sources, in place of this source's own)
            max_rows = max(1, scratch_bytes // (C * p.dtype.itemsize)) if row_budget is None else max(1, int(row_budget))
            if whole:
                self._piece, max_rows = (None if p.uploads else max_rows), T
        if bins is not None:
            blocks = [(a, b, int(bins[a]), int(bins[b])) for a, b in _bin_blocks(bins, max_rows)]
        elif halo is not None:
            blocks = _halo_blocks(T, max_rows, halo)
            if blocks is None:
                raise ValueError(f"scratch_bytes={scratch_bytes} holds {max_rows} steps of {C} cells: too few for one step and the "
                                 f"{halo[0]} + {halo[1]} steps of its window around it; raise scratch_bytes")
        else:
            blocks = [(r0, r1, r0, r1) for r0, r1 in _time_blocks(T, max_rows)]
        self.cells, self._blocks, self._producer = C, blocks, p
        self._buffer = field if p is None else self._ctx.empty((max(b1 - b0 for _, _, b0, b1 in blocks), C), p.dtype)
        return self

    def result(self, shape, out=None):
        """``out``, or a new float64 DeviceArray that is freed if the walk ends in an exception"""
        buf = self._ctx._result_buffer(out, shape, True)
        if out is None:
            self._results.append(buf)
        return buf

    def __iter__(self):
        p = self._producer
        for i0, i1, b0, b1 in self._blocks:
            block = self._buffer.rows(0, b1 - b0)
            if p is not None:
                for r0, r1 in _time_blocks(b1 - b0, self._piece or b1 - b0):
                    p.produce(b0 + r0, b0 + r1, out=block.rows(r0, r1))
            yield i0, i1, block, b0

    def __exit__(self, exc_type, exc, tb):
        for a in [self._buffer] + (self._results if exc_type is not None else []):
            a.free()
        return False


class walk_pair:
    """``with walk_pair(a, b, dim, ctx, scratch_bytes, consumer, bins=offsets) as w: for i0, i1, block_a, block_b, b0 in w: ...``: two
    sources of the same steps and cells walked in lock-step, each through a ``walk`` of its own.  If neither is a lazy array the
    consumer takes whole from HBM, both are cut into the same runs of whole bins, sized so that the two blocks together stay within
    ``scratch_bytes`` (at least one bin).  If one is taken whole, the other is brought in whole too (``whole=True``).  A bin always lies
    within one block of both.  ``w.cells``, ``w.result(shape)`` and the freeing of every buffer are those of ``walk``."""

    def __init__(self, a, b, dim, ctx, scratch_bytes, consumer, bins, verb="compare"):
        self._args = a, b, dim, int(scratch_bytes), consumer, bins, verb
        self._ctx, self._stack, self._walks = ctx, None, None

    def __enter__(self):
        a, b, dim, scratch_bytes, consumer, bins, verb = self._args
        for s in (a, b):
            if min(s.sizes.values(), default=1) < 1:
                raise ValueError(f"nothing to {verb}: the array has sizes {s.sizes}")
        if takes_whole(a, consumer, dim) or takes_whole(b, consumer, dim):
            plans = [dict(source=s, whole=True) for s in (a, b)]
        else:
            pa, pb = producer_of(a, dim, self._ctx), producer_of(b, dim, self._ctx)
            if (pa.rows, pa.cells) != (pb.rows, pb.cells):
                raise ValueError(f"the sources differ: [{pa.rows}, {pa.cells}] and [{pb.rows}, {pb.cells}] steps by cells")
            budget = max(1, scratch_bytes // (pa.cells * (pa.dtype.itemsize + pb.dtype.itemsize)))
            plans = [dict(source=p, row_budget=budget) for p in (pa, pb)]
        with contextlib.ExitStack() as stack:
            self._walks = [stack.enter_context(walk(p.pop("source"), dim, self._ctx, scratch_bytes, consumer, bins=bins, verb=verb, **p))
                           for p in plans]
            wa, wb = self._walks
            if wa.cells != wb.cells or [k[:2] for k in wa._blocks] != [k[:2] for k in wb._blocks]:
                raise ValueError(f"the sources differ: {wa.cells} and {wb.cells} cells per step")
            self.cells = wa.cells
            self._stack = stack.pop_all()
        return self

    def result(self, shape, out=None):
        return self._walks[0].result(shape, out)

    def __iter__(self):
        for (i0, i1, block_a, b0), (_, _, block_b, _) in zip(*self._walks):
            yield i0, i1, block_a, block_b, b0

    def __exit__(self, exc_type, exc, tb):
        return self._stack.__exit__(exc_type, exc, tb)
