"""CPU stand-in for ``ctx.lib``: every ``sd_*`` attribute is a callable that checks its arguments against ``_lib.SIGNATURES`` (their
number, and that each converts with the argtype's ``from_param``), fills the outputs of ``*_info`` and of creating calls, records
``(name, decoded arguments)`` and returns 0.  Nothing is computed.

Decoding: a pointer into a registered array becomes ``(name, element offset)``, the context handle ``"ctx"``, a handle this library gave
out ``"state<n>"``, any other address ``"mem"`` (the wrappers' own temporaries: status, converted copies, fresh host results), NULL
``None``; an output passed with ``byref`` becomes ``"&"``; numbers are themselves.  Allocation, copies and frees go to ``traffic``, every
other call to ``log``, so that a finalizer running late does not disturb a pinned call list."""
import ctypes as C

import numpy as np

from skdownscale_amd import _lib
from skdownscale_amd.engine import Context, DeviceArray

CTX_HANDLE = 0xC0DE0000
FIRST_STATE = 0x51A7E000
FIRST_BLOCK = 0x7000_0000_0000
TRAFFIC = ("sd_dev_alloc", "sd_dev_free", "sd_memcpy_h2d", "sd_memcpy_d2h", "sd_ctx_destroy")


class RecordingLib:
    def __init__(self):
        self.log, self.traffic = [], []
        self.info = {}  # name of an ``*_info`` entry point -> the values it writes, in the order of its outputs
        self._spans = []  # (first byte, bytes, itemsize, name)
        self._states = {}
        self._next_block = FIRST_BLOCK

    # ---- what the tests register ----
    def host(self, name, a):
        """a host array by its address; -> the array"""
        assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"]
        self._spans.append((a.ctypes.data, max(a.nbytes, 1), a.itemsize, name))
        return a

    def resident(self, ctx, name, shape, dtype=np.float64):
        """a made-up resident array (nothing is allocated); -> the DeviceArray, which owns nothing"""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = DeviceArray(ctx, shape, dtype, dptr=self._block(name, nbytes, np.dtype(dtype).itemsize), owner=False)
        return a

    def _block(self, name, nbytes, itemsize):
        first = self._next_block
        self._next_block += (nbytes + 0xFFF) // 0x1000 * 0x1000 + 0x1000
        self._spans.append((first, max(nbytes, 1), itemsize, name))
        return first

    # ---- decoding ----
    def _address(self, value):
        if value is None:
            return None
        if value == CTX_HANDLE:
            return "ctx"
        if value in self._states:
            return self._states[value]
        for first, nbytes, itemsize, name in self._spans:
            if first <= value < first + nbytes:
                assert (value - first) % itemsize == 0, (name, value - first)
                return (name, (value - first) // itemsize)
        return "mem"

    def _decode(self, arg, argtype):
        argtype.from_param(arg)  # raises what a call into the real library would raise
        if hasattr(arg, "_obj"):  # byref(x)
            return "&"
        if argtype is C.c_void_p:
            return self._address(arg.value if isinstance(arg, C.c_void_p) else arg)
        if argtype is C.c_char_p:
            return arg
        return float(arg) if argtype is C.c_double else int(arg)

    def __getattr__(self, name):
        if not name.startswith("sd_"):
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments, the header has {len(argtypes)}"
            decoded = [self._decode(a, t) for a, t in zip(args, argtypes)]
            outputs = [a._obj for a in args if hasattr(a, "_obj")]
            if name == "sd_dev_alloc":
                outputs[0].value = self._block(f"block{sum(n == name for n, _ in self.traffic)}", int(args[1]), 1)
            elif name.endswith("_info") and name in self.info:
                assert len(outputs) == len(self.info[name]), name
                for o, v in zip(outputs, self.info[name]):
                    o.value = v
            elif outputs and argtypes[-1] == C.POINTER(C.c_void_p):  # a creating call: its last argument takes the handle
                handle = FIRST_STATE + 0x100 * len(self._states)
                self._states[handle] = f"state{len(self._states)}"
                outputs[-1].value = handle
            (self.traffic if name in TRAFFIC else self.log).append((name, decoded))
            return 0

        return call


def context(lib=None):
    """a Context that never saw a GPU: ``lib`` is a RecordingLib"""
    ctx = Context.__new__(Context)
    ctx.lib = RecordingLib() if lib is None else lib
    ctx.handle = C.c_void_p(CTX_HANDLE)
    ctx.device = 0
    return ctx
