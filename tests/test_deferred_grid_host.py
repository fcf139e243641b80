"""``DeferredGridArray`` (skdownscale_amd/core.py), the base of what ``interp_like``, ``resample`` and ``disaggregate`` return, on a stub
whose ``_compute_values`` counts its calls: nothing is computed before the field is asked for, and it is computed once.  And
``chunk_lengths``, the block lengths ``GridArray.chunk`` and the lazy arrays' own ``chunk`` share.  No GPU."""
import numpy as np
import pytest

from skdownscale_amd.core import DeferredGridArray, GridArray, chunk_lengths


class Stub(DeferredGridArray):
    def __init__(self):
        self.dims, self.coords, self.name = ("time", "y", "x"), {"time": np.arange(2), "y": np.arange(3.0), "x": np.arange(4.0)}, "stub"
        self.calls = 0

    @property
    def sizes(self):
        return {"time": 2, "y": 3, "x": 4}

    def _compute_values(self):
        self.calls += 1
        return self._in_dims(np.arange(24.0).reshape(3, 8), ("y", "time", "x"))  # (rows of y, the other two dims flattened)

    def __repr__(self):
        return f"<Stub {self.sizes} computed={self.computed}>"


def test_nothing_is_computed_before_the_field_is_asked_for():
    a = Stub()
    assert a.shape == (2, 3, 4) and a.sizes == {"time": 2, "y": 3, "x": 4} and a.dtype == np.float64
    assert repr(a) == "<Stub {'time': 2, 'y': 3, 'x': 4} computed=False>"
    assert a.chunks is None and a.chunksizes is None
    assert a.calls == 0 and not a.computed


def test_the_field_is_computed_once():
    a = Stub()
    want = np.arange(24.0).reshape(3, 2, 4).transpose(1, 0, 2)
    v = a.values
    assert a.calls == 1 and a.computed and v.shape == a.shape and np.array_equal(v, want)
    assert a.values is v
    c = a.compute()
    assert type(c) is GridArray and c.values is v and c.dims == a.dims and c.name == "stub" and set(c.coords) == set(a.coords)
    t = a.transpose("x", "time", "y")
    assert type(t) is GridArray and t.dims == ("x", "time", "y") and np.array_equal(t.values, want.transpose(2, 0, 1))
    s = a.isel(y=slice(1, 3), x=slice(0, 2))
    assert type(s) is GridArray and np.array_equal(s.values, want[:, 1:3, 0:2]) and np.array_equal(s.coords["y"], [1.0, 2.0])
    assert np.array_equal(a.transpose("time", ...).values, want) and np.array_equal(a.values, want)
    assert a.calls == 1
    assert repr(a) == "<Stub {'time': 2, 'y': 3, 'x': 4} computed=True>"


def test_any_first_request_computes():
    for ask in (lambda a: a.compute(), lambda a: a.transpose("x", "y", "time"), lambda a: a.isel(time=slice(0, 1)), lambda a: a.values):
        a = Stub()
        ask(a)
        ask(a)
        assert a.calls == 1


# size -> block length asked for -> block lengths: one block for -1, None and a length that reaches the end, a shorter last block else
CHUNKS = {0: {-1: (0,), None: (0,), 3: (0,), 10: (0,), 11: (0,)},
          1: {-1: (1,), None: (1,), 3: (1,), 10: (1,), 11: (1,)},
          7: {-1: (7,), None: (7,), 3: (3, 3, 1), 10: (7,), 11: (7,)},
          10: {-1: (10,), None: (10,), 3: (3, 3, 3, 1), 10: (10,), 11: (10,)}}


@pytest.mark.parametrize("n", sorted(CHUNKS))
@pytest.mark.parametrize("block", [-1, None, 3, 10, 11])
def test_chunk_lengths(n, block):
    assert chunk_lengths({"x": n}, {"x": block}) == {"x": CHUNKS[n][block]}
    assert GridArray(np.zeros(n), ("x",)).chunk({"x": block}).chunksizes == {"x": CHUNKS[n][block]}


def test_chunk_lengths_of_a_dim_that_is_not_named():
    assert chunk_lengths({"x": 7, "y": 10}, {"y": 3}) == {"x": (7,), "y": (3, 3, 3, 1)}
    assert chunk_lengths({"x": 7, "y": 10}, None) == {"x": (7,), "y": (10,)}
