"""GPU: the argument layer of the estimator wrappers (engine.py) on a real context.  Every refusal here is raised before the library is
entered, with its text, once per family, and an ordinary call on the same context afterwards gives the bits it gave before; a host
``out`` is written and handed back by the five wrappers that used to ignore it; ``status()`` of LinregState and QmState equals
``export()["status"]``.

C = 8 cells inside a pitch of 12, T = 24, Tq = 6, F = 2, k = 3: the sizes at which a pitch, a view offset or a rank can still be got
wrong.  The ARRM state alone is fitted on 50 samples, the fewest sd_arrm_fit takes; its queries have Tq = 6 like the others.  Nothing
is computed that tests/test_gpu_state_contract.py does not compute at its larger sizes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, PITCH, C0, T, TQ, F, K = 8, 12, 2, 24, 6, 2, 3
GID, GIDQ = np.repeat(np.arange(2), T // 2).astype(np.int32), np.repeat(np.arange(2), TQ // 2).astype(np.int32)
DAY, YEAR = (np.arange(T) % 12).astype(np.int32), (np.arange(T) // 12).astype(np.int32)  # twelve days of two years
KEY, KEYQ = (np.arange(T) % 4).astype(np.int32), (np.arange(TQ) % 4).astype(np.int32)
RNG = np.random.default_rng(20)
X2, XQ2 = RNG.normal(size=(T, C)), RNG.normal(size=(TQ, C))
X3, XQ3 = RNG.normal(size=(T, F, C)), RNG.normal(size=(TQ, F, C))
Y = 0.8 * X2 + 0.3 * X3.sum(axis=1) + RNG.normal(0.0, 0.5, (T, C))
X_ARRM = RNG.normal(size=(50, C))
Y_ARRM = 0.8 * X_ARRM + RNG.normal(0.0, 0.5, (50, C))

# family -> (fit(ctx) -> state, predict(ctx, state, Xq, out) -> (result, status, ..), the host query, the name of the query in refusals)
FAMILIES = {
    "bcsd": (lambda c: c.bcsd_fit(0, X2, Y, GID, 2), lambda c, s, q, out: c.bcsd_predict(s, q, GIDQ, out=out), XQ2, "X"),
    "qm_predict": (lambda c: c.qm_fit(X2, Y), lambda c, s, q, out: c.qm_predict(s, 0, q, out=out), XQ2, "X"),
    "qm_cunnane": (lambda c: c.qm_fit(X2), lambda c, s, q, out: c.qm_cunnane(s, 0, q, out=out), XQ2, "X"),
    "analog": (lambda c: c.analog_fit(X3, Y), lambda c, s, q, out: c.analog_predict(s, q, K, 3, out=out), XQ3, "Xq"),
    "analogreg": (lambda c: c.analog_fit(X3, Y), lambda c, s, q, out: c.analogreg_predict(s, q, K, out=out), XQ3, "Xq"),
    "linreg": (lambda c: c.linreg_fit(X3, Y), lambda c, s, q, out: c.linreg_predict(s, q, out=out), XQ3, "Xq"),
    "zscore": (lambda c: c.zscore_fit(X2, Y, 2, DAY, YEAR, 12), lambda c, s, q, out: c.zscore_predict(s, q, out=out), XQ2, "Xp"),
    "grouped": (lambda c: c.grouped_fit(X3, Y, KEY, 4, 1), lambda c, s, q, out: c.grouped_predict(s, q, KEYQ, out=out), XQ3, "Xq"),
    "arrm": (lambda c: c.arrm_fit(X_ARRM, Y_ARRM, 2), lambda c, s, q, out: c.arrm_predict(s, q, out=out), XQ2, "Xq"),
}
HOST_OUT_WAS_IGNORED = ("qm_cunnane", "qm_predict", "analog", "analogreg", "linreg")


def resident(ctx, a, dtype=np.float64):
    """a [.., C] on the device as the cells [C0, C0 + C) of a [.., PITCH] parent"""
    parent = np.full(a.shape[:-1] + (PITCH,), 7.0)
    parent[..., C0:C0 + C] = a
    return ctx.to_device(parent, dtype).cells(C0, C0 + C)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


class World:
    """one context with a fitted state and the host-form prediction of every family, made once"""

    def __init__(self, device=0):
        from skdownscale_amd.engine import Context

        self.ctx = Context(device)
        self.states, self.base = {}, {}

    def state(self, family):
        if family not in self.states:
            self.states[family] = FAMILIES[family][0](self.ctx)
        return self.states[family]

    def predict(self, family, q, out=None, state=None):
        return FAMILIES[family][1](self.ctx, self.state(family) if state is None else state, q, out)

    def expected(self, family):
        if family not in self.base:
            self.base[family] = self.predict(family, FAMILIES[family][2])
        return self.base[family]

    def still_works(self, family):
        """the ordinary resident call on a view, after a refusal: the bits of the host form"""
        want, status = self.expected(family)[:2]
        out = self.ctx.empty(want.shape[:-1] + (PITCH,)).cells(C0, C0 + C)
        got = self.predict(family, resident(self.ctx, FAMILIES[family][2]), out)
        assert got[0] is out and same(out.to_host(), want) and np.array_equal(got[1], status)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def elsewhere():
    """a second context on the same device"""
    return World()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_float32_resident_field_is_refused(world, family):
    q, name = FAMILIES[family][2:]
    with pytest.raises(ValueError, match=rf"{name}: expected a float64 \[.*\] field, got shape .* of float32"):
        world.predict(family, resident(world.ctx, q, np.float32))
    world.still_works(family)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_array_of_another_context_is_refused(world, elsewhere, family):
    q, name = FAMILIES[family][2:]
    with pytest.raises(ValueError, match=rf"sd_downscale: sd_\w+: `{name}` belongs to another context"):
        world.predict(family, resident(elsewhere.ctx, q))
    world.still_works(family)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_state_of_another_context_is_refused(world, elsewhere, family):
    with pytest.raises(ValueError, match=r"sd_downscale: sd_\w+: `state` belongs to another context"):
        world.predict(family, resident(world.ctx, FAMILIES[family][2]), state=elsewhere.state(family))
    world.still_works(family)
    elsewhere.still_works(family)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_wrong_resident_out_is_refused(world, elsewhere, family):
    """[Tq, C] results (bcsd, qm, zscore, grouped, arrm) and [Tq, 3, C] ones (analog, analogreg, linreg)"""
    shape = world.expected(family)[0].shape
    q = resident(world.ctx, FAMILIES[family][2])
    words = rf"out: expected a float64 DeviceArray of shape \({', '.join(map(str, shape))}\)"
    from skdownscale_amd.engine import DeviceArray

    longer, whole = (TQ + 1,) + shape[1:], world.ctx.empty(shape)
    overlapping = DeviceArray(world.ctx, shape, dptr=whole.ptr, owner=False, ld=C - 1, base=whole)  # a pitch below the cells
    for out in (np.empty(shape), world.ctx.empty(shape, np.float32), world.ctx.empty(longer[:-1] + (PITCH,)).cells(C0, C0 + C), overlapping):
        with pytest.raises(ValueError, match=words):
            world.predict(family, q, out)
    with pytest.raises(ValueError, match=r"sd_downscale: sd_\w+: `out` belongs to another context"):
        world.predict(family, q, elsewhere.ctx.empty(shape))
    world.still_works(family)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_wrong_host_out_is_refused(world, family):
    shape = world.expected(family)[0].shape
    words = rf"out: expected a C-contiguous float64 array of shape \({', '.join(map(str, shape))}\)"
    for out in (np.zeros((1, 1)), np.zeros(shape, dtype=np.float32), np.zeros(shape[:-1] + (PITCH,))[..., :C], world.ctx.empty(shape)):
        with pytest.raises(ValueError, match=words):
            world.predict(family, FAMILIES[family][2], out)
    world.still_works(family)


@pytest.mark.parametrize("family", HOST_OUT_WAS_IGNORED)
def test_host_out_is_honoured(world, family):
    want, status = world.expected(family)[:2]
    out = np.full(want.shape, 7.0)
    got = world.predict(family, FAMILIES[family][2], out)
    assert got[0] is out and same(out, want) and np.array_equal(got[1], status)


@pytest.mark.parametrize("family", ["linreg", "qm_predict", "qm_cunnane"])
def test_status_is_the_exported_status(world, family):
    state = world.state(family)
    status = state.status()
    assert status.dtype == np.int32 and status.shape == (C,)
    assert np.array_equal(status, state.export(with_y=False)["status"] if family == "qm_cunnane" else state.export()["status"])
