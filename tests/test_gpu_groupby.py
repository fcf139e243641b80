"""GPU: groupby_reduce_kernel and groupby_apply_kernel (csrc/sd_groupby.hip) through Context.groupby_reduce / groupby_apply and the C
ABI against tests/_groupby_oracle.py, pandas' and the reference's results in tests/golden/g26_groupby.npz, and the lazy
GridArray.groupby surface with its chaining with interp_like, resample and disaggregate.

The oracle is the definition of the reduction (a row-by-row loop), so ``sum`` and ``mean`` are compared with it bit for bit, as are the
results of different layouts, cells per lane, geometries and cuts of the time axis: a (group, cell) is added in row order by one lane.
Against pandas and the reference the bound is that of tests/_groupby_oracle.py: |got - want| <= (n + 2) * 2^-53 * sum|x_i| for ``sum``
of a group with n non-NaN samples, the same divided by n plus one ulp for ``mean``."""
import os

import numpy as np
import pandas as pd
import pytest

import _groupby_oracle as go

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# T = 120, G = 12 (more than one workgroup): an absent first, middle and last group; 1 row; 7, 8, 9 rows (a partial, a whole and a whole
# + partial batch of 8); 16 and 31 rows
SIZES = [0, 1, 7, 8, 9, 31, 0, 31, 8, 16, 9, 0]
CELLS = [1, 63, 64, 65, 130, 257]
OPS = ["mean", "sum"]
APPLY = ["sub", "add", "mul", "div"]
KEYS = ("month", "dayofyear", "year", "season", "month_grouper")
SD_ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "g26_groupby.npz"))
    return {k: g[k] for k in g.files}


def scattered(rng, sizes=SIZES):
    """ids with these group sizes, scattered by a seeded permutation: no group is a run"""
    group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    if sizes is SIZES:
        for g in np.flatnonzero(np.asarray(sizes) > 1):
            rows = np.flatnonzero(group == g)
            assert rows[-1] - rows[0] > len(rows) - 1, f"group {g} is a run"
    return group


def field(rng, group, C):
    """temperatures with 5 % NaN samples, an all-NaN group in cell 0 (the first group of 31) and, in the last cell, NaN in 9 consecutive
    rows of a group"""
    T = len(group)
    x = 285.0 + 10.0 * rng.normal(size=(T, C))
    x[rng.random((T, C)) < 0.05] = np.nan
    sizes = np.bincount(group)
    long = int(np.flatnonzero(sizes == sizes.max())[0])
    rows = np.flatnonzero(group == long)
    x[rows, 0] = np.nan
    x[rows[3:12], -1] = np.nan
    return x


def view(ctx, host, ld, lead, fill=7):
    """the host field inside a wider device field: ``lead`` elements in front of every row, rows ``ld`` apart -> (parent, view)"""
    T, C = host.shape
    parent = np.full((T, ld), fill, dtype=host.dtype)
    parent[:, lead:lead + C] = host
    parent = ctx.to_device(parent, host.dtype)
    return parent, (parent.cells(lead, lead + C) if (ld, lead) != (C, 0) else parent)


def untouched(parent, lead, C, fill=7):
    back = parent.to_host()
    return (back[:, :lead] == fill).all() and (back[:, lead + C:] == fill).all()


def reduce_dev(ctx, src, group, G, op, s, n, carry, out):
    """sd_groupby_reduce_dev on the caller's accumulators (Context.groupby_reduce makes its own when it does not carry)"""
    from skdownscale_amd._lib import GROUPBY_REDUCE_OPS, check, ptr

    group = np.ascontiguousarray(group, dtype=np.int32)
    T, C = src.shape
    assert s.ld == n.ld
    check(ctx.lib.sd_groupby_reduce_dev(ctx.handle, GROUPBY_REDUCE_OPS[op], src.vptr, int(src.dtype == np.float32), src.ld, T, C, ptr(group), G,
                                        s.vptr, n.vptr, s.ld, int(carry), None if out is None else out.vptr, 0 if out is None else out.ld))


def layouts_of(C):
    even = C + 6 if C % 2 == 0 else C + 5  # a padded leading dimension that keeps two cells per lane possible
    quad = C + 8 - C % 4 if C % 4 == 0 else even  # ... and four for float32 where C allows
    # (name, source ld, elements in front of a source row, ld and lead of the accumulators, ld and lead of the output / table)
    return [("tight", C, 0, C, 0, C, 0), ("padded even", even + 2, 4, even, 2, even + 4, 2), ("padded by four", quad + 4, 4, quad, 4, quad + 8, 4),
            ("padded odd", C + 5 - C % 2, 4, C + 3 - C % 2, 2, C + 7 - C % 2, 1), ("output off by one double", C, 0, C, 0, C + 2, 1)]


@pytest.mark.parametrize("C", CELLS + [260])
def test_reduce_shape_sweep(ctx, C):
    rng = np.random.default_rng(2000 + C)
    group = scattered(rng)
    T, G = len(group), len(SIZES)
    assert T == 120 and G == 12
    x64 = field(rng, group, C)
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        want_acc = go.accumulate(host, group, G)
        for op in OPS:
            want = go.finish(want_acc, op)
            for name, ld, lead, ld_acc, lead_acc, ld_out, lead_out in layouts_of(C):
                what = f"C={C} {np.dtype(dtype).name} {op} {name}"
                _, src = view(ctx, host, ld, lead)
                ps, s = view(ctx, np.full((G, C), -3.25), ld_acc, lead_acc)      # garbage: carry == 0 starts from zero
                pn, n = view(ctx, np.full((G, C), 99, dtype=np.int32), ld_acc, lead_acc)
                po, out = view(ctx, np.full((G, C), 7.0), ld_out, lead_out)
                reduce_dev(ctx, src, group, G, op, s, n, 0, out)
                assert np.array_equal(out.to_host(), want, equal_nan=True), f"{what}: differs from the oracle"
                assert np.array_equal(s.to_host(), want_acc[0]) and np.array_equal(n.to_host(), want_acc[1]), f"{what}: accumulators differ"
                for parent, a, b in ((ps, lead_acc, "sum"), (pn, lead_acc, "count"), (po, lead_out, "out")):
                    assert untouched(parent, a, C), f"{what}: padding of {b} written"
            absent = np.asarray(SIZES) == 0
            assert np.isnan(want[absent]).all() if op == "mean" else (want[absent] == 0.0).all()
            assert np.isnan(want[5, 0]) if op == "mean" else want[5, 0] == 0.0  # the all-NaN group
        # the engine's own call and the one-shot host entry: the same bits
        for op in OPS:
            got, acc = ctx.groupby_reduce(host, group, G, op)
            assert np.array_equal(got.to_host(), go.finish(want_acc, op), equal_nan=True)
            assert np.array_equal(acc[0].to_host(), want_acc[0]) and np.array_equal(acc[1].to_host(), want_acc[1]) and acc[1].dtype == np.int32
            assert np.array_equal(ctx.groupby_reduce_host(host, group, G, op), got.to_host(), equal_nan=True)


@pytest.mark.parametrize("G", [1, 3, 8, 9, 16, 17, 25])  # one bin per wave up to 16 groups, two above; whole and partial workgroups
def test_group_counts_reach_every_geometry(ctx, G):
    rng = np.random.default_rng(G)
    sizes = rng.integers(1, 12, size=G)
    if G > 2:
        sizes[G // 2] = 0
    group = scattered(rng, sizes) if G > 1 else np.zeros(sizes[0], dtype=np.int32)
    for C in (65, 130):
        x = field(rng, group, C)
        for op in OPS:
            got, _ = ctx.groupby_reduce(x, group, G, op)
            assert got.shape == (G, C) and np.array_equal(got.to_host(), go.reduce(x, group, G, op), equal_nan=True), (G, C, op)


@pytest.mark.parametrize("cuts", [[37], [1, 38, 119], list(range(1, 120))], ids=["two", "four", "single rows"])
def test_carry_gives_the_bits_of_one_call(ctx, cuts):
    rng = np.random.default_rng(len(cuts))
    group = scattered(rng)
    for C, dtype in ((65, np.float64), (130, np.float64), (260, np.float32)):
        x = field(rng, group, C).astype(dtype)
        d = ctx.to_device(x, dtype)
        for op in OPS:
            whole, (s1, n1) = ctx.groupby_reduce(d, group, 12, op)
            acc, got = None, None
            for a, b in zip([0] + cuts, cuts + [120]):
                got, acc = ctx.groupby_reduce(d.rows(a, b), group[a:b], 12, op, acc=acc, finish=b == 120)
                assert (got is None) == (b != 120)
            assert np.array_equal(got.to_host(), whole.to_host(), equal_nan=True), (C, op)
            assert np.array_equal(acc[0].to_host(), s1.to_host()) and np.array_equal(acc[1].to_host(), n1.to_host())
            assert np.array_equal(got.to_host(), go.reduce(x, group, 12, op), equal_nan=True)


def test_consecutive_groups_equal_resample(ctx):
    rng = np.random.default_rng(11)
    group = np.repeat(np.arange(12), SIZES).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    for C, dtype in ((65, np.float64), (130, np.float64), (260, np.float32)):
        x = field(rng, group, C).astype(dtype)
        for op in OPS:
            got, _ = ctx.groupby_reduce(x, group, 12, op)
            assert np.array_equal(got.to_host(), ctx.resample(x, offsets, op).to_host(), equal_nan=True), (C, op)


def test_inf_follows_ieee(ctx):
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, inf, -inf, 1.0], [5.0, 5.0, 5.0, 5.0], [inf, -inf, nan, 2.0], [2.0, 1.0, nan, 3.0]])
    group = [0, 1, 0, 0]
    assert np.array_equal(ctx.groupby_reduce(x, group, 2, "sum")[0].to_host(), [[inf, nan, -inf, 6.0], [5.0] * 4], equal_nan=True)
    assert np.array_equal(ctx.groupby_reduce(x, group, 2, "mean")[0].to_host(), [[inf, nan, -inf, 2.0], [5.0] * 4], equal_nan=True)


@pytest.mark.parametrize("C", CELLS + [260])
def test_apply_shape_sweep(ctx, C):
    rng = np.random.default_rng(3000 + C)
    group = scattered(rng)
    T, G = len(group), len(SIZES)
    x64 = field(rng, group, C)
    table = 280.0 + 5.0 * rng.normal(size=(G, C))
    table[1, :] = 0.0            # a zero under DIV: inf, and NaN where the sample is zero too
    table[2, -1] = np.nan
    x64[np.flatnonzero(group == 1), C // 2] = 0.0
    for dtype in (np.float64, np.float32):
        host = x64.astype(dtype)
        for op in APPLY:
            want = go.apply(host, group, table, op)
            for name, ld, lead, _, _, ld_out, lead_out in layouts_of(C):
                what = f"C={C} {np.dtype(dtype).name} {op} {name}"
                _, src = view(ctx, host, ld, lead)
                pt, tab = view(ctx, table, ld_out, lead_out)
                po, out = view(ctx, np.full((T, C), 7.0), ld_out + 2, lead_out)
                ctx.groupby_apply(src, group, tab, op, out=out)
                assert np.array_equal(out.to_host(), want, equal_nan=True), f"{what}: differs from NumPy"
                assert untouched(po, lead_out, C) and np.array_equal(tab.to_host(), table, equal_nan=True), f"{what}: padding or table written"
            assert np.array_equal(ctx.groupby_apply(host, group, table, op).to_host(), want, equal_nan=True)
            assert np.array_equal(ctx.groupby_apply_host(host, group, table, op), want, equal_nan=True)
            # float32 equals the widened source
            assert np.array_equal(ctx.groupby_apply(host.astype(np.float64), group, table, op).to_host(), want, equal_nan=True)
        div = go.apply(host, group, table, "div")
        rows = np.flatnonzero(group == 1)
        assert np.isnan(div[rows, C // 2]).all() and (np.isinf(div[rows]) | np.isnan(div[rows])).all()


@pytest.mark.parametrize("T", [1, 8, 17, 33, 129, 300])  # a partial batch, runs and workgroups of the apply grid
def test_apply_row_counts(ctx, T):
    rng = np.random.default_rng(T)
    group = rng.integers(0, 5, size=T).astype(np.int32)
    for C in (65, 130):
        x, table = rng.normal(size=(T, C)), rng.normal(size=(5, C))
        assert np.array_equal(ctx.groupby_apply(x, group, table, "sub").to_host(), go.apply(x, group, table, "sub"))


def test_c_abi_refusals_write_nothing(ctx):
    from skdownscale_amd._lib import ptr

    lib, h = ctx.lib, ctx.handle
    x = ctx.to_device(np.ones((10, 4)))
    s, n, out = ctx.to_device(np.full((3, 4), 7.0)), ctx.to_device(np.full((3, 4), 7, dtype=np.int32), np.int32), ctx.to_device(np.full((3, 4), 7.0))
    table, big = ctx.to_device(np.full((3, 4), 2.0)), ctx.to_device(np.full((10, 4), 7.0))
    ok = np.array([0, 1, 2] * 3 + [0], dtype=np.int32)
    bad = ok.copy()
    bad[6] = 3

    def message():
        return lib.sd_last_error().decode()

    def reduce(op=0, ld=4, T=10, C=4, group=ok, G=3, ld_acc=4, ld_out=4):
        return lib.sd_groupby_reduce_dev(h, op, x.vptr, 0, ld, T, C, ptr(group), G, s.vptr, n.vptr, ld_acc, 0, out.vptr, ld_out)

    def apply(op=0, ld=4, T=10, C=4, group=ok, G=3, ld_t=4, ld_out=4):
        return lib.sd_groupby_apply_dev(h, op, x.vptr, 0, ld, T, C, ptr(group), G, table.vptr, ld_t, big.vptr, ld_out)

    for call, who, lds in ((reduce, "sd_groupby_reduce", ("ld", "ld_acc", "ld_out")), (apply, "sd_groupby_apply", ("ld", "ld_t", "ld_out"))):
        for kw, msg in ((dict(op=9), "unknown op code 9"), (dict(T=0), "bad sizes (T=0, C=4)"), (dict(C=-1), "bad sizes (T=10, C=-1)"),
                        (dict(G=0), "bad sizes (G=0)"), (dict(group=bad), "group[6] = 3 lies outside the 3 groups"),
                        (dict(G=2), "group[2] = 2 lies outside the 2 groups"), *((({name: 3}), f"{name} = 3 is less than the 4 cells of a row") for name in lds)):
            assert call(**kw) == SD_ERR_INVALID and message().endswith(f"{who}: {msg}"), (who, kw, message())
    assert lib.sd_groupby_reduce_dev(h, 0, x.vptr, 0, 4, 10, 4, ptr(ok), 3, None, n.vptr, 4, 0, out.vptr, 4) == SD_ERR_INVALID
    assert message().endswith("sd_groupby_reduce: NULL argument")
    host = np.ones((10, 4))
    res = np.full((3, 4), 7.0)
    assert lib.sd_groupby_reduce(h, 0, ptr(host), 0, 10, 4, ptr(bad), 3, ptr(res)) == SD_ERR_INVALID and (res == 7.0).all()
    for a in (s, n, out, big):
        assert (a.to_host() == 7).all()
    # the engine's words
    with pytest.raises(ValueError, match=r"sd_groupby_reduce: group\[6\] = 3 lies outside the 3 groups"):
        ctx.groupby_reduce(host, bad, 3)
    with pytest.raises(ValueError, match="group: expected one group id per row"):
        ctx.groupby_reduce(host, ok[:9], 3)
    with pytest.raises(NotImplementedError, match="only 'mean', 'sum'"):
        ctx.groupby_reduce(host, ok, 3, "max")
    with pytest.raises(ValueError, match="acc: expected the"):
        ctx.groupby_reduce(host, ok, 3, acc=(ctx.empty((2, 4)), ctx.empty((2, 4), np.int32)))
    with pytest.raises(ValueError, match="table: expected a float64"):
        ctx.groupby_apply(host, ok, np.zeros((3, 5)), "sub")
    with pytest.raises(ValueError, match="out: expected a float64 DeviceArray of shape"):
        ctx.groupby_apply(host, ok, np.zeros((3, 4)), "sub", out=ctx.empty((3, 4)))


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def groupby_of(a, key, **kw):
    from skdownscale_amd import MONTH_GROUPER

    return a.groupby(time=MONTH_GROUPER, name="month", **kw) if key == "month_grouper" else a.groupby("time." + key, **kw)


@pytest.mark.parametrize("key", KEYS)
def test_goldens_through_the_grid_array(ctx, golden, key):
    from skdownscale_amd import GridArray

    time = pd.DatetimeIndex(golden["time"])
    for name, values in (("f64", golden["values"]), ("f32", golden["values32"])):
        a = GridArray(values, ("time", "cell"), dict(time=time, cell=np.arange(6)))
        gb = groupby_of(a, key)
        G = len(gb.labels)
        for op in OPS:
            lazy = getattr(gb, op)()
            assert not lazy.computed and lazy.shape == golden[f"{name}.{key}.{op}"].shape
            got = lazy.values
            go.check(got, golden[f"{name}.{key}.{op}"], values, gb.group, G, op, f"{name} {key} {op} vs pandas")
            assert np.array_equal(got, go.reduce(values, gb.group, G, op), equal_nan=True), f"{name} {key} {op}: differs from the oracle"
            assert lazy.computed and np.array_equal(np.asarray(lazy.coords[lazy.group_dim]), golden[f"{name}.{key}.labels"])
            assert np.array_equal(lazy.device_field(ctx).to_host(), got, equal_nan=True)
            # five time blocks and more: identical bits
            for scratch_bytes in (1, 200 * 6 * values.itemsize):
                blocked = getattr(groupby_of(a, key, scratch_bytes=scratch_bytes), op)()
                assert np.array_equal(blocked.values, got, equal_nan=True), scratch_bytes


def test_the_reference_climatologies_and_anomalies(ctx, golden):
    from skdownscale_amd import GridArray

    time = pd.DatetimeIndex(golden["ref.time"])
    month = (time.month - 1).to_numpy()
    X = GridArray(golden["ref.X"], ("time", "cell"), dict(time=time))
    y = GridArray(golden["ref.y"], ("time", "cell"), dict(time=time))
    x_climo, y_climo = X.groupby("time.month").mean(), y.groupby("time.month").mean()
    go.check(y_climo.values, golden["ref.y_climo"], golden["ref.y"], month, 12, "mean", "y_climo_")
    go.check(x_climo.values, golden["ref.x_climo"], golden["ref.X"], month, 12, "mean", "_x_climo")
    # _remove_climatology: one subtraction of a climatology that is within the bound b of the reference's, so the anomalies are within
    # b of the reference's, plus one ulp of the anomaly for the rounding of the subtraction
    lazy = GridArray(golden["ref.X"], ("time", "cell"), dict(time=time)).groupby("time.month").mean()
    anoms = X.groupby("time.month") - lazy
    got = anoms.values
    assert not lazy.computed  # the climatology went from the reduction to the subtraction in HBM
    bound = go.bound(golden["ref.X"], month, 12, "mean")[month] + np.spacing(np.abs(golden["ref.anoms"]))
    err = np.abs(got - golden["ref.anoms"])
    print(f"_remove_climatology: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # with the reference's own climatology: exact
    assert np.array_equal((X.groupby("time.month") - golden["ref.x_climo"]).values, golden["ref.anoms"])


@pytest.fixture(scope="module")
def grids():
    from skdownscale_amd import GridArray

    rng = np.random.default_rng(26)
    T = 1096
    time = pd.date_range("2003-01-01", periods=T, freq="D")
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    clat, clon = np.linspace(42.0, 38.0, 4), np.linspace(-110.0, -104.0, 5)
    flat, flon = np.linspace(42.0, 38.0, 9), np.linspace(-110.0, -104.0, 11)
    coarse = GridArray(285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, 4, 5)), ("time", "lat", "lon"), dict(time=time, lat=clat, lon=clon))
    obs = GridArray(283.0 + season[:, None, None] + 2.0 * rng.normal(size=(T, 9, 11)), ("time", "lat", "lon"), dict(time=time, lat=flat, lon=flon))
    return coarse, obs


def test_interp_like_then_groupby_stays_resident(ctx, grids):
    coarse, obs = grids
    for op in OPS:
        fine = coarse.interp_like(obs)
        lazy = getattr(fine.groupby("time.month"), op)()
        got = lazy.values
        assert got.shape == (12, 9, 11) and not fine.computed  # the fine daily field never came to the host
        plain = getattr(coarse.interp_like(obs).compute().groupby("time.month"), op)().values
        assert np.array_equal(got, plain, equal_nan=True)
        blocked = getattr(coarse.interp_like(obs).groupby("time.month", scratch_bytes=200 * 99 * 8), op)().values  # six blocks
        assert np.array_equal(blocked, got, equal_nan=True)
    fine = coarse.interp_like(obs)
    clim = fine.groupby("time.month").mean()
    anom = (fine.groupby("time.month", scratch_bytes=150 * 99 * 8) - clim).values
    assert not fine.computed and not clim.computed
    full = coarse.interp_like(obs).values
    month = obs.coords["time"].month - 1
    assert np.array_equal(anom, full - clim.values[month], equal_nan=True)


def test_resample_then_groupby_stays_resident(ctx, grids):
    from skdownscale_amd import GridArray

    _, obs = grids
    monthly = obs.resample(time="MS").mean()
    clim = monthly.groupby("time.month").mean()
    got = clim.values
    assert got.shape == (12, 9, 11) and not monthly.computed  # neither the daily nor the monthly field crossed PCIe
    computed = obs.resample(time="MS").mean().compute()
    assert type(computed) is GridArray and np.array_equal(computed.groupby("time.month").mean().values, got)
    # time in the middle of the source, and a sliced lazy reduction
    swapped = GridArray(obs.values.transpose(1, 0, 2), ("lat", "time", "lon"), obs.coords).groupby("time.month").mean()
    assert swapped.dims == ("lat", "month", "lon")
    assert np.array_equal(swapped.values.transpose(1, 0, 2), obs.groupby("time.month").mean().values)
    part = obs.groupby("time.month").mean().isel(lat=slice(2, 5), lon=slice(1, 8))
    assert not part.computed and np.array_equal(part.values, obs.groupby("time.month").mean().values[:, 2:5, 1:8])


def test_anomalies_disaggregate_with_the_lazy_climatology(ctx, grids):
    _, obs = grids
    m = obs.resample(time="MS").mean()
    clim = m.groupby("time.month").mean()
    anom = m.groupby("time.month") - clim
    got = anom.disaggregate(obs, years="same", climatology=clim).values
    want = m.disaggregate(obs, years="same").values
    assert got.shape == want.shape == obs.shape
    # two roundings separate the two targets: anom = fl(m - c) and tgt' = fl(c + anom), each within half an ulp of its result, so
    # |tgt' - m| <= e = 2^-53 * (|m - c| + |tgt'|) <= 2^-53 * (2 |m| + |c| + e).  The kernel then forms by = fl(tgt - mean) and
    # out = fl(x + by): by moves by at most e plus one ulp of by (the two roundings of by need not agree), out by that plus one ulp of
    # out.  |by| <= |m| + |mean| + e <= 2 A with A the largest magnitude of either field.
    mv, cv = m.values, clim.values[m.coords["time"].month - 1]
    e = 2.0 ** -53 * (2 * np.abs(mv) + np.abs(cv)) * (1 + 2.0 ** -50)
    A = max(np.abs(mv).max(), np.abs(obs.values).max())
    month_of_day = np.repeat(np.arange(len(mv)), m.coords["time"].days_in_month)
    bound = e[month_of_day] + np.spacing(2 * A) + np.spacing(np.abs(want))
    err = np.abs(got - want)
    print(f"anomaly round trip: max err = {err.max():.3e}, max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
