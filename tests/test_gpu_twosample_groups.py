"""GPU: Context.twosample_groups / sd_twosample_groups -- the kernels of sd_twosample (csrc/sd_twosample.hip) reading their rows through
the group-sorted row table -- against the grouped oracle (tests/_grouped_pair_oracle.py) and against ``ctx.twosample`` on the fields
gathered on the host, ``(a[rows], b[rows], offsets)``: the defining property, bit for bit."""
import numpy as np
import pytest

import _grouped_pair_oracle as gp
import _twosample_oracle as ts

pytestmark = pytest.mark.gpu

STATS = list(ts.STATS)
WIDTH, ORIGIN = 0.5, 0.0625
CELLS = [1, 8, 9, 17]
# the longest group -> the kernels that serve the call: every segment width, then the series path (1 216 = 64 * 19 is the widest segment)
KERNELS = {320: ["twosample_segment_kernel<5>"], 321: ["twosample_segment_kernel<7>"], 448: ["twosample_segment_kernel<7>"],
           832: ["twosample_segment_kernel<13>"], 1216: ["twosample_segment_kernel<19>"],
           1217: ["quantile_runs_kernel<13>", "twosample_select_kernel<13>"]}


@pytest.fixture(scope="module")
def ctx():
    from skdownscale_amd.engine import Context

    return Context(0)


def deal(rng, sizes):
    """group ids with ``sizes[g]`` rows of group g, in a shuffled order"""
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def fields(rng, shape, nan_share=0.05, tied=True):
    """a pair of fields -- in multiples of 1 / 8 (exact in float32 too, heavily tied) or continuous -- with NaN at places of their own"""
    a = rng.normal(size=shape) * 2.0
    b = 0.25 + rng.normal(size=shape) * 2.5
    if tied:
        a, b = np.round(a * 8.0) / 8.0, np.round(b * 8.0) / 8.0
    a[rng.random(shape) < nan_share] = np.nan
    b[rng.random(shape) < nan_share] = np.nan
    return a, b


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} want {want[bad][0]!r}"


def kernels_of(ctx, call):
    """the profiler names of the launches of ``call()``"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        res = call()
        names = sorted(ctx.prof())
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    return res, names


def gathered(ctx, a, b, group, G, stats, width=WIDTH, origin=ORIGIN):
    rows, offsets = gp.tables(group, G)
    return ctx.twosample(np.ascontiguousarray(a[rows]), np.ascontiguousarray(b[rows]), offsets, stats, width, origin).to_host()


@pytest.mark.parametrize("longest", list(KERNELS))
def test_every_path_with_interleaved_ids(ctx, longest):
    rng = np.random.default_rng(300 + longest)
    sizes = [0, 1, 7, longest, 40, 0, 33]  # an id that never occurs first and in the middle, one row, short groups, the longest
    group = deal(rng, sizes)
    G, T = len(sizes), len(group)
    assert T <= 2600
    for C in CELLS:
        a64, b64 = fields(rng, (T, C))
        b64[group == 4, 0] = np.nan  # a group that is all NaN in one field only, in cell 0
        a64[group == 3, C - 1] = np.nan  # ... and the longest in the other, in the last cell
        want = gp.twosample(a64, b64, group, G, STATS, WIDTH, ORIGIN)
        for ta, tb in ((np.float64, np.float64), (np.float32, np.float64)):  # (multiples of 1 / 8 are exact in float32: the same expectation)
            what = f"longest={longest} C={C} {np.dtype(ta).name} {np.dtype(tb).name}"
            a, b = a64.astype(ta), b64.astype(tb)
            got, names = kernels_of(ctx, lambda: ctx.twosample_groups(a, b, group, G, STATS, WIDTH, ORIGIN).to_host())
            assert names == KERNELS[longest], names
            same(got, want, what)
            same(got, gathered(ctx, a, b, group, G, STATS), what + " against ctx.twosample on the gathered fields")
        got = got.reshape(4, G, C)
        assert (got[2:, [0, 5]] == 0.0).all() and np.isnan(got[:2, [0, 5]]).all()  # the ids that never occur
        assert got[3, 4, 0] == 0.0 and got[2, 4, 0] > 0 and np.isnan(got[:2, 4, 0]).all()  # nb = 0, na > 0
        assert got[2, 3, C - 1] == 0.0 and got[3, 3, C - 1] > 0 and np.isnan(got[:2, 3, C - 1]).all()
        if C > 2:  # NaN are unpaired: each field counts its own samples
            na, nb = got[2, 3, 1], got[3, 3, 1]
            va, vb = ~np.isnan(a64[group == 3, 1]), ~np.isnan(b64[group == 3, 1])
            assert na == va.sum() and nb == vb.sum() and min(na, nb) > (va & vb).sum()
    # symmetric under swapping the fields; continuous data with float32 on one side: the expectation of the cast field
    a64, b64 = fields(rng, (T, 9), 0.05, tied=False)
    a32 = a64.astype(np.float32)
    fwd = ctx.twosample_groups(a32, b64, group, G, ["ks", "perkins", "na", "nb"], WIDTH, ORIGIN).to_host()
    same(fwd, gp.twosample(a32, b64, group, G, STATS, WIDTH, ORIGIN), f"longest={longest} continuous float32")
    bwd = ctx.twosample_groups(b64, a32, group, G, ["ks", "perkins", "nb", "na"], WIDTH, ORIGIN).to_host()
    same(bwd, fwd, f"longest={longest} swapped")


def test_groups_that_are_runs_of_rows_equal_the_binned_call(ctx):
    rng = np.random.default_rng(12)
    for lengths in ([0, 1, 40, 330, 9], [3, 1300, 0, 50]):  # the segment path and the series path
        group = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        a, b = fields(rng, (len(group), 9))
        same(ctx.twosample_groups(a, b, group, len(lengths), STATS, WIDTH, ORIGIN).to_host(),
             ctx.twosample(a, b, offsets, STATS, WIDTH, ORIGIN).to_host(), f"lengths={lengths}")


def test_views_the_host_twin_and_each_statistic_alone(ctx):
    rng = np.random.default_rng(8)
    for sizes in ([0, 1, 40, 330, 9], [1300, 20]):
        group = deal(rng, sizes)
        G, T, C = len(sizes), len(group), 9
        a, b = fields(rng, (T, C))
        want = gp.twosample(a, b, group, G, STATS, WIDTH, ORIGIN)
        same(ctx.twosample_groups_host(a, b, group, G, STATS, WIDTH, ORIGIN), want, "sd_twosample_groups")
        for s, stat in enumerate(STATS):
            same(ctx.twosample_groups(a, b, group, G, [stat], WIDTH, ORIGIN).to_host(), want[s * G:(s + 1) * G], f"{stat} alone")
        # padded and offset views of a, b and the output, the planes of the output two rows further apart than G
        pa, pb = np.full((T, C + 5), 7.0), np.full((T, C + 8), 7.0)
        pa[:, 1:1 + C], pb[:, 4:4 + C] = a, b
        plane = G + 2
        parent = ctx.to_device(np.full((4 * plane, C + 3), 7.0))
        view = parent.cells(2, 2 + C)
        ctx.twosample_groups(ctx.to_device(pa).cells(1, 1 + C), ctx.to_device(pb).cells(4, 4 + C), group, G, STATS, WIDTH, ORIGIN, out=view.rows(0, G),
                             plane_rows=plane)
        back = parent.to_host().reshape(4, plane, C + 3)
        same(np.ascontiguousarray(back[:, :G, 2:2 + C]).reshape(4 * G, C), want, "views")
        back[:, :G, 2:2 + C] = 7.0
        assert (back == 7.0).all()  # padding untouched


def test_refusals_through_the_c_abi_launch_nothing(ctx):
    from skdownscale_amd._lib import check, ptr

    x = np.arange(40.0).reshape(10, 4)
    a, b, out = ctx.to_device(x), ctx.to_device(x + 1.0), ctx.empty((6, 4))
    ids = np.array([1, 0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=np.int32)
    codes = np.array([0, 1, 2, 0], dtype=np.intc)

    def call(ld_a=4, ld_b=4, T=10, C=4, group=ids, G=2, stats=codes, nstat=3, width=1.0, origin=0.0, ld_out=4, stride=8):
        check(ctx.lib.sd_twosample_groups_dev(ctx.handle, a.vptr, 0, ld_a, b.vptr, 0, ld_b, T, C, ptr(group), G, ptr(stats), nstat, width, origin,
                                              out.vptr, ld_out, stride))

    ctx.prof_reset()
    ctx.prof_enable(True)
    who = "sd_twosample_groups: "
    bad = ids.copy()
    bad[3] = 2
    for kw, msg in ((dict(stats=np.array([0, 4, 0, 0], dtype=np.intc)), who + r"unknown statistic code 4 \(stats\[1\]\)"),
                    (dict(nstat=5), who + "nstat = 5, expected 1 to 4 statistics"), (dict(width=0.0), who + "width = 0, expected a positive finite bin width"),
                    (dict(origin=np.inf), who + "origin = inf"), (dict(T=0), who + r"bad sizes \(T=0, C=4\)"),
                    (dict(ld_b=3), who + "ld_b = 3 is less than the 4 cells of a row"),
                    (dict(stride=7), who + r"stride_out = 7 is less than the 8 elements of one statistic \(G \* ld_out\)"),
                    (dict(G=0, stride=0), who + r"bad sizes \(G=0\)"), (dict(group=bad), who + r"group\[3\] = 2 lies outside the 2 groups"),
                    (dict(group=bad, G=0, stride=0), who + r"bad sizes \(G=0\)"), (dict(group=bad, ld_a=1 << 29), who + r"group\[3\] = 2"),
                    (dict(ld_a=1 << 29), who + "rows of 536870912 and 4 elements exceed the 32-bit row addressing")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    big = np.zeros((19458, 1))
    ids_big = np.zeros(19458, dtype=np.int32)
    ids_big[7] = 1  # 19 457 rows in group 0, not consecutive
    with pytest.raises(NotImplementedError, match=who + r"a group of 19457 samples exceeds the workgroup merge \(19456\)"):
        ctx.twosample_groups(big, big, ids_big, 2, ["ks"])
    with pytest.raises(NotImplementedError, match=who + "a group of 19457 samples"):
        ctx.twosample_groups_host(big, big, ids_big, 2, ["ks"])
    assert not any(k.startswith(("twosample", "quantile")) for k in ctx.prof())  # nothing was launched
    call()
    assert ctx.prof()["twosample_segment_kernel<5>"]["launches"] == 1
    ctx.prof_enable(False)
    same(out.to_host(), gp.twosample(x, x + 1.0, ids, 2, ["ks", "perkins", "na"], 1.0), "the raw call")
    ids_big[5000:5002] = 1  # 19 455 rows: the longest the series path takes but one
    got = ctx.twosample_groups(big, big, ids_big, 2, ["ks", "na"]).to_host()
    assert list(got[:, 0]) == [0.0, 0.0, 19455.0, 3.0]
    # the Python wrapper
    with pytest.raises(ValueError, match="perkins needs the width"):
        ctx.twosample_groups(x, x, ids, 2, ["perkins"])
    with pytest.raises(ValueError, match=r"group: expected one group id per row \(10\), got shape \(9,\)"):
        ctx.twosample_groups(x, x, ids[:9], 2, ["ks"])
    with pytest.raises(ValueError, match=r"sd_twosample_groups: bad sizes \(G=-1\)"):
        ctx.twosample_groups(x, x, ids, -1, ["ks"])
