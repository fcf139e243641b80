"""Records, for a fixed list of calls of one kernel family (one call per path of its launch plan: csrc/sd_analog_plan.h,
csrc/sd_qm_plan.h), the profiler's kernel names with their launch counts and a SHA-256 of the outputs.  Two trees that launch the
same kernels and compute the same bits give the same file.

    python tools/dev/plan_launches.py --family analog|qm --out FILE --section prod
    SD_DOWNSCALE_LIB=.../libsd_downscale_dev.so python tools/dev/plan_launches.py --family qm --out FILE --section dev   # + the switches

--root DIR runs the package of another checkout of this repository (A/B against a parent build).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

BEST, SAMPLE, WEIGHT, MEAN = 0, 1, 2, 3


def analog_fields(seed, T, Tq, C, F=1, ties=0, decimals=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, F, C))
    y = 2.0 * X[:, 0, :] + rng.standard_normal((T, C))
    Xq = rng.standard_normal((Tq, F, C))
    if ties:  # equal training values: those cells leave the tagged sort and the fused kernel
        X[:, 0, :ties] = np.round(X[:, 0, :ties], decimals)
    return X, y, Xq


def analog_calls(ctx):
    """-> (calls, [(switch, call)]): one call per path of the analog plan; the development switches, each on the call it redirects"""
    fields = analog_fields

    def predict(X, y, Xq, k, kind, **kw):
        st = ctx.analog_fit(X, y)
        return ctx.analog_predict(st, Xq, k, kind, **kw)

    def regress(X, y, Xq, k, twice=False, **kw):
        st = ctx.analog_fit(X, y)
        outs = ctx.analogreg_predict(st, Xq, k, **kw)
        return outs + ctx.analogreg_predict(st, Xq, k, **kw) if twice else outs

    big = fields(1, 14600, 14600, 2048)  # the bench shape of config 4, fewer cells
    tied = fields(2, 14600, 14600, 2048, ties=40)
    most = fields(3, 9400, 3000, 64, ties=48)
    f3 = fields(4, 4096, 4096, 512, F=3)
    short = fields(5, 3000, 1000, 200)
    calls = {
        "fused_mean_k30": lambda: ctx.analog_fit_predict(*big, 30, MEAN),
        "fused_some_handed_back": lambda: ctx.analog_fit_predict(*tied, 30, MEAN),
        "fused_most_handed_back": lambda: ctx.analog_fit_predict(*most, 30, MEAN),
        "fit_predict_weight_split": lambda: ctx.analog_fit_predict(*big, 30, WEIGHT),
        "mean3_from_state": lambda: predict(*big, 30, MEAN),
        "mean3_k1": lambda: predict(*short, 1, MEAN),
        "default_best_n200_window": lambda: predict(*big, 200, BEST),
        "weight_k30_mean_kernel_runs": lambda: predict(*big, 30, WEIGHT),
        "mean_thresh_mean_kernel": lambda: predict(*short, 30, MEAN, thresh=0.5),
        "regression_k30_direct": lambda: regress(*big, 30),
        "regression_n200_prefix_twice": lambda: regress(*big, 200, twice=True),
        "regression_thresh_walk": lambda: regress(*short, 30, thresh=0.5),
        "neighbors_walk": lambda: predict(*short, 30, MEAN, want_neighbors=True),
        "sample_walk": lambda: predict(*short, 30, SAMPLE, sample_inds=np.random.default_rng(9).integers(0, 30, (1000, 200)).astype(np.int32)),
        "f3_slab_topk": lambda: predict(*f3, 30, MEAN),
        "f3_slab_heap_k40": lambda: predict(*f3, 40, MEAN),
        "f3_regression_k30": lambda: regress(*f3, 30),
        "f2_long_queries_bf2": lambda: predict(*fields(6, 1000, 20000, 16, F=2), 30, MEAN),
        "f2_k300_bf": lambda: predict(*fields(7, 1000, 500, 16, F=2), 300, MEAN),
        "f1_T20000_bf2": lambda: predict(*fields(8, 20000, 100, 8), 5, MEAN),
    }
    switches = [
        ("SD_ANALOG_NOSLAB", "f3_slab_topk"), ("SD_ANALOG_SLAB_CLASSES", "f3_slab_topk"), ("SD_ANALOG_HEAP", "f3_slab_topk"),
        ("SD_ANALOG_NOTILE", "fused_mean_k30"), ("SD_ANALOG_REG_PREFIX", "regression_k30_direct"), ("SD_ANALOG_NORUNS", "weight_k30_mean_kernel_runs"),
        ("SD_ANALOG_RUNS_ALWAYS", "fused_mean_k30"), ("SD_ANALOG_COUNT", "fused_some_handed_back"), ("SD_ANALOG_RUNS_ALWAYS", "mean3_from_state"),
    ]
    return calls, switches


def qm_calls(ctx):
    """-> (calls, [(switch, call)]): one call per path of the quantile-mapping plan"""
    C = 72  # nine tiles of eight cells: two groups of eight tiles, the second one partial

    def fields(seed, T, Tp, bad=False):
        rng = np.random.default_rng(seed)
        X = np.round(3 * rng.standard_normal((T, C)), 3)  # (rounded: ties in the sorts and the ranks)
        y = np.round(4 * rng.standard_normal((T, C)), 3) + 2.0
        Xp = np.round(3.5 * rng.standard_normal((Tp, C)), 3) + 1.0
        if bad:
            X[0, 3] = np.nan   # a masked cell
            y[17, 5] = np.inf  # non-finite cells: in the fit, in the new series
            Xp[2, 7] = np.nan
        return X, y, Xp

    def fit(T, with_y):
        X, y, _ = fields(T, T, 10)
        st = ctx.qm_fit(X, y if with_y else None)
        e = st.export(with_y=with_y)
        st.close()
        return [e["x_sorted"], e["status"]] + ([e["y_sorted"]] if with_y else [])

    def predict(f, model, ex):
        st = ctx.qm_fit(f[0], f[1])
        out = ctx.qm_predict(st, model, f[2], ex, 10)
        st.close()
        return out

    def cunnane(f, direction):
        st = ctx.qm_fit(f[0])
        Z = f[2] if direction == 0 else np.random.default_rng(5).uniform(-0.2, 1.2, f[2].shape)
        out = ctx.qm_cunnane(st, direction, Z, "both", 10)
        st.close()
        return out

    short = fields(11, 3000, 1000)
    long_ = fields(12, 14600, 14600)  # fitted series above half of the LDS: one qm_map_kernel workgroup per CU
    calls = {}
    for T in (3000, 14600, 17408, 17409):  # tile widths 13 / 15 / 17 and transpose + qm_sort_kernel<19>
        calls[f"fit_y_T{T}"] = lambda T=T: fit(T, True)
        calls[f"fit_no_y_T{T}"] = lambda T=T: fit(T, False)
    for name, model in (("qmr", 0), ("ecm_difference", 1), ("ecm_ratio", 2)):
        for ex in (None, "1to1", "min", "both"):
            calls[f"{name}_{ex}"] = lambda model=model, ex=ex: predict(short, model, ex)
    calls["cunnane_forward"] = lambda: cunnane(short, 0)
    calls["cunnane_inverse"] = lambda: cunnane(short, 1)
    calls["qmr_T14600_Tp14600"] = lambda: predict(long_, 0, None)
    calls["ecm_T14600_Tp14600"] = lambda: predict(long_, 1, None)
    calls["ecm_T14600_Tp9000"] = lambda: predict((long_[0], long_[1], long_[2][:9000]), 1, None)
    calls["qmr_T3000_Tp10241"] = lambda: predict(fields(13, 3000, 10241), 0, "both")
    calls["masked_and_nonfinite_cells"] = lambda: predict(fields(14, 3000, 1000, bad=True), 1, "both")
    return calls, [("SD_QM_NOTILE", "fit_y_T14600"), ("SD_QM_DIVIDE", "ecm_difference_both")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["analog", "qm"], required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--section", default="prod")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.root, "scikit-downscale_amd"))
    from skdownscale_amd.engine import Context

    ctx = Context(0)
    ctx.prof_enable(True)
    result = {}

    def record(name, fn, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        ctx.prof_reset()
        outs = fn()
        for k in env or {}:
            del os.environ[k]
        h = hashlib.sha256()
        for a in outs:
            h.update(np.ascontiguousarray(a).tobytes())
        result[name] = {"launches": {k: v["launches"] for k, v in sorted(ctx.prof().items())}, "sha256": h.hexdigest()}
        print(name, result[name], flush=True)

    calls, switches = (analog_calls if args.family == "analog" else qm_calls)(ctx)
    if args.section == "dev":
        for var, call in switches:
            record(f"{var}:{call}", calls[call], {var: "1"})
    else:
        for name, fn in calls.items():
            record(name, fn)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc[args.section] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
