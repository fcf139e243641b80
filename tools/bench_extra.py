#!/usr/bin/env python
"""Secondary measurements (BASELINE configs 3 and 4 and the other estimators) on one MI355X.

Not the headline bench (bench.py); prints one JSON line per workload with the same roofline convention:
algorithmic bytes per cell / kernel time from HIP events on the engine's stream.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scikit-downscale_amd"))
from skdownscale_amd import _lib, synth  # noqa: E402
from skdownscale_amd.engine import Context  # noqa: E402


def regrid_case(T, Ny, Nx, ny=16, nx=25):
    """a coarse [T, ny, nx] temperature field (descending latitude, like gridMET) and a fine grid inside its hull"""
    rng = np.random.default_rng(24)
    sy, sx = np.linspace(50.0, 30.0, ny), np.linspace(-125.0, -100.0, nx)
    dy, dx = np.linspace(49.9, 30.1, Ny), np.linspace(-124.9, -100.1, Nx)
    season = 10.0 * np.sin(2.0 * np.pi * np.arange(T) / 365.25)
    return 285.0 + season[:, None, None] + 3.0 * rng.normal(size=(T, ny, nx)), sy, sx, dy, dx


def device_fill_ms(nbytes, dptr, repeats):
    """median HIP-event time of hipMemsetAsync over nbytes of device memory: the rate a plain fill of the output buffer reaches"""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    ms, times = ctypes.c_float(), []
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    for _ in range(repeats + 1):  # (the first one warms up)
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemsetAsync(ctypes.c_void_p(dptr), 0, ctypes.c_size_t(nbytes), None) == 0
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1) == 0
        times.append(ms.value)
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
    return float(np.median(times[1:]))


def bench_regrid(ctx, args):
    """regrid_kernel: a 16 x 25 coarse field onto 250 x 400 cells, float64 and float32 sources; GB/s by algorithmic bytes
    (8 * T * C written + the source read once), beside a plain device fill of the same output buffer, parity against the oracle on the
    first 256 cells"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _regrid_oracle as ro

    T, Ny, Nx = args.times, 250, 400
    C = Ny * Nx
    src, sy, sx, dy, dx = regrid_case(T, Ny, Nx)
    state = ctx.regrid_create(sy, sx, dy, dx)
    out = ctx.empty((T, C))
    repeats = max(args.steps, 5)
    res = {"workload": f"regrid 16x25 -> {Ny}x{Nx} ({C} cells) x {T} steps, bilinear", "repeats": repeats}
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        host = src.astype(dtype)
        d = ctx.to_device(host, dtype)
        state.apply(d, out=out)
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            state.apply(d, out=out)
            times.append(ctx.prof()["regrid_kernel"]["ms"])
        ctx.prof_enable(False)
        ms = float(np.median(times))
        nbytes = 8 * T * C + host.nbytes
        want = ro.regrid(host, sy, sx, dy[:1], dx[:256]).reshape(T, 256)
        got = out.cells(0, 256).to_host()
        err = float(np.abs(got - want).max() / np.abs(host).max())
        res[name] = {"kernel_ms": ms, "kernel_ms_min_max": [min(times), max(times)], "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                     "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "max_err_over_max_src_first_256_cells": err,
                     "bit_identical_to_oracle": bool(np.array_equal(got, want))}
        d.free()
    fill_ms = device_fill_ms(8 * T * C, out.ptr, repeats)
    res["device_fill"] = {"ms": fill_ms, "bytes": 8 * T * C, "GBps": 8 * T * C / fill_ms / 1e6}
    res["kernel_over_fill"] = {k: res[k]["kernel_ms"] / fill_ms for k in ("f64", "f32")}
    return res


def bench_regrid_e2e(ctx, args):
    """PointWiseDownscaler(BcsdTemperature()) fit + predict from host data, twice in this process: X_hist / X_fut as materialised fine
    host grids, and as coarse.interp_like(obs) (the fine X is produced in HBM); cells/s of both legs, outputs compared bit for bit"""
    import pandas as pd

    from skdownscale_amd import BcsdTemperature, GridArray, PointWiseDownscaler

    T, Nx = args.times, 400
    Ny = max(1, args.cells // Nx)
    C = Ny * Nx
    hist, sy, sx, dy, dx = regrid_case(T, Ny, Nx)
    time_index = pd.date_range("1980-01-01", periods=T, freq="D")
    rng = np.random.default_rng(25)
    coords = dict(time=time_index, lat=sy, lon=sx)
    fine = dict(time=time_index, lat=dy, lon=dx)
    coarse = {"hist": GridArray(hist, ("time", "lat", "lon"), coords), "fut": GridArray(hist + 1.5 + rng.normal(size=hist.shape), ("time", "lat", "lon"), coords)}
    obs = GridArray(hist.mean(axis=(1, 2))[:, None, None] - 2.0 + 2.0 * rng.normal(size=(T, Ny, Nx)), ("time", "lat", "lon"), fine)
    legs = {"interpolated": {k: v.interp_like(obs) for k, v in coarse.items()},
            "materialised": {k: GridArray(v.interp_like(obs).values, ("time", "lat", "lon"), fine) for k, v in coarse.items()}}

    def run(X):
        model = PointWiseDownscaler(BcsdTemperature())
        model.fit(X["hist"], obs)
        return np.asarray(model.predict(X["fut"]).values)

    run(legs["materialised"])  # warm-up: code objects, pinned rings, the block cache
    res = {"workload": f"PointWiseDownscaler(BcsdTemperature) fit + predict from host data, 16x25 -> {Ny}x{Nx} ({C} cells) x {T} steps", "repeats": args.steps}
    outs = {}
    for _ in range(args.steps):  # the two legs alternate
        for name, X in legs.items():
            t0 = time.perf_counter()
            outs[name] = run(X)
            res.setdefault(name, []).append(time.perf_counter() - t0)
    for name in legs:
        s = float(np.median(res[name]))
        res[name] = {"seconds": s, "cells_per_s": C / s}
    res["speedup"] = res["materialised"]["seconds"] / res["interpolated"]["seconds"]
    res["bit_identical"] = bool(np.array_equal(outs["interpolated"], outs["materialised"], equal_nan=True))
    res["fine_X_reached_the_host"] = any(v.computed for v in legs["interpolated"].values())
    return res


def device_copy_ms(ctx, dst, src, nbytes, repeats):
    """median HIP-event time of sd_memcpy_d2d over nbytes on the engine's stream: the rate a plain device copy of the source reaches"""
    times = []
    for _ in range(repeats + 1):  # (the first one warms up)
        ctx.timer_start()
        _lib.check(ctx.lib.sd_memcpy_d2d(ctx.handle, dst.vptr, src.vptr, nbytes))
        times.append(ctx.timer_stop())
    return float(np.median(times[1:])), [min(times[1:]), max(times[1:])]


def bench_resample(ctx, args):
    """resample_kernel: daily steps to 'MS' bins (14 600 -> 480) on 100 000 cells, float64 and float32 sources, mean; GB/s by algorithmic
    bytes (the source read once + 8 * M * C written), beside sd_memcpy_d2d of the same source bytes in the same run, parity against the
    oracle on the first 256 cells"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _resample_oracle as so
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    labels, offsets = time_bins(index, "MS")
    M = len(labels)
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    d64, first = fill(C), fill(256).to_host()
    out, spare = ctx.empty((M, C)), ctx.empty((T, C))
    repeats = max(args.steps, 5)
    res = {"workload": f"resample {T} daily steps -> {M} 'MS' bins x {C} cells, mean", "repeats": repeats}
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        if dtype == np.float32:
            d = ctx.empty((T, C), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, d64.vptr, T * C, d.vptr))
            ctx.synchronize()
        else:
            d = d64
        host = first.astype(dtype)
        ctx.resample(d, offsets, "mean", out=out)
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            ctx.resample(d, offsets, "mean", out=out)
            times.append(ctx.prof()["resample_kernel"]["ms"])
        ctx.prof_enable(False)
        ms = float(np.median(times))
        src_bytes = T * C * np.dtype(dtype).itemsize
        nbytes = src_bytes + 8 * M * C
        got, want = out.cells(0, 256).to_host(), so.resample(host, offsets, "mean")
        with contextlib.redirect_stdout(sys.stderr):  # (the check prints its figure; stdout carries the JSON line alone)
            ratio = so.check(got, want, host, offsets, "mean", f"bench {name}")
        copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
        res[name] = {"kernel_ms": ms, "kernel_ms_min_max": [min(times), max(times)], "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                     "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "max_err_over_bound_first_256_cells": ratio, "parity": bool(ratio <= 1.0),
                     "bit_identical_to_oracle": bool(np.array_equal(got, want, equal_nan=True)),
                     "device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6},
                     "kernel_over_copy_ms": ms / copy_ms, "GBps_over_copy_GBps": (nbytes / ms) / (src_bytes / copy_ms)}
        if d is not d64:
            d.free()
    return res


def bench_disagg(ctx, args):
    """disagg_kernel: the monthly means of a 40-year daily record (480 months) back to daily rows on 100 000 cells, every month borrowing
    a seeded year of the record, shift, float64 and float32 observations; GB/s by algorithmic bytes (the borrowed rows read once + 8 * M
    * C read + 8 * Tout * C written), beside sd_memcpy_d2d of the same source bytes in the same run, the first 256 cells compared bit
    for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _disagg_oracle as do
    import pandas as pd
    from skdownscale_amd.disagg import time_map
    from skdownscale_amd.resample import time_bins

    years, C = max(1, round(args.times / 365)), 100_000
    index = pd.date_range("1980-01-01", f"{1980 + years - 1}-12-31", freq="D")
    To = len(index)
    months = pd.date_range("2020-01-01", periods=12 * years, freq="MS")
    _, src_row, offsets = time_map(months, index, None, 0)
    Tout, M = len(src_row), len(months)
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((To, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    d64, first = fill(C), fill(256).to_host()
    target = ctx.resample(d64, time_bins(index, "MS")[1], "mean")  # month k of the output is brought to the mean of month k of the record
    t_first = target.cells(0, 256).to_host()
    out, spare = ctx.empty((Tout, C)), ctx.empty((Tout, C))
    repeats = max(args.steps, 7)
    res = {"workload": f"disagg {M} months -> {Tout} daily rows x {C} cells on a {To}-day record, shift, seeded years", "repeats": repeats}
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        if dtype == np.float32:
            d = ctx.empty((To, C), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, d64.vptr, To * C, d.vptr))
            ctx.synchronize()
        else:
            d = d64
        ctx.disaggregate(target, d, src_row, offsets, "shift", out=out)
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            ctx.disaggregate(target, d, src_row, offsets, "shift", out=out)
            times.append(ctx.prof()["disagg_kernel"]["ms"])
        ctx.prof_enable(False)
        ms = float(np.median(times))
        src_bytes = Tout * C * np.dtype(dtype).itemsize
        nbytes = src_bytes + 8 * Tout * C + 8 * M * C
        got, want = out.cells(0, 256).to_host(), do.disaggregate(t_first, first.astype(dtype), src_row, offsets, "shift")
        copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
        res[name] = {"kernel_ms": ms, "kernel_ms_min_max": [min(times), max(times)], "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                     "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": bool(np.array_equal(got, want, equal_nan=True)),
                     "device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6},
                     "kernel_over_copy_ms": ms / copy_ms, "GBps_over_copy_GBps": (nbytes / ms) / (src_bytes / copy_ms)}
        if d is not d64:
            d.free()
    return res


def bench_groupby(ctx, args):
    """groupby_reduce_kernel by month (G = 12) and by day of year (G = 366, mean) and groupby_apply_kernel (SUB of the monthly
    climatology) on 14 600 daily steps x 100 000 cells, float64 and float32 sources, each timed through ctx.prof() beside sd_memcpy_d2d
    of the same source bytes and beside resample_kernel ('MS', mean) on the same field in the same run; GB/s by algorithmic bytes
    (reduce: the source read once + 12 * G * C accumulators + 8 * G * C written; apply: the source + 8 * G * C read, 8 * T * C written);
    the first 256 cells compared bit for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _groupby_oracle as go
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    _, offsets = time_bins(index, "MS")
    groups = {"month": (np.asarray(index.month) - 1).astype(np.int32), "dayofyear": (np.asarray(index.dayofyear) - 1).astype(np.int32)}
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(kernel, call, repeats):
        call()
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            times.append(ctx.prof()[kernel]["ms"])
        ctx.prof_enable(False)
        return float(np.median(times)), [min(times), max(times)]

    d64, first = fill(C), fill(256).to_host()
    spare, monthly = ctx.empty((T, C)), ctx.empty((len(offsets) - 1, C))
    repeats = max(args.steps, 5)
    res = {"workload": f"groupby {T} daily steps x {C} cells: mean by month (G=12) and by day of year (G=366), minus the monthly climatology",
           "repeats": repeats, "bins_per_wave": {"G=12": 1, "G=366": 2}}
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        if dtype == np.float32:
            d = ctx.empty((T, C), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, d64.vptr, T * C, d.vptr))
            ctx.synchronize()
        else:
            d = d64
        host = first.astype(dtype)
        src_bytes = T * C * np.dtype(dtype).itemsize
        copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
        rs_ms, rs_min_max = timed("resample_kernel", lambda: ctx.resample(d, offsets, "mean", out=monthly), repeats)
        leg = {"device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6},
               "resample_kernel_MS_mean": {"kernel_ms": rs_ms, "kernel_ms_min_max": rs_min_max}}
        clim = None
        for key, group in groups.items():
            G = int(group.max()) + 1
            out = ctx.empty((G, C))

            def reduce():
                for a in ctx.groupby_reduce(d, group, G, "mean", out=out)[1]:
                    a.free()

            ms, min_max = timed("groupby_reduce_kernel", reduce, repeats)
            nbytes = src_bytes + 12 * G * C + 8 * G * C
            same = bool(np.array_equal(out.cells(0, 256).to_host(), go.reduce(host, group, G, "mean"), equal_nan=True))
            leg[f"reduce_{key}"] = {"G": G, "kernel_ms": ms, "kernel_ms_min_max": min_max, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                                    "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": same,
                                    "kernel_over_copy_ms": ms / copy_ms, "kernel_over_resample_ms": ms / rs_ms}
            if key == "month":
                clim = out
            else:
                out.free()
        ms, min_max = timed("groupby_apply_kernel", lambda: ctx.groupby_apply(d, groups["month"], clim, "sub", out=spare), repeats)
        nbytes = src_bytes + 8 * 12 * C + 8 * T * C
        same = bool(np.array_equal(spare.cells(0, 256).to_host(), go.apply(host, groups["month"], clim.cells(0, 256).to_host(), "sub"), equal_nan=True))
        leg["apply_sub_month"] = {"G": 12, "kernel_ms": ms, "kernel_ms_min_max": min_max, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                                  "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": same,
                                  "kernel_over_copy_ms": ms / copy_ms, "kernel_over_resample_ms": ms / rs_ms}
        clim.free()
        res[name] = leg
        if d is not d64:
            d.free()
    return res


def bench_rolling(ctx, args):
    """rolling_kernel on 14 600 daily steps x 100 000 cells, float64 and float32 sources: centred mean at w = 9 and w = 31, centred std at
    w = 31 (staged in LDS) and a centred mean at w = 91 (too long for the LDS budget: rolling_unstaged_kernel), each the median of 7
    HIP-event times through ctx.prof() beside sd_memcpy_d2d of the same source bytes and beside groupby_apply_kernel (SUB of the monthly
    climatology: the same traffic, source read once and T * C doubles written) on the same field in the same run; GB/s by algorithmic
    bytes (the source read once + 8 * T * C written); the first 256 cells compared bit for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _rolling_oracle as ro

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    month = (np.asarray(index.month) - 1).astype(np.int32)
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(kernel, call, repeats):
        call()
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            times.append(ctx.prof()[kernel]["ms"])
        ctx.prof_enable(False)
        return float(np.median(times)), [min(times), max(times)]

    d64, first = fill(C), fill(256).to_host()
    spare = ctx.empty((T, C))
    repeats = max(args.steps, 7)
    cases = (("mean_w9", 9, "mean", "rolling_kernel"), ("mean_w31", 31, "mean", "rolling_kernel"), ("std_w31", 31, "std", "rolling_kernel"),
             ("mean_w91_unstaged", 91, "mean", "rolling_unstaged_kernel"))
    res = {"workload": f"rolling {T} daily steps x {C} cells, centred windows: mean w=9, mean w=31, std w=31 (staged), mean w=91 (unstaged)",
           "repeats": repeats}
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        if dtype == np.float32:
            d = ctx.empty((T, C), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, d64.vptr, T * C, d.vptr))
            ctx.synchronize()
        else:
            d = d64
        host = first.astype(dtype)
        src_bytes = T * C * np.dtype(dtype).itemsize
        nbytes = src_bytes + 8 * T * C
        copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
        clim, acc = ctx.groupby_reduce(d, month, 12, "mean")
        for a in acc:
            a.free()
        ap_ms, ap_min_max = timed("groupby_apply_kernel", lambda: ctx.groupby_apply(d, month, clim, "sub", out=spare), repeats)
        clim.free()
        leg = {"device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6},
               "groupby_apply_kernel_sub_month": {"kernel_ms": ap_ms, "kernel_ms_min_max": ap_min_max, "GBps": (nbytes + 8 * 12 * C) / ap_ms / 1e6}}
        for key, w, op, kernel in cases:
            back = w // 2
            ms, min_max = timed(kernel, lambda: ctx.rolling(d, w, op, back, 1, out=spare), repeats)
            same = bool(np.array_equal(spare.cells(0, 256).to_host(), ro.finish(ro.moments(host, w, back), op, 1, 1), equal_nan=True))
            leg[key] = {"window": w, "op": op, "kernel": kernel, "kernel_ms": ms, "kernel_ms_min_max": min_max, "algorithmic_bytes": nbytes,
                        "GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": same,
                        "kernel_over_copy_ms": ms / copy_ms, "kernel_over_apply_ms": ms / ap_ms}
        res[name] = leg
        if d is not d64:
            d.free()
    return res


def bench_quantile(ctx, args):
    """the quantile kernels on 14 600 daily steps x 100 000 cells float64: by month (G = 12) with q = [0.05, 0.5, 0.95] -- the segment path
    at its widest width -- and the whole axis with q = 0.5 -- the series path --, each kernel timed through ctx.prof() beside
    sd_memcpy_d2d of the same source bytes, beside groupby_reduce_kernel (mean by month) and beside the kernels of a BcsdPrecipitation
    fit of the same field (sd_bcsd_fit_dev, SD_BCSD_PR: the same twelve sorts per cell) in the same run; GB/s by algorithmic bytes (8 * T
    * C read + 8 * Q * G * C written); the first 256 cells compared bit for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _quantile_oracle as qo

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    month = (np.asarray(index.month) - 1).astype(np.int32)
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(call, repeats):
        """per kernel: (median ms, [min, max]) of ``repeats`` profiled calls after one warm-up"""
        call()
        ctx.prof_enable(True)
        seen = {}
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            for name, v in ctx.prof().items():
                seen.setdefault(name, []).append(v["ms"])
        ctx.prof_enable(False)
        return {name: {"kernel_ms": float(np.median(v)), "kernel_ms_min_max": [min(v), max(v)]} for name, v in seen.items()}

    d, first = fill(C), fill(256).to_host()
    spare = ctx.empty((T, C))
    repeats = max(args.steps, 5)
    src_bytes = 8 * T * C
    copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
    spare.free()
    res = {"workload": f"quantile {T} daily steps x {C} cells float64: q = [0.05, 0.5, 0.95] by month (G=12), and q = 0.5 of the whole axis",
           "repeats": repeats, "device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6}}
    mean = ctx.empty((12, C))

    def reduce():
        for a in ctx.groupby_reduce(d, month, 12, "mean", out=mean)[1]:
            a.free()

    res["groupby_reduce_kernel_month_mean"] = timed(reduce, repeats)["groupby_reduce_kernel"]
    mean.free()

    def fit():
        ctx.bcsd_fit(_lib.BCSD_PR, None, d, month, 12, True).close()

    kernels = timed(fit, repeats)
    res["bcsd_pr_fit"] = {"kernels": kernels, "kernel_ms": sum(k["kernel_ms"] for k in kernels.values())}
    for name, q, group, G in (("by_month", [0.05, 0.5, 0.95], month, 12), ("whole_axis", [0.5], None, 1)):
        out = ctx.empty((len(q) * G, C))
        kernels = timed(lambda: ctx.quantile(d, q, group, G, out=out), repeats)
        ms = sum(k["kernel_ms"] for k in kernels.values())
        nbytes = src_bytes + 8 * len(q) * G * C
        same = qo.same(out.cells(0, 256).to_host(), qo.quantile_field(first, q, group, G))
        res[name] = {"G": G, "q": q, "kernels": kernels, "kernel_ms": ms, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                     "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": bool(same),
                     "kernel_over_copy_ms": ms / copy_ms, "kernel_over_groupby_reduce_ms": ms / res["groupby_reduce_kernel_month_mean"]["kernel_ms"],
                     "kernel_over_bcsd_pr_fit_ms": ms / res["bcsd_pr_fit"]["kernel_ms"]}
        out.free()
    return res


def bench_remap(ctx, args):
    """remap_kernel alone (ctx.prof(): an event pair around the launch): 14 600 daily steps of a 250 x 400 fine field onto 16 x 25
    coarse cells by area overlap (latitude in sin(lat); 250 / 16 is not an integer, so target rows share source rows), float64 and
    float32 sources, beside sd_memcpy_d2d of the same source bytes and beside resample_kernel ('MS', mean) on the same field in the
    same run.  GB/s by algorithmic bytes (the source read once + 8 * T * Ny * Nx written); the first two and the last time step
    compared bit for bit with the oracle.  -> one result per source type"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _remap_oracle as mo
    from skdownscale_amd.resample import time_bins

    T, (ny, nx), (Ny, Nx) = args.times, (250, 400), (16, 25)
    C = ny * nx
    index = synth.daily_calendar(T)
    _, offsets = time_bins(index, "MS")
    tab = synth.tas_tables(index)["y_obs"]
    d64 = ctx.synth_fill(ctx.empty((T, C)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])
    syb, sxb = np.sin(np.deg2rad(np.linspace(30.0, 50.0, ny + 1))), np.linspace(-120.0, -100.0, nx + 1)
    dyb, dxb = np.sin(np.deg2rad(np.linspace(30.0, 50.0, Ny + 1))), np.linspace(-120.0, -100.0, Nx + 1)
    state = ctx.remap_create(syb, sxb, dyb, dxb)
    spare, monthly, out = ctx.empty((T, C)), ctx.empty((len(offsets) - 1, C)), ctx.empty((T, Ny * Nx))
    repeats = max(args.steps, 5)
    picks = [0, 1, T - 1]

    def timed(kernel, call):
        call()
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            times.append(ctx.prof()[kernel]["ms"])
        ctx.prof_enable(False)
        return float(np.median(times)), [min(times), max(times)]

    results = []
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        if dtype == np.float32:
            d = ctx.empty((T, C), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, d64.vptr, T * C, d.vptr))
            ctx.synchronize()
        else:
            d = d64
        src_bytes = T * C * np.dtype(dtype).itemsize
        copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
        rs_ms, rs_min_max = timed("resample_kernel", lambda: ctx.resample(d, offsets, "mean", out=monthly))
        ms, min_max = timed("remap_kernel", lambda: state.apply(d, 0.5, out=out))
        host = np.stack([d.rows(t, t + 1).to_host()[0] for t in picks]).reshape(len(picks), ny, nx)
        got = np.stack([out.rows(t, t + 1).to_host()[0] for t in picks])
        same = bool(np.array_equal(got, mo.remap(host, syb, sxb, dyb, dxb, 0.5).reshape(len(picks), -1), equal_nan=True))
        nbytes = src_bytes + 8 * T * Ny * Nx
        results.append({"workload": f"remap {T} daily steps of {ny}x{nx} -> {Ny}x{Nx} by area overlap, min_valid=0.5, {name} source", "repeats": repeats,
                        "source": name, "kernel_ms": ms, "kernel_ms_min_max": min_max, "algorithmic_bytes": nbytes, "read_GBps": src_bytes / ms / 1e6,
                        "GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_steps_0_1_last": same,
                        "device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6},
                        "resample_kernel_MS_mean": {"kernel_ms": rs_ms, "kernel_ms_min_max": rs_min_max, "read_GBps": src_bytes / rs_ms / 1e6},
                        "read_rate_over_copy": copy_ms / ms, "read_rate_over_resample": rs_ms / ms})
        if d is not d64:
            d.free()
    return results


def bench_spells(ctx, args):
    """spells_kernel on 14 600 daily steps x 100 000 cells float64 with 'YS' bins: a scalar threshold with one statistic, and a [366, C]
    day-of-year table (the day-of-year means of the field) with three statistics (fraction, spell_days at min_length 6, count), each
    timed through ctx.prof() -- median and [min, max] of 7 profiled calls after a warm-up -- beside sd_memcpy_d2d of the same source
    bytes, resample_kernel (mean over the same bins) and groupby_apply_kernel (minus the same table) in the same run; GB/s by algorithmic bytes (8 * T * C read, + 8 * T * C
    of table rows for the table case, + 8 * nstat * M * C written) and, for the table case, by distinct bytes too (the table once, 8 * 366 * C:
    each of its rows is read again in every year, which the caches can serve); the first 256 cells compared bit for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _spells_oracle as sp
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    labels, offsets = time_bins(index, "YS")
    M = len(labels)
    doy = (np.asarray(index.dayofyear) - 1).astype(np.int32)
    tab = synth.tas_tables(index)["y_obs"]

    def fill(cells):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(call, kernel, repeats):
        call()
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            times.append(ctx.prof()[kernel]["ms"])
        ctx.prof_enable(False)
        return {"kernel_ms": float(np.median(times)), "kernel_ms_min_max": [min(times), max(times)]}

    d, first = fill(C), fill(256).to_host()
    repeats = 7
    src_bytes = 8 * T * C
    spare = ctx.empty((T, C))
    copy_ms, copy_min_max = device_copy_ms(ctx, spare, d, src_bytes, repeats)
    spare.free()
    res = {"workload": f"spells {T} daily steps -> {M} 'YS' bins x {C} cells float64: scalar threshold, 1 statistic; [366, C] day-of-year table, 3 statistics",
           "repeats": repeats, "device_copy": {"ms": copy_ms, "ms_min_max": copy_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6}}
    mean = ctx.empty((M, C))
    res["resample_kernel_mean"] = timed(lambda: ctx.resample(d, offsets, "mean", out=mean), "resample_kernel", repeats)
    res["resample_kernel_mean"]["algorithmic_bytes"] = src_bytes + 8 * M * C
    mean.free()
    clim, acc = ctx.groupby_reduce(d, doy, 366, "mean")
    for a in acc:
        a.free()
    anom = ctx.empty((T, C))  # the yardstick of the table case: groupby_apply_kernel reads the same source and table rows (and writes 8 * T * C)
    res["groupby_apply_kernel_sub_doy"] = timed(lambda: ctx.groupby_apply(d, doy, clim, "sub", out=anom), "groupby_apply_kernel", repeats)
    res["groupby_apply_kernel_sub_doy"]["algorithmic_bytes"] = 3 * src_bytes + 8 * 366 * C
    anom.free()
    threshold = float(np.nanmean(first))
    cases = (("scalar_1_statistic", ">", threshold, None, ["longest_spell"], 1, 0, 0),
             ("doy_table_3_statistics", ">", clim, doy, ["fraction", "spell_days", "count"], 6, 8 * T * C, 8 * 366 * C))
    for name, op, thr, group, stats, L, table_bytes, table_distinct in cases:
        out = ctx.empty((len(stats) * M, C))
        r = timed(lambda: ctx.spells(d, op, thr, offsets, stats, L, group, out=out), "spells_kernel", repeats)
        ms = r["kernel_ms"]
        nbytes = src_bytes + table_bytes + 8 * len(stats) * M * C
        host_thr = thr if group is None else thr.cells(0, 256).to_host()
        got, want = out.cells(0, 256).to_host(), sp.spells(first, offsets, op, host_thr, stats, L, group)
        distinct = src_bytes + table_distinct + 8 * len(stats) * M * C
        r.update({"op": op, "statistics": stats, "min_length": L, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                  "distinct_bytes": distinct, "GBps_of_distinct_bytes": distinct / ms / 1e6,
                  "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": bool(np.array_equal(got, want, equal_nan=True)),
                  "kernel_over_copy_ms": ms / copy_ms, "kernel_over_resample_ms": ms / res["resample_kernel_mean"]["kernel_ms"],
                  "kernel_over_groupby_apply_ms": ms / res["groupby_apply_kernel_sub_doy"]["kernel_ms"]})
        res[name] = r
        out.free()
    return res


def bench_skill(ctx, args):
    """skill_kernel on 14 600 daily steps x 100 000 cells, float64 against float64 (a synthetic downscaled field against synthetic
    observations), with one whole-axis bin and with 'YS' bins: ["bias", "rmse"] (one pass over both fields) and ["bias", "rmse", "corr"]
    (two passes), each timed through ctx.prof() -- median and [min, max] of 7 profiled calls after a warm-up -- beside sd_memcpy_d2d of
    the same source bytes (both fields) and beside spells_kernel (one statistic of a scalar threshold over the same bins of one field)
    in the same run; GB/s by algorithmic bytes (16 * T * C read per pass + 8 * nstat * M * C written); the first 256 cells compared bit
    for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _skill_oracle as sk
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    labels, yearly = time_bins(index, "YS")
    tabs = synth.tas_tables(index)

    def fill(cells, tab):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(call, kernel, repeats):
        call()
        ctx.prof_enable(True)
        times = []
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            times.append(ctx.prof()[kernel]["ms"])
        ctx.prof_enable(False)
        return {"kernel_ms": float(np.median(times)), "kernel_ms_min_max": [min(times), max(times)]}

    a, b = fill(C, tabs["X_hist"]), fill(C, tabs["y_obs"])
    first_a, first_b = fill(256, tabs["X_hist"]).to_host(), fill(256, tabs["y_obs"]).to_host()
    repeats = 7
    src_bytes = 2 * 8 * T * C
    spare = ctx.empty((T, C))
    one_ms, one_min_max = device_copy_ms(ctx, spare, a, src_bytes // 2, repeats)  # (two copies of one field's bytes: the same bytes moved)
    spare.free()
    copy_ms = 2 * one_ms
    res = {"workload": f"skill {T} daily steps x {C} cells float64 against float64: one whole-axis bin and {len(labels)} 'YS' bins; bias, rmse (one pass) and bias, rmse, corr (two passes)",
           "repeats": repeats, "device_copy": {"ms": copy_ms, "ms_of_one_field_min_max": one_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6}}
    for bins_name, offsets in (("whole_axis", np.array([0, T], dtype=np.int64)), ("YS", np.asarray(yearly, dtype=np.int64))):
        M = len(offsets) - 1
        count = ctx.empty((M, C))
        sp_r = timed(lambda: ctx.spells(b, ">", 13.0, offsets, ["count"], out=count), "spells_kernel", repeats)
        sp_r["algorithmic_bytes"] = 8 * T * C + 8 * M * C
        sp_r["GBps"] = sp_r["algorithmic_bytes"] / sp_r["kernel_ms"] / 1e6
        count.free()
        res[f"{bins_name}_spells_kernel_count"] = sp_r
        for stats, passes in ((["bias", "rmse"], 1), (["bias", "rmse", "corr"], 2)):
            out = ctx.empty((len(stats) * M, C))
            r = timed(lambda: ctx.skill(a, b, offsets, stats, out=out), "skill_kernel", repeats)
            ms = r["kernel_ms"]
            nbytes = passes * src_bytes + 8 * len(stats) * M * C
            got, want = out.cells(0, 256).to_host(), sk.skill(first_a, first_b, offsets, stats)
            r.update({"statistics": stats, "passes": passes, "bins": M, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                      "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": bool(np.array_equal(got, want, equal_nan=True)),
                      "kernel_over_copy_ms": ms / copy_ms, "read_rate_over_copy": (passes * src_bytes / ms) / (src_bytes / copy_ms),
                      "read_rate_over_spells": (passes * src_bytes / ms) / (8 * T * C / sp_r["kernel_ms"])})
            res[f"{bins_name}_{'_'.join(stats)}"] = r
            out.free()
    return res


def bench_twosample(ctx, args):
    """the two-sample kernels on 14 600 daily steps x 100 000 cells, float64 against float64 (the fields of the skill workload): 'YS'
    bins -- the segment path -- and one whole-axis bin -- the series path --, ["ks", "perkins"] from one call, timed through ctx.prof()
    (the sum over the kernels of a call; median and [min, max] of 7 profiled calls after a warm-up) beside sd_memcpy_d2d of the same source
    bytes (both fields), beside skill_kernel (bias, rmse) over the same bins, and beside two sd_quantile_dev calls with Q = 1 on the two
    fields over the same groups: the same gathers and sorts with a quantile evaluation as the last step.  GB/s by algorithmic bytes
    (16 * T * C read + 8 * nstat * M * C written); the first 64 cells compared bit for bit with the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _twosample_oracle as ts
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    labels, yearly = time_bins(index, "YS")
    tabs = synth.tas_tables(index)

    def fill(cells, tab):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(call, repeats):
        call()
        ctx.prof_enable(True)
        times, kernels = [], {}
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            prof = ctx.prof()
            times.append(sum(v["ms"] for v in prof.values()))
            for k, v in prof.items():
                kernels.setdefault(k, []).append(v["ms"])
        ctx.prof_enable(False)
        return {"kernel_ms": float(np.median(times)), "kernel_ms_min_max": [min(times), max(times)],
                "kernels_ms": {k: float(np.median(v)) for k, v in kernels.items()}}

    a, b = fill(C, tabs["X_hist"]), fill(C, tabs["y_obs"])
    first_a, first_b = fill(64, tabs["X_hist"]).to_host(), fill(64, tabs["y_obs"]).to_host()
    repeats = 7
    src_bytes = 2 * 8 * T * C
    spare = ctx.empty((T, C))
    one_ms, one_min_max = device_copy_ms(ctx, spare, a, src_bytes // 2, repeats)  # (two copies of one field's bytes: the same bytes moved)
    spare.free()
    copy_ms = 2 * one_ms
    stats, width, origin = ["ks", "perkins"], 1.0, 0.0
    res = {"workload": f"twosample {T} daily steps x {C} cells float64 against float64: {len(labels)} 'YS' bins (segment path) and one whole-axis bin (series path); ks, perkins(width=1)",
           "repeats": repeats, "device_copy": {"ms": copy_ms, "ms_of_one_field_min_max": one_min_max, "bytes": src_bytes, "GBps_of_bytes_copied": src_bytes / copy_ms / 1e6}}
    year = (np.searchsorted(np.asarray(yearly), np.arange(T), side="right") - 1).astype(np.int32)
    for bins_name, offsets, group in (("YS", np.asarray(yearly, dtype=np.int64), year), ("whole_axis", np.array([0, T], dtype=np.int64), None)):
        M = len(offsets) - 1
        two = ctx.empty((2 * M, C))
        sk_r = timed(lambda: ctx.skill(a, b, offsets, ["bias", "rmse"], out=two), repeats)
        res[f"{bins_name}_skill_kernel_bias_rmse"] = sk_r
        med = ctx.empty((M, C))
        q_a = timed(lambda: ctx.quantile(a, [0.5], group, None if group is None else M, out=med), repeats)
        q_b = timed(lambda: ctx.quantile(b, [0.5], group, None if group is None else M, out=med), repeats)
        med.free()
        res[f"{bins_name}_quantile_q1_a"], res[f"{bins_name}_quantile_q1_b"] = q_a, q_b
        quantile_ms = q_a["kernel_ms"] + q_b["kernel_ms"]
        r = timed(lambda: ctx.twosample(a, b, offsets, stats, width, origin, out=two), repeats)
        ms = r["kernel_ms"]
        nbytes = src_bytes + 8 * len(stats) * M * C
        got, want = two.cells(0, 64).to_host(), ts.twosample(first_a, first_b, offsets, stats, width, origin)
        r.update({"statistics": stats, "bins": M, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0,
                  "bit_identical_to_oracle_first_64_cells": bool(np.array_equal(got, want, equal_nan=True)), "kernel_over_copy_ms": ms / copy_ms,
                  "kernel_over_skill_ms": ms / sk_r["kernel_ms"], "two_quantile_calls_ms": quantile_ms, "kernel_over_two_quantile_calls": ms / quantile_ms})
        res[f"{bins_name}_ks_perkins"] = r
        ks_only = timed(lambda: ctx.twosample(a, b, offsets, ["ks"], out=two.rows(0, M)), repeats)
        ks_only["kernel_over_two_quantile_calls"] = ks_only["kernel_ms"] / quantile_ms
        res[f"{bins_name}_ks"] = ks_only
        two.free()
    return res


def bench_skill_groups(ctx, args):
    """compare(...).groupby(...) on the fields of the skill workload (14 600 daily steps x 100 000 cells, float64 against float64):
    skill_groups_kernel for ["bias", "rmse"] (one pass) and ["bias", "rmse", "corr"] (two passes) by month (12 groups), by season (4)
    and by day of year (366), each beside skill_kernel over the 40 'YS' bins with the same statistics in the same run (the same bytes
    of both fields; GB/s by algorithmic bytes: 16 * T * C read per pass + 8 * T of row table per tile of cells + 8 * nstat * G * C
    written); then sd_twosample_groups for ["ks"] and ["ks", "perkins"] (width 1) by month (the series path) and by day of year (the
    segment path), beside two sd_quantile_dev(by=) calls with Q = 1 on the two fields over the same groups.  Timed through ctx.prof()
    (the sum over the kernels of a call; median and [min, max] of 7 profiled calls after a warm-up); the first 256 (paired) and 64
    (two-sample) cells compared bit for bit with the grouped oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _grouped_pair_oracle as gp
    from skdownscale_amd.groupby import group_labels
    from skdownscale_amd.resample import time_bins

    T, C = args.times, 100_000
    index = synth.daily_calendar(T)
    labels, yearly = time_bins(index, "YS")
    yearly = np.asarray(yearly, dtype=np.int64)
    tabs = synth.tas_tables(index)

    def fill(cells, tab):  # (a cell shard of the synthetic field holds the same values as those cells of the whole field)
        return ctx.synth_fill(ctx.empty((T, cells)), synth.GAUSS, 0, tab["stream"], c_full=C, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])

    def timed(call, repeats):
        call()
        ctx.prof_enable(True)
        times, kernels = [], {}
        for _ in range(repeats):
            ctx.prof_reset()
            call()
            prof = ctx.prof()
            times.append(sum(v["ms"] for v in prof.values()))
            for k, v in prof.items():
                kernels.setdefault(k, []).append(v["ms"])
        ctx.prof_enable(False)
        return {"kernel_ms": float(np.median(times)), "kernel_ms_min_max": [min(times), max(times)],
                "kernels_ms": {k: float(np.median(v)) for k, v in kernels.items()}}

    def ids_of(field):
        found, ids = np.unique(group_labels(index, field), return_inverse=True)
        return ids.astype(np.int32), len(found)

    a, b = fill(C, tabs["X_hist"]), fill(C, tabs["y_obs"])
    first_a, first_b = fill(256, tabs["X_hist"]).to_host(), fill(256, tabs["y_obs"]).to_host()
    repeats = 7
    src_bytes = 2 * 8 * T * C
    res = {"workload": f"skill_groups {T} daily steps x {C} cells float64 against float64: bias, rmse (one pass) and bias, rmse, corr (two passes) by month, "
                       f"season and day of year beside {len(labels)} 'YS' bins; ks and ks, perkins(width=1) by month and day of year", "repeats": repeats}
    groupings = {name: ids_of(name) for name in ("month", "season", "dayofyear")}
    M = len(yearly) - 1
    for stats, passes in ((["bias", "rmse"], 1), (["bias", "rmse", "corr"], 2)):
        key = "_".join(stats)
        out = ctx.empty((len(stats) * M, C))
        ys = timed(lambda: ctx.skill(a, b, yearly, stats, out=out), repeats)
        out.free()
        ys.update({"statistics": stats, "bins": M, "algorithmic_bytes": passes * src_bytes + 8 * len(stats) * M * C})
        ys["GBps"] = ys["algorithmic_bytes"] / ys["kernel_ms"] / 1e6
        res[f"YS_skill_kernel_{key}"] = ys
        for name, (ids, G) in groupings.items():
            out = ctx.empty((len(stats) * G, C))
            r = timed(lambda: ctx.skill_groups(a, b, ids, G, stats, out=out), repeats)
            ms = r["kernel_ms"]
            ctiles = -(-C // 128)  # two cells per lane
            nbytes = passes * (src_bytes + 8 * T * ctiles) + 8 * len(stats) * G * C
            got, want = out.cells(0, 256).to_host(), gp.skill(first_a, first_b, ids, G, stats)
            r.update({"statistics": stats, "passes": passes, "groups": G, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                      "frac_of_8TBps": nbytes / ms / 1e6 / 8000.0, "bit_identical_to_oracle_first_256_cells": bool(np.array_equal(got, want, equal_nan=True)),
                      "kernel_over_YS_skill_kernel_ms": ms / ys["kernel_ms"]})
            res[f"{name}_{key}"] = r
            out.free()
    width, origin = 1.0, 0.0
    for name in ("month", "dayofyear"):
        ids, G = groupings[name]
        med = ctx.empty((G, C))
        q_a = timed(lambda: ctx.quantile(a, [0.5], ids, G, out=med), repeats)
        q_b = timed(lambda: ctx.quantile(b, [0.5], ids, G, out=med), repeats)
        med.free()
        res[f"{name}_quantile_q1_a"], res[f"{name}_quantile_q1_b"] = q_a, q_b
        quantile_ms = q_a["kernel_ms"] + q_b["kernel_ms"]
        for stats in (["ks"], ["ks", "perkins"]):
            two = ctx.empty((len(stats) * G, C))
            r = timed(lambda: ctx.twosample_groups(a, b, ids, G, stats, width, origin, out=two), repeats)
            ms = r["kernel_ms"]
            nbytes = src_bytes + 8 * len(stats) * G * C
            got, want = two.cells(0, 64).to_host(), gp.twosample(first_a[:, :64], first_b[:, :64], ids, G, stats, width, origin)
            r.update({"statistics": stats, "groups": G, "longest_group": int(np.bincount(ids).max()), "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                      "bit_identical_to_oracle_first_64_cells": bool(np.array_equal(got, want, equal_nan=True)), "two_quantile_calls_ms": quantile_ms,
                      "kernel_over_two_quantile_calls": ms / quantile_ms})
            res[f"{name}_{'_'.join(stats)}"] = r
            two.free()
    return res


def bench_constructed(ctx, args):
    """The three constructed-analog kernels, each alone (ctx.prof(): an event pair around the launch; median and [min, max] of the
    repeats after a warm-up), at Tl = 14 600 library days, Tq = 3 650 targets, Cc = 400 (20 x 20) coarse and Cf = 100 000 fine cells,
    k = 30, window 45, with the fine library as float32 and as float64, beside sd_memcpy_d2d of the output bytes.  ca_select_kernel:
    achieved float64 operations per second (3 per target, day and used column beside the square) against the vector peak;
    ca_apply_kernel: time against the floor Tl * Cf * itemsize + 8 * Tq * Cf bytes at 8 TB/s.  ``--part apply`` runs the apply kernel
    only (for a counter pass of its own).  -> one result per type of the fine library"""
    Tl, Tq, Cc, Cf, k, window = args.times, max(1, args.times // 4), 400, args.cells if args.cells != 8192 else 100_000, args.k, 45
    index = synth.daily_calendar(Tl + Tq)
    doy = np.asarray(index.dayofyear).astype(np.int32)
    tab = synth.tas_tables(index[:Tl])["y_obs"]
    L = ctx.synth_fill(ctx.empty((Tl, Cc)), synth.GAUSS, 0, tab["stream"], c_full=Cc, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])
    tq = synth.tas_tables(index[Tl:])["X_fut"]
    Q = ctx.synth_fill(ctx.empty((Tq, Cc)), synth.GAUSS, 0, tq["stream"], c_full=Cc, base=tq["base"], amp=tq["amp"], cell_scale=tq["cell_scale"])
    wc = np.repeat(np.cos(np.deg2rad(np.linspace(30.0, 50.0, 20))), 20)
    F64 = ctx.synth_fill(ctx.empty((Tl, Cf)), synth.GAUSS, 0, tab["stream"], c_full=Cf, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])
    out, spare = ctx.empty((Tq, Cf)), ctx.empty((Tq, Cf))
    repeats = max(args.steps, 5)

    def timed(kernel, call, free=False):
        times = []
        for i in range(repeats + 1):  # (the first one warms up)
            ctx.prof_enable(True)
            ctx.prof_reset()
            made = call()
            ctx.synchronize()
            times.append(ctx.prof()[kernel]["ms"])
            ctx.prof_enable(False)
            if free and i < repeats:
                for a in made if isinstance(made, tuple) else (made,):
                    a.free()
        return float(np.median(times[1:])), [min(times[1:]), max(times[1:])], made

    select = lambda: ctx.ca_select(L, Q, wc, k, doy[:Tl], doy[Tl:], 366, window)  # noqa: E731
    if args.part == "apply":
        idx, dist, status = select()
        sel = wgt = None
    else:
        sel_ms, sel_mm, (idx, dist, status) = timed("ca_select_kernel", select, free=True)
        flops = 3.0 * Tq * Tl * Cc
        sel = {"kernel_ms": sel_ms, "kernel_ms_min_max": sel_mm, "float64_ops": flops, "TFLOPs": flops / sel_ms / 1e9,
               "frac_of_vector_peak_78.6_TFLOPs": flops / sel_ms / 1e9 / 78.6}
    first = lambda: ctx.ca_weights(L, Q, wc, idx, dist, status, "regression", 1e-6)  # noqa: E731
    if args.part == "apply":
        weights = first()
    else:
        wgt_ms, wgt_mm, weights = timed("ca_weights_kernel", first, free=True)
        wgt = {"kernel_ms": wgt_ms, "kernel_ms_min_max": wgt_mm}
    st = status.to_host()
    # three targets against the rule restated with plain loops (tests/_constructed_oracle.py), bit for bit
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _constructed_oracle as co

    picks = [0, 1, Tq - 1]
    Lh, Qh = L.to_host(), Q.to_host()[picks]
    none_l, none_q = np.full(Tl, -1, np.int32), np.full(len(picks), -1, np.int32)
    eidx, edist, est = co.select(Lh, Qh, wc, k, doy[:Tl], doy[Tl:][picks], 366, window, none_l, none_q)
    ew, eidx, edist, est = co.weights(Lh, Qh, wc, eidx, edist, est, co.REGRESSION, 1e-6)
    same = bool(np.array_equal(idx.to_host()[picks], eidx) and np.array_equal(dist.to_host()[picks], edist, equal_nan=True)
                and np.array_equal(weights.to_host()[picks], ew, equal_nan=True) and np.array_equal(st[picks], est))
    copy_ms, copy_mm = device_copy_ms(ctx, spare, out, 8 * Tq * Cf, repeats)
    results = []
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        if dtype == np.float32:
            F = ctx.empty((Tl, Cf), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, F64.vptr, Tl * Cf, F.vptr))
            ctx.synchronize()
        else:
            F = F64
        ms, mm, _ = timed("ca_apply_kernel", lambda: ctx.ca_apply(F, idx, weights, out=out))
        used = np.unique(eidx[eidx >= 0])  # the library rows of the three targets: the synthesis against the rule, whole rows
        Fs = np.stack([F.rows(int(t), int(t) + 1).to_host()[0] for t in used])
        got = np.stack([out.rows(q, q + 1).to_host()[0] for q in picks])
        same_out = bool(np.array_equal(got, co.apply(Fs, np.where(eidx >= 0, np.searchsorted(used, eidx), -1), ew), equal_nan=True))
        floor = Tl * Cf * np.dtype(dtype).itemsize + 8 * Tq * Cf
        naive = Tq * k * Cf * np.dtype(dtype).itemsize + 8 * Tq * Cf
        results.append({"workload": f"constructed analogs: Tl={Tl}, Tq={Tq}, Cc={Cc}, Cf={Cf}, k={k}, window={window}, {name} fine library",
                        "repeats": repeats, "fine": name, "targets_ok": int((st == 0).sum()),
                        "tables_bit_identical_to_oracle_targets_0_1_last": same, "ca_select_kernel": sel, "ca_weights_kernel": wgt,
                        "ca_apply_kernel": {"kernel_ms": ms, "kernel_ms_min_max": mm, "floor_bytes": floor, "floor_ms_at_8TBps": floor / 8e9,
                                            "time_over_floor": ms / (floor / 8e9), "gathered_bytes": naive, "gathered_GBps": naive / ms / 1e6,
                                            "bit_identical_to_oracle_targets_0_1_last": same_out},
                        "device_copy_of_output": {"ms": copy_ms, "ms_min_max": copy_mm, "bytes": 8 * Tq * Cf}})
        if F is not F64:
            F.free()
    return results


def bench_localized(ctx, args):
    """The two localized-analog kernels, each alone (ctx.prof(): an event pair around the launch; median and [min, max] of the repeats
    after a warm-up), at the constructed workload's shape: Tl = 14 600 library days, Tq = 3 650 targets, 20 x 20 coarse cells,
    Cf = 100 000 fine cells (250 x 400: a coarse cell is 20 fine cells wide), k = 30, radius 2, with the fine library as float32 and as
    float64 and adjust 'none' and 'shift'; beside ca_select_kernel, sd_memcpy_d2d of the output bytes and ca_apply_kernel of the same
    run.  ca_local_apply_kernel: time against the floor Tq * Cf * (itemsize + 8) bytes at 8 TB/s.  Three targets are compared with the
    rule restated with plain loops (tests/_localized_oracle.py), bit for bit.  -> one result per type of the fine library"""
    Tl, Tq, ny, nx, Cf, k, window, radius = args.times, max(1, args.times // 4), 20, 20, args.cells if args.cells != 8192 else 100_000, args.k, 45, (2, 2)
    Cc = ny * nx
    index = synth.daily_calendar(Tl + Tq)
    doy = np.asarray(index.dayofyear).astype(np.int32)
    tab = synth.tas_tables(index[:Tl])["y_obs"]
    L = ctx.synth_fill(ctx.empty((Tl, Cc)), synth.GAUSS, 0, tab["stream"], c_full=Cc, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])
    tq = synth.tas_tables(index[Tl:])["X_fut"]
    Q = ctx.synth_fill(ctx.empty((Tq, Cc)), synth.GAUSS, 0, tq["stream"], c_full=Cc, base=tq["base"], amp=tq["amp"], cell_scale=tq["cell_scale"])
    wc = np.repeat(np.cos(np.deg2rad(np.linspace(30.0, 50.0, ny))), nx)
    F64 = ctx.synth_fill(ctx.empty((Tl, Cf)), synth.GAUSS, 0, tab["stream"], c_full=Cf, base=tab["base"], amp=tab["amp"], cell_scale=tab["cell_scale"])
    fx = 400 if Cf % 400 == 0 else Cf  # the fine grid: rows of fx cells
    fy = Cf // fx
    f = np.arange(Cf)
    cell_of_host = ((f // fx) * ny // fy * nx + (f % fx) * nx // fx).astype(np.int32)
    cell_of = ctx.to_device(cell_of_host, np.int32)
    out, spare = ctx.empty((Tq, Cf)), ctx.empty((Tq, Cf))
    repeats = max(args.steps, 5)

    def timed(kernel, call, free=False):
        times = []
        for i in range(repeats + 1):  # (the first one warms up)
            ctx.prof_enable(True)
            ctx.prof_reset()
            made = call()
            ctx.synchronize()
            times.append(ctx.prof()[kernel]["ms"])
            ctx.prof_enable(False)
            if free and i < repeats:
                for a in made if isinstance(made, tuple) else (made,):
                    a.free()
        return float(np.median(times[1:])), [min(times[1:]), max(times[1:])], made

    sel_ms, sel_mm, (idx, dist, status) = timed("ca_select_kernel", lambda: ctx.ca_select(L, Q, wc, k, doy[:Tl], doy[Tl:], 366, window), free=True)
    loc_ms, loc_mm, (lidx, ldist) = timed("ca_local_kernel", lambda: ctx.ca_local(L, Q, wc, (ny, nx), radius, idx), free=True)
    weights = ctx.ca_weights(L, Q, wc, idx, dist, status, "regression", 1e-6)
    st = status.to_host()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _localized_oracle as lo

    picks = [0, 1, Tq - 1]
    Lh, Qh, lidx_h = L.to_host(), Q.to_host()[picks], lidx.to_host()
    eslot, elidx, eldist = lo.local(Lh, Qh, wc, idx.to_host()[picks], ny, nx, *radius)
    same = bool(np.array_equal(lidx_h[picks], elidx) and np.array_equal(ldist.to_host()[picks], eldist, equal_nan=True))
    sample = lidx_h[::37]  # (every 37th target)
    runs = len(sample) + int((np.diff(sample[:, cell_of_host], axis=1) != 0).sum())  # stretches of consecutive fine cells that copy one library day
    copy_ms, copy_mm = device_copy_ms(ctx, spare, out, 8 * Tq * Cf, repeats)
    results = []
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        if dtype == np.float32:
            F = ctx.empty((Tl, Cf), np.float32)
            _lib.check(ctx.lib.sd_convert_f64_to_f32_dev(ctx.handle, F64.vptr, Tl * Cf, F.vptr))
            ctx.synchronize()
        else:
            F = F64
        blend_ms, blend_mm, _ = timed("ca_apply_kernel", lambda: ctx.ca_apply(F, idx, weights, out=out))
        used = np.unique(elidx[elidx >= 0])  # the library rows of the three targets: the synthesis against the rule, whole rows
        Fs = np.stack([F.rows(int(t), int(t) + 1).to_host()[0] for t in used])
        floor = Tq * Cf * (np.dtype(dtype).itemsize + 8)
        res = {"workload": f"localized analogs: Tl={Tl}, Tq={Tq}, coarse {ny} x {nx}, Cf={Cf}, k={k}, window={window}, radius={radius[0]}, "
                           f"{name} fine library", "repeats": repeats, "fine": name, "targets_ok": int((st == 0).sum()),
               "distinct_days_per_target_mean": float(np.mean([len(np.unique(r)) for r in sample])),
               "mean_run_of_one_library_day_in_fine_cells": len(sample) * Cf / runs, "choice_bit_identical_to_oracle_targets_0_1_last": same,
               "ca_select_kernel": {"kernel_ms": sel_ms, "kernel_ms_min_max": sel_mm},
               "ca_local_kernel": {"kernel_ms": loc_ms, "kernel_ms_min_max": loc_mm, "over_ca_select_kernel": loc_ms / sel_ms},
               "ca_apply_kernel": {"kernel_ms": blend_ms, "kernel_ms_min_max": blend_mm},
               "device_copy_of_output": {"ms": copy_ms, "ms_min_max": copy_mm, "bytes": 8 * Tq * Cf}}
        for adjust in ("none", "shift"):
            ms, mm, _ = timed("ca_local_apply_kernel", lambda: ctx.ca_local_apply(F, cell_of, lidx, L, Q, adjust=adjust, out=out))
            got = np.stack([out.rows(q, q + 1).to_host()[0] for q in picks])
            want = lo.local_apply(Fs, cell_of_host, np.where(elidx >= 0, np.searchsorted(used, elidx), -1).astype(np.int32), Lh[used], Qh,
                                  getattr(lo, "ADJUST_" + adjust.upper()))
            res[f"ca_local_apply_kernel_{adjust}"] = {"kernel_ms": ms, "kernel_ms_min_max": mm, "floor_bytes": floor, "floor_ms_at_8TBps": floor / 8e9,
                                                      "time_over_floor": ms / (floor / 8e9), "floor_GBps": floor / ms / 1e6,
                                                      "over_ca_apply_kernel": ms / blend_ms, "over_device_copy": ms / copy_ms,
                                                      "bit_identical_to_oracle_targets_0_1_last": bool(np.array_equal(got, want, equal_nan=True))}
        results.append(res)
        if F is not F64:
            F.free()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["bcsd_pr", "analog", "analogreg", "qmr", "ecm", "pure_regression", "zscore", "grouped", "arrm", "regrid", "regrid_e2e", "resample", "disagg", "groupby", "rolling", "remap", "quantile", "spells", "skill", "twosample", "skill_groups", "constructed", "localized"],
                    default="analog")
    ap.add_argument("--cells", type=int, default=8192)
    ap.add_argument("--times", type=int, default=14600)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--kind", default="mean_analogs")
    ap.add_argument("--features", type=int, default=1)
    ap.add_argument("--part", default="all", choices=["all", "apply"], help="constructed: time every kernel, or run ca_apply_kernel only")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    ctx = Context(0)
    if args.workload in ("remap", "constructed", "localized"):  # one JSON line per source type
        for res in {"remap": bench_remap, "constructed": bench_constructed, "localized": bench_localized}[args.workload](ctx, args):
            line = json.dumps(res)
            print(line)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        return
    if args.workload in ("regrid", "regrid_e2e", "resample", "disagg", "groupby", "rolling", "quantile", "spells", "skill", "twosample", "skill_groups"):
        line = json.dumps({"regrid": bench_regrid, "regrid_e2e": bench_regrid_e2e, "resample": bench_resample, "disagg": bench_disagg,
                           "groupby": bench_groupby, "rolling": bench_rolling, "quantile": bench_quantile, "spells": bench_spells, "skill": bench_skill,
                           "twosample": bench_twosample, "skill_groups": bench_skill_groups}[args.workload](ctx, args))
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return
    T, C = args.times, args.cells
    index = synth.daily_calendar(T)
    gid = (np.asarray(index.month) - 1).astype(np.int32)

    def field(kind, stream, **kw):
        d = ctx.empty((T, C))
        ctx.synth_fill(d, kind, 0, stream, c_full=C, **kw)
        return d

    if args.workload == "bcsd_pr":
        f = {n: field(synth.PRECIP, synth.PR_FIELDS[n]["stream"], amp=synth.PR_FIELDS[n]["amp"], p_dry=synth.PR_FIELDS[n]["p_dry"])
             for n in ("X_hist", "y_obs", "X_fut")}
        out = ctx.empty((T, C))
        step = lambda: ctx.bcsd_fit_predict(_lib.BCSD_PR, f["X_hist"], f["y_obs"], gid, 12, f["X_fut"], gid, True, out=out)  # noqa: E731
        bytes_per_cell = 8 * (T + 2 * T)  # y_obs, X_fut, out (X_hist is only validated: + 8*T actually read)
        name = f"BcsdPrecipitation zero-inflated, {C} cells x {T} steps"
    elif args.workload == "zscore":
        from skdownscale_amd.zscore import ZScoreGridModel

        tabs = synth.tas_tables(index)
        f = {n: field(synth.GAUSS, tabs[n]["stream"], base=tabs[n]["base"], amp=tabs[n]["amp"], cell_scale=tabs[n]["cell_scale"])
             for n in ("X_hist", "y_obs", "X_fut")}
        out = ctx.empty((T, C))

        def step():
            gm = ZScoreGridModel(31, ctx=ctx).fit(f["X_hist"], f["y_obs"], index)
            r = gm.predict(f["X_fut"], out=out)
            gm.state.close()
            return r
        bytes_per_cell = 8 * (2 * T + 2 * T)  # fit reads X and y, predict reads X_fut and writes out: 32 B per cell-step
        name = f"ZScoreRegressor w=31 (fit + predict), {C} cells x {T} steps"
    elif args.workload == "grouped":
        from skdownscale_amd.grouping import GroupedGridModel

        F = args.features
        tabs = synth.tas_tables(index)
        y = field(synth.GAUSS, tabs["y_obs"]["stream"], base=tabs["y_obs"]["base"], amp=tabs["y_obs"]["amp"], cell_scale=tabs["y_obs"]["cell_scale"])
        X3, Xq3 = ctx.empty((T, F, C)), ctx.empty((T, F, C))
        for n, arr in (("X_hist", X3), ("X_fut", Xq3)):  # [T, F, C]: feature f of time t is row t*F + f
            ctx.synth_fill(ctx.wrap(arr.ptr, (T * F, C)), synth.GAUSS, 0, tabs[n]["stream"], c_full=C, base=np.repeat(tabs[n]["base"], F),
                           amp=tabs[n]["amp"])
        out = ctx.empty((T, C))

        def step():
            gm = GroupedGridModel(15, ctx=ctx).fit(X3, y, index)
            r = gm.predict(Xq3, index, out=out)
            gm.state.close()
            return r
        bytes_per_cell = 8 * ((F + 1) * T + (F + 1) * T)  # fit reads X and y, predict reads X_fut and writes out
        name = f"GroupedRegressor LinearRegression per day of year, window=15, F={F} (fit + predict), {C} cells x {T} steps"
    elif args.workload == "arrm":
        from skdownscale_amd.arrm import ArrmGridModel

        f = {n: field(synth.GAUSS, s0, amp=a) for n, s0, a in (("X", 30, 3.0), ("y", 31, 4.0), ("Xp", 32, 3.5))}
        out = ctx.empty((T, C))

        def step():
            gm = ArrmGridModel(7, ctx=ctx).fit(f["X"], f["y"])
            r = gm.predict(f["Xp"], out=out)
            gm.state.close()
            return r
        bytes_per_cell = 8 * (2 * T + 2 * T)  # fit reads X and y, predict reads Xp and writes out
        name = f"PiecewiseLinearRegression fit_option='arrm', n_segments=7 (fit + predict), {C} cells x {T} steps"
    elif args.workload in ("qmr", "ecm"):
        f = {n: field(synth.GAUSS, s0, amp=a) for n, s0, a in (("X", 30, 3.0), ("y", 31, 4.0), ("Xp", 32, 3.5))}
        out = ctx.empty((T, C))
        code = 0 if args.workload == "qmr" else 1

        def step():
            st = ctx.qm_fit(f["X"], f["y"])
            r = ctx.qm_predict(st, code, f["Xp"], out=out)
            st.close()
            return r
        bytes_per_cell = 8 * (2 * T + 2 * T)  # X, y, Xp read, out written
        name = f"{'QuantileMappingReressor' if code == 0 else 'EquidistantCdfMatcher difference'} (whole series), {C} cells x {T} steps"
    else:
        F = args.features
        y = field(synth.GAUSS, 20, amp=2.0, stream2=21, amp2=1.0)
        X3, Xq3 = ctx.empty((T, F, C)), ctx.empty((T, F, C))
        for name, arr, s0 in (("X", X3, 20), ("Xq", Xq3, 22)):  # [T, F, C]: feature f of time t is row t*F + f
            rows = ctx.wrap(arr.ptr, (T * F, C))
            ctx.synth_fill(rows, synth.GAUSS, 0, s0, c_full=C)
        out = ctx.empty((T, 3, C))
        kinds = {"best_analog": 0, "sample_analogs": 1, "weight_analogs": 2, "mean_analogs": 3}

        def step():
            if args.workload == "pure_regression":
                st = ctx.linreg_fit(X3, y)
                r = ctx.linreg_predict(st, Xq3, out=out)
                st.close()
                return r
            st = ctx.analog_fit(X3, y)
            if args.workload == "analog":
                k_eff = 1 if args.kind == "best_analog" else args.k  # gard.py:291-296: best_analog queries one neighbour
                r = ctx.analog_predict(st, Xq3, k_eff, kinds[args.kind], out=out)
            else:
                r = ctx.analogreg_predict(st, Xq3, args.k, out=out)
            st.close()
            return r
        bytes_per_cell = 8 * (F * T + T + F * T + 3 * T)
        label = {"analog": "PureAnalog " + args.kind + f" k={args.k}", "analogreg": f"AnalogRegression k={args.k}",
                 "pure_regression": "PureRegression"}[args.workload]
        name = f"{label} F={args.features}, {C} cells x {T} steps"
    step()
    ctx.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    ctx.prof_enable(False)
    prof = {k: v["ms"] / args.steps for k, v in ctx.prof().items()}
    kms = sum(prof.values())
    achieved = C * bytes_per_cell / (kms * 1e-3) / 1e9
    line = json.dumps({"workload": name, "cells_per_s": C / dt, "ms_per_step": dt * 1e3, "kernel_ms_per_step": prof,
                      "roofline": {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                                   "algorithmic_bytes_per_cell": bytes_per_cell}})
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
