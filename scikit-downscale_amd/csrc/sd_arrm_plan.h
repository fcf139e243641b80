// Host-side launch plan of an ARRM piecewise-linear fit (PiecewiseLinearRegression(fit_option='arrm'), arrm.py:19-105 and
// 144-167 of the reference), as pure host functions (no HIP header: tests/arrm_plan_check.cpp compiles them with g++ alone).
// sd_arrm.hip takes the window geometry, every refusal that depends only on sizes, and the grid, block and LDS size of each of
// its kernels from here.
//
// Geometry of the reference, restated: n = T samples, start = argmin |plotting_positions(n) - 0.4| (first minimum),
// width = max(round(0.05 n), 10) and mid = round((left + right) / 2), both with Python's round (half to even).  The upper loop
// visits right = start .. n (left = right - width), the lower loop left = start2 .. 0 with start2 = min(upper picks) - 6, which
// only the device knows; a lower window is cut at n like a Python slice.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"

namespace sdarrm {

constexpr int kMinWidth = 10;      // arrm.py:37: the smallest window, and the half width of the mask around a pick
constexpr int kMinT = 50;          // below it start < width: the upper loop would slice from a negative left
constexpr int kMaxBreaks = 16;     // breaks per cell (2 * (max_breakpoints / 2))
constexpr int kWindowThreads = 512;  // arrm_select_kernel: one workgroup per cell
constexpr int kCells = 64;         // adjacent cells of an accumulate / predict workgroup: 512-byte row fragments
constexpr int kMaxSlices = 8;      // time slices (grid.y) of arrm_accum_kernel

// callable from the kernels too: sd_arrm.hip takes the slot and last-writer rules from here, so there is one definition
#if defined(__HIPCC__)
#define SDARRM_HD __host__ __device__
#else
#define SDARRM_HD
#endif

// Python's round() of a double: half to even (the default rounding mode of nearbyint)
inline int64_t py_round(double v) { return (int64_t)std::nearbyint(v); }
// arrm.py:66, 90: the r2 slot of the window [left, right), round((left + right) / 2) with Python's round: an odd sum lies half way
// between k and k + 1 and goes to the even one (integer arithmetic; tests/test_arrm_plan.py holds it against Python)
SDARRM_HD inline int64_t mid_of(int64_t left, int64_t right) {
    const int64_t s = left + right, k = s >> 1;
    return (s & 1) == 0 ? k : k + (k & 1);
}
// arrm.py:58
inline int64_t window_width(int64_t n) {
    const int64_t w = py_round(0.05 * (double)n);
    return w > kMinWidth ? w : kMinWidth;
}
// arrm.py:47, 55 with quantile.py:43: (arange(1, n + 1) - 0.4) / (n + 1.0 - 0.4 - 0.4), first index closest to 0.4
inline int64_t start_index(int64_t n) {
    const double denom = (double)n + 1.0 - 0.4 - 0.4;
    int64_t best = 0;
    double best_d = INFINITY;
    for (int64_t i = 0; i < n; ++i) {
        const double d = std::fabs(((double)(i + 1) - 0.4) / denom - 0.4);
        if (d < best_d) {
            best_d = d;
            best = i;
        }
    }
    return best;
}
// The upper loop runs in ascending order of right, the lower loop in descending order of left, so of two windows that share a
// slot (odd width) the later one stays: the larger left above, the smaller left below.
SDARRM_HD inline bool upper_final(int64_t left, int64_t width, int64_t n) {
    return left + 1 + width > n || mid_of(left + 1, left + 1 + width) != mid_of(left, left + width);
}
SDARRM_HD inline bool lower_final(int64_t left, int64_t width) { return left == 0 || mid_of(left - 1, left - 1 + width) != mid_of(left, left + width); }

}  // namespace sdarrm

struct ArrmCall {
    int64_t T = 0, C = 0, ld = 0;
    int max_breakpoints = 0;
    size_t lds_max = 0;
    int cu_count = 0;
};

struct ArrmLaunch {
    int64_t gx, gy;
    int block;
    size_t lds;  // dynamic LDS bytes
};

struct ArrmPlan {
    int error = SD_OK;  // an error code, with its message: nothing is allocated, nothing runs
    char message[256] = "";
    int half = 0, B = 0;            // picks per phase, breaks per cell
    int64_t start = 0, width = 0;   // first right of the upper loop, window width
    int nacc = 0;                   // doubles per (cell, slice) of the accumulate pass: 5 per segment + sum of squares
    int slices = 0;                 // grid.y of arrm_accum_kernel
    ArrmLaunch select{}, accum{}, solve{};
};

namespace arrm_plan_detail {
template <class... A>
bool fail(ArrmPlan* pl, int code, const char* fmt, A... a) {
    snprintf(pl->message, sizeof pl->message, fmt, a...);
    pl->error = code;
    return false;
}
}  // namespace arrm_plan_detail

inline ArrmPlan arrm_plan(const ArrmCall& c) {
    using namespace sdarrm;
    using arrm_plan_detail::fail;
    ArrmPlan pl;
    if (!(c.T > 0 && c.C > 0 && c.ld >= c.C)) {
        fail(&pl, SD_ERR_INVALID, "%s", "sd_arrm_fit: bad sizes");
        return pl;
    }
    if (c.T < kMinT) {
        fail(&pl, SD_ERR_INVALID, "sd_arrm_fit: T = %lld samples, at least %d are needed (the first window would start before the series)",
             (long long)c.T, kMinT);
        return pl;
    }
    pl.half = c.max_breakpoints / 2;
    pl.B = 2 * pl.half;
    if (c.max_breakpoints < 2 || pl.B > kMaxBreaks) {
        fail(&pl, SD_ERR_INVALID, "sd_arrm_fit: max_breakpoints = %d gives %d breaks, supported are 2 .. %d", c.max_breakpoints,
             c.max_breakpoints < 0 ? 0 : pl.B, kMaxBreaks);
        return pl;
    }
    pl.start = start_index(c.T);
    pl.width = window_width(c.T);
    // arrm_select_kernel keeps the r2 series of its cell in LDS; the reduction buffers are static
    pl.select.lds = sizeof(double) * (size_t)c.T;
    if (pl.select.lds + 8192 > c.lds_max) {
        fail(&pl, SD_ERR_UNSUPPORTED, "sd_arrm_fit: the r2 series of %lld samples does not fit in LDS", (long long)c.T);
        return pl;
    }
    const int64_t per_cu = (int64_t)(c.lds_max / (pl.select.lds + 8192));
    const int64_t resident = (int64_t)c.cu_count * (per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu);
    pl.select.gx = c.C < resident ? c.C : resident;
    pl.select.gy = 1;
    pl.select.block = kWindowThreads;
    // arrm_accum_kernel: every thread owns 5 sums per segment in LDS; 256 threads when that fits in 64 KB, else 128
    pl.nacc = 5 * (pl.B - 1) + 1;
    pl.accum.block = sizeof(double) * (size_t)(pl.nacc - 1) * 256 <= ((size_t)64 << 10) ? 256 : 128;
    pl.accum.lds = sizeof(double) * (size_t)(pl.nacc - 1) * pl.accum.block + sizeof(double) * (size_t)kMaxBreaks * kCells;
    pl.accum.gx = (c.C + kCells - 1) / kCells;
    // time slices: at least 64 steps per thread.  The count depends on T alone, so a cell's sums are added in the same order
    // whatever grid it is part of (a chunked grid equals the whole grid bit for bit)
    int64_t want = c.T / (64 * (pl.accum.block / kCells));
    if (want > kMaxSlices) want = kMaxSlices;
    if (want < 1) want = 1;
    pl.slices = (int)want;
    pl.accum.gy = pl.slices;
    pl.solve = {(c.C + 255) / 256, 1, 256, 0};
    return pl;
}

// arrm_predict_kernel: 64 cells x 4 time slices per workgroup, the model of the 64 cells in LDS
inline ArrmLaunch arrm_predict_launch(int64_t Tq, int64_t C, int B) {
    const int64_t rows = 4 * 64;  // time steps of one workgroup
    return {(C + sdarrm::kCells - 1) / sdarrm::kCells, (Tq + rows - 1) / rows, 256, sizeof(double) * 2 * (size_t)B * sdarrm::kCells};
}
