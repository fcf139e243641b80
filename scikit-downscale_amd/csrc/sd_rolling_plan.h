// Launch plan of the rolling-window call (GridArray.rolling: a [T, C] field, cells fastest; output row t is a statistic of the rows
// t - back .. t - back + window - 1 of its own cell), as pure host functions (no HIP header: tests/rolling_plan_check.cpp compiles
// this file with g++ alone).
//
// rolling_plan: every refusal, then the geometry of rolling_kernel (sd_rolling.hip).  The cell tiling is that of sd_bins_plan.h -- a
// workgroup of kWaves waves owns a tile of kLanes * cols adjacent cells -- and a workgroup also owns a run of `run` consecutive output
// rows, of which wave k takes the rows k, k + kWaves, ...  Two paths:
//   staged:    the workgroup loads the run + window - 1 source rows its windows touch into LDS once (positions first .. first + run +
//              window - 2 with first = the run's first row - back; a position outside [0, T) is taken modulo T with wrap and read by
//              no window without) and every window is evaluated from there.  One staged row is the tile's row as the source type: row_bytes =
//              kLanes * cols * sizeof(S).  The staged bytes stay within kLdsBudget, which leaves two workgroups per CU (160 KiB of
//              LDS).  run = max(window, kRun) where that fits -- the halo then at most doubles the reads -- else what fits; a window
//              that leaves fewer than kMinRun rows is not staged.
//   unstaged:  the same evaluation reads its rows from global memory; run = kMinRun.
// Both paths add the samples of a window in time order: they give the same bits.
#pragma once
#include "sd_bins_plan.h"

namespace sdrl {
using namespace sdbn;  // the cell tiling and kBatch are the shared ones
constexpr int64_t kLdsBudget = 64 * 1024;  // staged bytes of a workgroup: two workgroups fit the 160 KiB of a CU
constexpr int kRun = 32;                   // output rows of a staged workgroup at small windows
constexpr int kMinRun = 16;                // the fewest output rows worth staging for; the run of the unstaged path
}  // namespace sdrl

struct RollingCall {
    int op = SD_ROLLING_MEAN;
    bool src_is_f32 = false;
    int64_t T = 0, C = 0;  // rows and cells of the source block
    int64_t ld = 0;        // elements between two rows of the source (>= C)
    int64_t window = 0;    // rows of a window
    int64_t back = 0;      // the window of row t starts at t - back: window - 1 for a trailing window, window / 2 for a centred one
    int64_t min_periods = 0;
    int64_t ddof = 0;
    bool wrap = false;     // rows are taken modulo T instead of being clipped to [0, T)
    int64_t t0 = 0, n_out = 0;  // the rows t0 .. t0 + n_out - 1 are computed
    int64_t ld_out = 0;    // elements between two rows of the output (>= C)
    bool src_aligned16 = true, out_aligned16 = true;
};

struct RollingPlan {
    int error = SD_OK;
    char message[256] = "";
    int cols = 0;        // adjacent cells of a lane
    int block = 0;       // threads of a workgroup
    bool staged = false;
    int run = 0;         // output rows of a workgroup
    int64_t lds_rows = 0, lds_bytes = 0;  // staged: run + window - 1 rows of row_bytes; else 0
    int64_t ctiles = 0, row_groups = 0, blocks = 0;  // cell tiles by runs of rows, cell tile fastest
};

inline RollingPlan rolling_plan(const RollingCall& c) {
    using namespace sdrl;
    const char* const who = "sd_rolling";
    RollingPlan pl;
    if (!(c.op == SD_ROLLING_MEAN || c.op == SD_ROLLING_SUM || c.op == SD_ROLLING_VAR || c.op == SD_ROLLING_STD))
        return fail(pl, SD_ERR_INVALID, "%s: unknown op code %d", who, c.op);
    if (!(c.T > 0 && c.C > 0)) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld)", who, (long long)c.T, (long long)c.C);
    if (c.window < 1) return fail(pl, SD_ERR_INVALID, "%s: window = %lld, expected at least 1", who, (long long)c.window);
    if (c.back < 0 || c.back >= c.window)
        return fail(pl, SD_ERR_INVALID, "%s: back = %lld lies outside [0, window = %lld)", who, (long long)c.back, (long long)c.window);
    if (c.min_periods < 0 || c.min_periods > c.window)
        return fail(pl, SD_ERR_INVALID, "%s: min_periods = %lld lies outside [0, window = %lld]", who, (long long)c.min_periods, (long long)c.window);
    if (c.ddof < 0) return fail(pl, SD_ERR_INVALID, "%s: ddof = %lld is negative", who, (long long)c.ddof);
    if (c.t0 < 0 || c.n_out <= 0 || c.n_out > c.T - c.t0)
        return fail(pl, SD_ERR_INVALID, "%s: the output rows %lld .. %lld lie outside the %lld rows of the source", who, (long long)c.t0,
                    (long long)c.t0 + c.n_out - 1, (long long)c.T);
    if (c.wrap && c.window > c.T)
        return fail(pl, SD_ERR_INVALID, "%s: window = %lld is longer than the %lld rows it wraps around", who, (long long)c.window, (long long)c.T);
    if (c.ld < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld = %lld is less than the %lld cells of a row", who, (long long)c.ld, (long long)c.C);
    if (c.ld_out < c.C)
        return fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of both fields stay far from the end of int64_t)
    if (c.T > most / c.ld || c.n_out > most / c.ld_out) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    // the cell tiling of the binned kernels: four cells per lane for float32, else two, else one, where every access is whole and aligned
    const auto fits = [&](int cols) { return c.C % cols == 0 && c.ld % cols == 0 && c.ld_out % cols == 0 && c.src_aligned16 && c.out_aligned16; };
    pl.cols = (c.src_is_f32 && fits(4)) ? 4 : fits(2) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.ctiles = (c.C - 1) / (kLanes * pl.cols) + 1;
    const int64_t row_bytes = (int64_t)kLanes * pl.cols * (c.src_is_f32 ? 4 : 8);
    const int64_t fit = kLdsBudget / row_bytes - (c.window - 1);  // output rows whose staged rows fit the budget
    pl.staged = fit >= kMinRun;
    const int64_t want = c.window > kRun ? c.window : kRun;
    int64_t run = pl.staged ? (want < fit ? want : fit) : kMinRun;
    if (run > c.n_out) run = c.n_out;
    pl.run = (int)run;
    pl.lds_rows = pl.staged ? run + c.window - 1 : 0;
    pl.lds_bytes = pl.lds_rows * row_bytes;
    pl.row_groups = (c.n_out - 1) / run + 1;
    if (pl.row_groups > (kGridLimit - 1) / pl.ctiles)  // blocks < 2^31
        return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = pl.ctiles * pl.row_groups;
    return pl;
}
