// Launch plans of the constructed-analog calls (ConstructedAnalogs: sd_ca_select_dev, sd_ca_weights_dev, sd_ca_apply_dev), as pure host
// functions (no HIP header: tests/constructed_plan_check.cpp compiles this file with g++ alone).  The rule is stated in
// include/sd_downscale.h; the kernels are in sd_constructed.hip.  Every refusal that depends only on sizes and small host tables is made
// here, in the order of the checks below, before anything is allocated or launched.  Nothing depends on the CU count.
//
// ca_select_plan:   ca_select_kernel -- a workgroup of kSelBlock threads owns kSelQ consecutive targets and sweeps the whole library in
//                   tiles of kSelL days; the used columns are staged kSelCols at a time.  Grid: one workgroup per target tile.
// ca_weights_plan:  ca_weights_kernel -- one workgroup of kWgtBlock threads per target; the k analog rows are staged kWgtCols used
//                   columns at a time.
// ca_apply_plan:    ca_apply_kernel -- a workgroup of kAppWaves waves owns kAppCells consecutive fine cells and kAppRows consecutive
//                   targets (each wave kAppRows / kAppWaves of them).  Grid: the workgroup ids of one XCD (every kXcds-th id) walk the row
//                   groups of one cell tile before the next tile, so that the workgroups in flight share few cell tiles and their slab of
//                   the fine library (Tl * cells in flight * itemsize) is re-read from cache.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "sd_bins_plan.h"

namespace sdca {
constexpr int kLanes = 64;
constexpr int kMaxK = 32;               // analogs of a target: one lane of half a wave each in the k-list
// ca_select_kernel
constexpr int kSelBlock = 256;
constexpr int kSelQ = 8;                // targets of a workgroup
constexpr int kSelL = 128;              // library days of a tile
constexpr int kSelCols = 32;            // used columns staged per step
constexpr int kSelQPerThread = 1, kSelLPerThread = 4;  // the register tile of (q, t) accumulators
constexpr int kSelPad = 2;              // doubles between two staged columns of the library tile (16-byte aligned rows)
static_assert((kSelQ / kSelQPerThread) * (kSelL / kSelLPerThread) == kSelBlock, "one register tile per thread");
static_assert(kSelQ % (kSelBlock / kLanes) == 0, "whole targets per wave in the merge");
static_assert(kSelL % kLanes == 0, "whole waves of candidates in the merge");
constexpr int64_t sel_lds_bytes() {
    return (int64_t)sizeof(double) * (kSelCols * (kSelL + kSelPad) + kSelCols * kSelQ + kSelCols + kSelQ * kSelL) + 4 * kSelQ;
}
static_assert(sel_lds_bytes() <= 64 * 1024, "at least two workgroups share the 160 KB of a CU");
// ca_weights_kernel
constexpr int kWgtBlock = 256;
constexpr int kWgtCols = 64;            // used columns staged per step
constexpr int kWgtEntries = kMaxK * (kMaxK + 1) / 2 + kMaxK;  // lower triangle of G and b: 560 sums
constexpr int kWgtPerThread = (kWgtEntries + kWgtBlock - 1) / kWgtBlock;
// ca_apply_kernel
constexpr int kAppWaves = 4;
constexpr int kAppBlock = kLanes * kAppWaves;
constexpr int kAppCells = kLanes;       // fine cells of a workgroup: one per lane
constexpr int kAppRows = 32;            // targets of a workgroup
constexpr int kAppBatch = 8;            // analog rows whose loads are in flight before their arithmetic
constexpr int kXcds = 8;                // consecutive workgroup ids go to consecutive XCDs, each with an L2 of its own
static_assert(kAppRows % kAppWaves == 0, "whole targets per wave");
// limits of the plans
constexpr int64_t kMaxTl = (int64_t)1 << 24;   // library days (day numbers are int32; the sentinel of the k-list is INT32_MAX)
constexpr int64_t kMaxCc = (int64_t)1 << 16;   // coarse columns (the column flags come back to the host once per call)
constexpr int64_t kGridLimit = (int64_t)1 << 31;
}  // namespace sdca

// ---- what all three calls share -----------------------------------------------------------------------------------------------------
struct CaPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int block = 0;        // threads of a workgroup
    int64_t lds_bytes = 0;
    int64_t blocks = 0;   // workgroups
    // ca_select_kernel
    int64_t q_tiles = 0, l_tiles = 0;
    // ca_apply_kernel
    int64_t ctiles = 0, row_groups = 0;
};

struct CaCoarse {  // the coarse side of a call: sd_ca_select_dev and sd_ca_weights_dev
    int64_t Tl = 0, Tq = 0, Cc = 0, ld_l = 0, ld_q = 0;
    int k = 0;
    const double* wc = nullptr;  // host [Cc]
};

inline CaPlan ca_coarse_checks(const char* who, const CaCoarse& c) {
    using namespace sdca;
    CaPlan pl;
    if (!(c.Tl > 0 && c.Tq > 0 && c.Cc > 0))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: bad sizes (Tl=%lld, Tq=%lld, Cc=%lld)", who, (long long)c.Tl, (long long)c.Tq, (long long)c.Cc);
    if (c.k < 1 || c.k > kMaxK) return sdbn::fail(pl, SD_ERR_INVALID, "%s: k = %d lies outside [1, %d]", who, c.k, kMaxK);
    if (c.ld_l < c.Cc)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_l = %lld is less than the %lld columns of a row", who, (long long)c.ld_l, (long long)c.Cc);
    if (c.ld_q < c.Cc)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_q = %lld is less than the %lld columns of a row", who, (long long)c.ld_q, (long long)c.Cc);
    for (int64_t i = 0; i < c.Cc && i < kMaxCc; ++i)
        if (!(c.wc[i] >= 0.0) || std::isinf(c.wc[i]))
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: wc[%lld] = %g, expected a finite weight >= 0", who, (long long)i, c.wc[i]);
    if (c.Tl > kMaxTl) return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Tl = %lld library days, at most %lld are supported", who, (long long)c.Tl, (long long)kMaxTl);
    if (c.Cc > kMaxCc) return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Cc = %lld columns, at most %lld are supported", who, (long long)c.Cc, (long long)kMaxCc);
    const int64_t most = std::numeric_limits<int64_t>::max();
    if (c.Tl > most / c.ld_l || c.Tq > most / c.ld_q) return sdbn::fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    return pl;
}

// ---- sd_ca_select_dev -----------------------------------------------------------------------------------------------------------------
inline CaPlan ca_select_plan(const CaCoarse& c, int64_t period, int64_t window) {
    using namespace sdca;
    const char* who = "sd_ca_select";
    CaPlan pl = ca_coarse_checks(who, c);
    if (pl.error != SD_OK) return pl;
    if (window >= 0 && period <= 0)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: period = %lld with window = %lld, expected a period > 0", who, (long long)period, (long long)window);
    if (period > std::numeric_limits<int32_t>::max() || window > std::numeric_limits<int32_t>::max())
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: period and window must fit 32 bits", who);
    pl.block = kSelBlock;
    pl.lds_bytes = sel_lds_bytes();
    pl.q_tiles = (c.Tq - 1) / kSelQ + 1;
    pl.l_tiles = (c.Tl - 1) / kSelL + 1;
    if (pl.q_tiles > kGridLimit - 1) return sdbn::fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = pl.q_tiles;
    return pl;
}

// ---- sd_ca_weights_dev ----------------------------------------------------------------------------------------------------------------
inline CaPlan ca_weights_plan(const CaCoarse& c, int kind, double ridge) {
    using namespace sdca;
    const char* who = "sd_ca_weights";
    CaPlan pl = ca_coarse_checks(who, c);
    if (pl.error != SD_OK) return pl;
    if (kind != SD_CA_REGRESSION && kind != SD_CA_MEAN) return sdbn::fail(pl, SD_ERR_INVALID, "%s: unknown kind %d", who, kind);
    if (!(ridge >= 0.0) || std::isinf(ridge)) return sdbn::fail(pl, SD_ERR_INVALID, "%s: ridge = %g, expected a finite factor >= 0", who, ridge);
    if (c.Tq > kGridLimit - 1) return sdbn::fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.block = kWgtBlock;
    pl.blocks = c.Tq;
    return pl;
}

// ---- sd_ca_apply_dev ------------------------------------------------------------------------------------------------------------------
struct CaApplyCall {
    int64_t Tl = 0, Cf = 0, ld_f = 0, Tq = 0, q0 = 0, q1 = 0, ld_out = 0;
    int k = 0;
};

inline CaPlan ca_apply_plan(const CaApplyCall& c) {
    using namespace sdca;
    const char* who = "sd_ca_apply";
    CaPlan pl;
    if (!(c.Tl > 0 && c.Tq > 0 && c.Cf > 0))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: bad sizes (Tl=%lld, Tq=%lld, Cf=%lld)", who, (long long)c.Tl, (long long)c.Tq, (long long)c.Cf);
    if (c.k < 1 || c.k > kMaxK) return sdbn::fail(pl, SD_ERR_INVALID, "%s: k = %d lies outside [1, %d]", who, c.k, kMaxK);
    if (!(0 <= c.q0 && c.q0 < c.q1 && c.q1 <= c.Tq))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: rows [%lld, %lld) lie outside the %lld targets", who, (long long)c.q0, (long long)c.q1, (long long)c.Tq);
    if (c.ld_f < c.Cf)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_f = %lld is less than the %lld cells of a row", who, (long long)c.ld_f, (long long)c.Cf);
    if (c.ld_out < c.Cf)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.Cf);
    if (c.Tl > kMaxTl) return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Tl = %lld library days, at most %lld are supported", who, (long long)c.Tl, (long long)kMaxTl);
    const int64_t most = std::numeric_limits<int64_t>::max();
    if (c.Tl > most / c.ld_f || c.Tq > most / c.ld_out) return sdbn::fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    pl.block = kAppBlock;
    pl.ctiles = (c.Cf - 1) / kAppCells + 1;
    pl.row_groups = (c.q1 - c.q0 - 1) / kAppRows + 1;
    // workgroup b serves XCD b % kXcds; the ids of one XCD walk the row groups of one cell tile, then those of the next: tile
    // (b / kXcds / row_groups) * kXcds + b % kXcds, padded to whole rounds of kXcds tiles (a workgroup past the last tile returns)
    const int64_t padded = ((pl.ctiles - 1) / kXcds + 1) * kXcds;
    if (pl.row_groups > (kGridLimit - 1) / padded) return sdbn::fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = padded * pl.row_groups;
    return pl;
}
