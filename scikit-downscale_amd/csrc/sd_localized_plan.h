// Launch plans of the localized-analog calls (LocalizedAnalogs: sd_ca_local_dev, sd_ca_local_apply_dev), as pure host functions (no HIP
// header: tests/localized_plan_check.cpp compiles this file with g++ alone).  The rule is stated in include/sd_downscale.h; the kernels
// are in sd_localized.hip.  Every refusal that depends only on sizes and small host tables is made here, in the order of the checks
// below, before anything is allocated or launched.  Nothing depends on the CU count.
//
// ca_local_plan:        ca_local_kernel -- one workgroup of kLocBlock threads per target.  It stages Q[q] and, analog by analog, the row
//                       of terms wc * (e * e) in LDS: 16 bytes per coarse cell.  Thread tid owns the coarse cells tid + s * kLocBlock,
//                       s < kLocPerThread, and keeps their running minima in registers, so a grid has at most
//                       SD_CA_LOCAL_MAX_CELLS = kLocBlock * kLocPerThread cells (64 KB of LDS at the limit).
// ca_local_apply_plan:  ca_local_apply_kernel -- a workgroup of kLapBlock threads owns kLapCells consecutive fine cells, one per
//                       thread, and kLapRows consecutive targets, which each thread walks kLapBatch at a time.  Grid: workgroup b has
//                       cell tile b % ctiles and row group b / ctiles.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "sd_constructed_plan.h"

namespace sdlo {
using sdca::kGridLimit;
using sdca::kLanes;
using sdca::kMaxK;
using sdca::kMaxTl;
// ca_local_kernel
constexpr int kLocBlock = 512;
constexpr int kLocPerThread = 8;        // coarse cells of a thread: their running minima live in registers
constexpr int64_t kLocMaxCells = (int64_t)kLocBlock * kLocPerThread;
constexpr int64_t loc_lds_bytes(int64_t Cc) { return (int64_t)sizeof(double) * 2 * Cc; }  // Q[q] and the terms of one analog
static_assert(kLocMaxCells == SD_CA_LOCAL_MAX_CELLS, "the limit named in include/sd_downscale.h");
static_assert(kLocMaxCells >= 4096, "the least grid the plan must take");
static_assert(loc_lds_bytes(kLocMaxCells) <= 64 * 1024, "what ca_local_kernel stages fits the LDS a workgroup may ask for");
// ca_local_apply_kernel
constexpr int kLapWaves = 4;
constexpr int kLapBlock = kLanes * kLapWaves;
constexpr int kLapCells = kLapBlock;    // fine cells of a workgroup: one per thread
constexpr int kLapRows = 16;            // targets of a workgroup
constexpr int kLapBatch = 4;            // targets whose gathers are in flight before their arithmetic
static_assert(kLapRows % kLapBatch == 0, "whole batches per row group");
}  // namespace sdlo

struct CaLocalPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int block = 0;        // threads of a workgroup
    int64_t lds_bytes = 0;
    int64_t blocks = 0;   // workgroups
    // ca_local_kernel
    int ry = 0, rx = 0;   // the radii, cut to the grid
    // ca_local_apply_kernel
    int64_t ctiles = 0, row_groups = 0;
};

// ---- sd_ca_local_dev ------------------------------------------------------------------------------------------------------------------
struct CaLocalCall {
    int64_t Tl = 0, Tq = 0, ny = 0, nx = 0, ld_l = 0, ld_q = 0, ry = 0, rx = 0;
    int k = 0;
    const double* wc = nullptr;  // host [ny * nx]
};

inline CaLocalPlan ca_local_plan(const CaLocalCall& c) {
    using namespace sdlo;
    const char* who = "sd_ca_local";
    CaLocalPlan pl;
    if (!(c.Tl > 0 && c.Tq > 0 && c.ny > 0 && c.nx > 0))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: bad sizes (Tl=%lld, Tq=%lld, ny=%lld, nx=%lld)", who, (long long)c.Tl, (long long)c.Tq,
                          (long long)c.ny, (long long)c.nx);
    if (c.k < 1 || c.k > kMaxK) return sdbn::fail(pl, SD_ERR_INVALID, "%s: k = %d lies outside [1, %d]", who, c.k, kMaxK);
    if (c.ry < 0 || c.rx < 0)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: radii (%lld, %lld), expected two numbers of coarse cells >= 0", who, (long long)c.ry, (long long)c.rx);
    // (the cell count before the leading dimensions: ny * nx must not overflow)
    const bool large = c.ny > kLocMaxCells || c.nx > kLocMaxCells || c.ny * c.nx > kLocMaxCells;
    const int64_t Cc = large ? kLocMaxCells : c.ny * c.nx;
    if (!large) {
        if (c.ld_l < Cc)
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_l = %lld is less than the %lld columns of a row", who, (long long)c.ld_l, (long long)Cc);
        if (c.ld_q < Cc)
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_q = %lld is less than the %lld columns of a row", who, (long long)c.ld_q, (long long)Cc);
    }
    for (int64_t i = 0; i < Cc; ++i)
        if (!(c.wc[i] >= 0.0) || std::isinf(c.wc[i]))
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: wc[%lld] = %g, expected a finite weight >= 0", who, (long long)i, c.wc[i]);
    if (c.Tl > kMaxTl) return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Tl = %lld library days, at most %lld are supported", who, (long long)c.Tl, (long long)kMaxTl);
    if (large)
        return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: a coarse grid of %lld x %lld cells, at most %lld cells are supported", who, (long long)c.ny,
                          (long long)c.nx, (long long)kLocMaxCells);
    const int64_t most = std::numeric_limits<int64_t>::max();
    if (c.Tl > most / c.ld_l || c.Tq > most / c.ld_q) return sdbn::fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    if (c.Tq > kGridLimit - 1) return sdbn::fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.block = kLocBlock;
    pl.lds_bytes = loc_lds_bytes(Cc);
    pl.blocks = c.Tq;
    pl.ry = (int)(c.ry < c.ny ? c.ry : c.ny - 1);  // (a radius that reaches past the grid reads the same cells as one that just covers it)
    pl.rx = (int)(c.rx < c.nx ? c.rx : c.nx - 1);
    return pl;
}

// ---- sd_ca_local_apply_dev ------------------------------------------------------------------------------------------------------------
struct CaLocalApplyCall {
    int64_t Tl = 0, Cf = 0, ld_f = 0, Cc = 0, ld_l = 0, ld_q = 0, Tq = 0, q0 = 0, q1 = 0, ld_out = 0;
    int adjust = 0;
    double max_scale = 0.0;
    bool has_coarse = false;  // L_dev and Q_dev are given
};

inline CaLocalPlan ca_local_apply_plan(const CaLocalApplyCall& c) {
    using namespace sdlo;
    const char* who = "sd_ca_local_apply";
    CaLocalPlan pl;
    if (!(c.Tl > 0 && c.Tq > 0 && c.Cf > 0 && c.Cc > 0))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: bad sizes (Tl=%lld, Tq=%lld, Cf=%lld, Cc=%lld)", who, (long long)c.Tl, (long long)c.Tq,
                          (long long)c.Cf, (long long)c.Cc);
    if (c.adjust != SD_CA_ADJUST_NONE && c.adjust != SD_CA_ADJUST_SHIFT && c.adjust != SD_CA_ADJUST_SCALE)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: unknown adjust %d", who, c.adjust);
    if (c.adjust != SD_CA_ADJUST_NONE && !c.has_coarse)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: adjust %d needs L_dev and Q_dev", who, c.adjust);
    if (!(c.max_scale >= 0.0)) return sdbn::fail(pl, SD_ERR_INVALID, "%s: max_scale = %g, expected 0 (no limit) or a limit > 0", who, c.max_scale);
    if (!(0 <= c.q0 && c.q0 < c.q1 && c.q1 <= c.Tq))
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: rows [%lld, %lld) lie outside the %lld targets", who, (long long)c.q0, (long long)c.q1, (long long)c.Tq);
    if (c.ld_f < c.Cf)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_f = %lld is less than the %lld cells of a row", who, (long long)c.ld_f, (long long)c.Cf);
    if (c.ld_out < c.Cf)
        return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.Cf);
    if (c.adjust != SD_CA_ADJUST_NONE) {
        if (c.ld_l < c.Cc)
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_l = %lld is less than the %lld columns of a row", who, (long long)c.ld_l, (long long)c.Cc);
        if (c.ld_q < c.Cc)
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: ld_q = %lld is less than the %lld columns of a row", who, (long long)c.ld_q, (long long)c.Cc);
    }
    if (c.Tl > kMaxTl) return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Tl = %lld library days, at most %lld are supported", who, (long long)c.Tl, (long long)kMaxTl);
    if (c.Cc > kLocMaxCells)
        return sdbn::fail(pl, SD_ERR_UNSUPPORTED, "%s: Cc = %lld coarse cells, at most %lld are supported", who, (long long)c.Cc, (long long)kLocMaxCells);
    const int64_t most = std::numeric_limits<int64_t>::max();
    if (c.Tl > most / c.ld_f || c.Tq > most / c.ld_out) return sdbn::fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    if (c.adjust != SD_CA_ADJUST_NONE && (c.Tl > most / c.ld_l || c.Tq > most / c.ld_q)) return sdbn::fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    pl.block = kLapBlock;
    pl.ctiles = (c.Cf - 1) / kLapCells + 1;
    pl.row_groups = (c.q1 - c.q0 - 1) / kLapRows + 1;
    if (pl.row_groups > (kGridLimit - 1) / pl.ctiles) return sdbn::fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = pl.ctiles * pl.row_groups;
    return pl;
}
