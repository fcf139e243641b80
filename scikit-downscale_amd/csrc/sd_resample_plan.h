// Launch plan of a time resampling call (GridArray.resample(time=rule).mean() / .sum(): a [T, C] field, cells fastest, reduced over
// runs of consecutive rows into [M, C]), as pure host functions (no HIP header: tests/resample_plan_check.cpp compiles this file with
// g++ alone).
//
// The bins are not computed here: pandas makes them on the host (skdownscale_amd/resample.py: time_bins) and hands over the table
// offsets [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].
//
// resample_plan:           every refusal that depends only on sizes and codes, then the geometry of resample_kernel (sd_resample.hip)
//                          from sd_bins_plan.h.  The launcher takes all of it from here.
// resample_check_offsets:  the refusals of the table itself (sd_bins_plan.h: check_offsets, ending at T).
#pragma once
#include "sd_bins_plan.h"

namespace sdrs {
using namespace sdbn;  // the constants of this plan are the shared ones
}

struct ResampleCall {
    int op = SD_RESAMPLE_MEAN;
    bool src_is_f32 = false;
    int64_t T = 0, C = 0;      // rows and cells of the source
    int64_t ld = 0;            // elements between two rows of the source (>= C)
    int64_t M = 0;             // bins
    int64_t ld_out = 0;        // elements between two rows of the output (>= C)
    bool src_aligned16 = true;  // the source pointer is a multiple of 16 bytes
    bool out_aligned16 = true;  // the output pointer is a multiple of 16 bytes
};

using ResamplePlan = sdbn::BinsPlan;

inline ResamplePlan resample_plan(const ResampleCall& c) {
    using sdbn::fail;
    ResamplePlan pl;
    if (!(c.op == SD_RESAMPLE_MEAN || c.op == SD_RESAMPLE_SUM)) return fail(pl, SD_ERR_INVALID, "sd_resample: unknown op code %d", c.op);
    if (!(c.T > 0 && c.C > 0 && c.M > 0))
        return fail(pl, SD_ERR_INVALID, "sd_resample: bad sizes (T=%lld, C=%lld, M=%lld)", (long long)c.T, (long long)c.C, (long long)c.M);
    if (c.ld < c.C)
        return fail(pl, SD_ERR_INVALID, "sd_resample: ld = %lld is less than the %lld cells of a row", (long long)c.ld, (long long)c.C);
    if (c.ld_out < c.C)
        return fail(pl, SD_ERR_INVALID, "sd_resample: ld_out = %lld is less than the %lld cells of a row", (long long)c.ld_out, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of both fields stay far from the end of int64_t)
    if (c.T > most / c.ld || c.M > most / c.ld_out) return fail(pl, SD_ERR_INVALID, "%s", "sd_resample: field too large");
    // cols divides C and both leading dimensions: an access of cols cells is whole and aligned in every row
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld % cols == 0 && c.ld_out % cols == 0;
        return whole && c.src_aligned16 && c.out_aligned16;
    };
    return sdbn::bins_plan("sd_resample", c.src_is_f32, c.C, c.M, fits);
}

// the table of a call that resample_plan accepted: offsets [M + 1]
inline ResamplePlan resample_check_offsets(ResamplePlan pl, const ResampleCall& c, const int64_t* offsets) {
    return sdbn::check_offsets(pl, "sd_resample", offsets, c.M, "T", c.T);
}
