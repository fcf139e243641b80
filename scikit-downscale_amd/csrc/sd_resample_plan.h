// Launch plan of a time resampling call (GridArray.resample(time=rule).mean() / .sum(): a [T, C] field, cells fastest, reduced over
// runs of consecutive rows into [M, C]), as pure host functions (no HIP header: tests/resample_plan_check.cpp compiles this file with
// g++ alone).
//
// The bins are not computed here: pandas makes them on the host (skdownscale_amd/resample.py: time_bins) and hands over the table
// offsets [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].
//
// resample_plan:           the geometry of resample_kernel (sd_resample.hip) from the sizes of the call -- grid, block, cells per lane,
//                          bins per workgroup -- and every refusal that depends only on sizes and codes.  The launcher takes all of it
//                          from here.  The kernel keeps nothing in LDS and its grid does not depend on the CU count.
// resample_check_offsets:  the refusals of the table itself: it starts at 0, never decreases and ends at T, so that every row the
//                          kernel reads lies inside the field.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"

namespace sdrs {
constexpr int kLanes = 64;
constexpr int kWaves = 4;         // waves of a workgroup: the same cells, consecutive runs of bins
constexpr int kBinsPerWave = 2;   // whole bins of one wave, one after the other
constexpr int kBatch = 8;         // rows whose loads are in flight before their arithmetic
constexpr int kBinsPerGroup = kWaves * kBinsPerWave;  // bins of a workgroup
constexpr int64_t kGridLimit = (int64_t)1 << 31;
}  // namespace sdrs

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

struct ResamplePlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int cols = 0;       // adjacent cells of a lane: one load of cols source elements per row, one store of cols doubles per bin
    int block = 0;      // threads of a workgroup
    int64_t ctiles = 0;      // cell tiles of kLanes * cols cells
    int64_t bin_groups = 0;  // runs of kBinsPerGroup bins
    int64_t blocks = 0;      // ctiles * bin_groups, cell tile fastest
};

namespace resample_plan_detail {
template <class... A>
ResamplePlan fail(ResamplePlan pl, int code, const char* fmt, A... a) {
    snprintf(pl.message, sizeof pl.message, fmt, a...);
    pl.error = code;
    return pl;
}
}  // namespace resample_plan_detail

inline ResamplePlan resample_plan(const ResampleCall& c) {
    using namespace sdrs;
    using resample_plan_detail::fail;
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
    // cols cells per lane: every load of cols source elements and every store of cols doubles is one aligned access of up to 16 bytes
    // (float32 x 4 is stored as two 16-byte halves), in every row -- so cols divides C and both leading dimensions
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld % cols == 0 && c.ld_out % cols == 0;
        return whole && c.src_aligned16 && c.out_aligned16;
    };
    pl.cols = (c.src_is_f32 && fits(4)) ? 4 : fits(2) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.ctiles = (c.C - 1) / (kLanes * pl.cols) + 1;
    pl.bin_groups = (c.M - 1) / kBinsPerGroup + 1;
    if (pl.bin_groups > (kGridLimit - 1) / pl.ctiles)  // blocks < 2^31
        return fail(pl, SD_ERR_INVALID, "%s", "sd_resample: grid too large");
    pl.blocks = pl.ctiles * pl.bin_groups;
    return pl;
}

// the table of a call that resample_plan accepted: offsets [M + 1]
inline ResamplePlan resample_check_offsets(ResamplePlan pl, const ResampleCall& c, const int64_t* offsets) {
    using resample_plan_detail::fail;
    if (pl.error != SD_OK) return pl;
    if (offsets[0] != 0) return fail(pl, SD_ERR_INVALID, "sd_resample: offsets[0] = %lld, expected 0", (long long)offsets[0]);
    for (int64_t m = 0; m < c.M; ++m)
        if (offsets[m + 1] < offsets[m])
            return fail(pl, SD_ERR_INVALID, "sd_resample: offsets decrease at bin %lld (%lld after %lld)", (long long)m, (long long)offsets[m + 1],
                        (long long)offsets[m]);
    if (offsets[c.M] != c.T)
        return fail(pl, SD_ERR_INVALID, "sd_resample: offsets[M] = %lld, expected T = %lld", (long long)offsets[c.M], (long long)c.T);
    return pl;
}
