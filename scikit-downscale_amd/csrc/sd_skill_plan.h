// Launch plan of a paired skill call (GridArray.compare(other).resample(time=rule).bias() / .rmse() / .corr() / ...: two [T, C] fields,
// cells fastest, walked in lock-step and summarised over runs of consecutive rows into nstat [M, C] fields), as pure host functions
// (no HIP header: tests/skill_plan_check.cpp compiles this file with g++ alone).
//
// The bins are not computed here: pandas makes them on the host (skdownscale_amd/resample.py: time_bins) and hands over the table
// offsets [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].
//
// skill_plan:  every refusal, in the order of the checks below -- codes, nstat, sizes, T, leading dimensions, stride, too large, the
//              table of bins (check_offsets, ending at T) -- then the geometry of skill_kernel (sd_skill.hip) from sd_bins_plan.h.  The
//              launcher takes all of it from here.  offsets is read only after everything that depends on sizes and codes alone has
//              passed.
#pragma once
#include "sd_bins_plan.h"

namespace sdsk {
using namespace sdbn;  // the constants of this plan are the shared ones
constexpr int kMaxStats = SD_SKILL_STD_RATIO + 1;  // statistics of one call at the most (a code may repeat)
}

struct SkillCall {
    bool a_is_f32 = false, b_is_f32 = false;
    int64_t T = 0, C = 0;          // rows and cells of both sources
    int64_t ld_a = 0, ld_b = 0;    // elements between two rows of a source (>= C)
    int64_t M = 0;                 // bins
    int nstat = 0;                 // statistics asked for
    int stats[sdsk::kMaxStats] = {0, 0, 0, 0, 0, 0, 0};  // their codes, the first nstat are read
    int64_t ld_out = 0;            // elements between two rows of an output field (>= C)
    int64_t stride_out = 0;        // elements between the output fields of two statistics (>= M * ld_out)
    bool a_aligned16 = true, b_aligned16 = true, out_aligned16 = true;  // the pointers are multiples of 16 bytes
};

using SkillPlan = sdbn::BinsPlan;

// offsets [M + 1]: a host array
inline SkillPlan skill_plan(const SkillCall& c, const int64_t* offsets) {
    using namespace sdsk;
    const char* const who = "sd_skill";
    SkillPlan pl;
    for (int s = 0; s < c.nstat && s < kMaxStats; ++s)
        if (c.stats[s] < SD_SKILL_COUNT || c.stats[s] > SD_SKILL_STD_RATIO)
            return fail(pl, SD_ERR_INVALID, "%s: unknown statistic code %d (stats[%d])", who, c.stats[s], s);
    if (c.nstat < 1 || c.nstat > kMaxStats) return fail(pl, SD_ERR_INVALID, "%s: nstat = %d, expected 1 to %d statistics", who, c.nstat, kMaxStats);
    if (!(c.T > 0 && c.C > 0 && c.M > 0))
        return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld, M=%lld)", who, (long long)c.T, (long long)c.C, (long long)c.M);
    if (c.T >= (int64_t)1 << 31) return fail(pl, SD_ERR_INVALID, "%s: T = %lld steps, the counts are int32 (T < 2^31)", who, (long long)c.T);
    if (c.ld_a < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld_a = %lld is less than the %lld cells of a row", who, (long long)c.ld_a, (long long)c.C);
    if (c.ld_b < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld_b = %lld is less than the %lld cells of a row", who, (long long)c.ld_b, (long long)c.C);
    if (c.ld_out < c.C)
        return fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of every field stay far from the end of int64_t)
    if (c.M <= most / c.ld_out && c.stride_out < c.M * c.ld_out)
        return fail(pl, SD_ERR_INVALID, "%s: stride_out = %lld is less than the %lld elements of one statistic (M * ld_out)", who,
                    (long long)c.stride_out, (long long)(c.M * c.ld_out));
    if (c.T > most / c.ld_a || c.T > most / c.ld_b || c.M > most / c.ld_out || c.stride_out > most / c.nstat)
        return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    pl = check_offsets(pl, who, offsets, c.M, "T", c.T);
    if (pl.error != SD_OK) return pl;
    // cols divides C and every leading dimension and stride: an access of cols cells is whole and aligned in every row of every field
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld_a % cols == 0 && c.ld_b % cols == 0 && c.ld_out % cols == 0 && c.stride_out % cols == 0;
        return whole && c.a_aligned16 && c.b_aligned16 && c.out_aligned16;
    };
    return bins_plan(who, c.a_is_f32 && c.b_is_f32, c.C, c.M, fits);  // four cells per lane only where both sources are float32
}
