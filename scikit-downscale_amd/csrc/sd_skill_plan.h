// Launch plans of the paired skill calls (GridArray.compare(other).resample(time=rule).bias() / .rmse() / .corr() / ... and
// GridArray.compare(other).groupby("time.month").bias() ...: two [T, C] fields, cells fastest, walked in lock-step and summarised over
// bins of rows into nstat [M, C] fields), as pure host functions (no HIP header: tests/skill_plan_check.cpp and
// tests/skill_groups_plan_check.cpp compile this file with g++ alone).
//
// The bins are not computed here: pandas makes them on the host (skdownscale_amd/resample.py: time_bins) and hands over the table
// offsets [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].  A grouped call
// hands over group [T] instead (skdownscale_amd/groupby.py: group_labels): bin g is the rows t with group[t] == g in ascending t.
//
// skill_plan:         every refusal, in the order of the checks below -- codes, nstat, sizes, T, leading dimensions, stride, too large
//                     (skill_check), the table of bins (check_offsets, ending at T) -- then the geometry of skill_kernel (sd_skill.hip)
//                     from sd_bins_plan.h.  The launcher takes all of it from here.  offsets is read only after everything that depends
//                     on sizes and codes alone has passed.
// skill_groups_plan:  the same checks (skill_check with M = G), then G <= 0, then the ids (groupby_check_groups), then the geometry of
//                     skill_groups_kernel, which is that of groupby_reduce_plan: a group is a bin whose rows are not consecutive, and
//                     with G <= kFewGroups a wave takes one group instead of kBinsPerWave.  The row tables are groupby_tables'.
#pragma once
#include "sd_bins_plan.h"
#include "sd_groupby_plan.h"

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
using SkillGroupsPlan = GroupbyPlan;  // with bins_per_wave: whole groups of one wave (1 or kBinsPerWave)

namespace sdsk {
// the refusals that depend on codes and sizes alone; binned: M counts bins and belongs to the sizes (a grouped call refuses its G after
// these, in the words of the groupby plans)
template <class Plan>
Plan skill_check(Plan pl, const SkillCall& c, const char* who, bool binned) {
    for (int s = 0; s < c.nstat && s < kMaxStats; ++s)
        if (c.stats[s] < SD_SKILL_COUNT || c.stats[s] > SD_SKILL_STD_RATIO)
            return fail(pl, SD_ERR_INVALID, "%s: unknown statistic code %d (stats[%d])", who, c.stats[s], s);
    if (c.nstat < 1 || c.nstat > kMaxStats) return fail(pl, SD_ERR_INVALID, "%s: nstat = %d, expected 1 to %d statistics", who, c.nstat, kMaxStats);
    if (binned && !(c.T > 0 && c.C > 0 && c.M > 0))
        return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld, M=%lld)", who, (long long)c.T, (long long)c.C, (long long)c.M);
    if (!(c.T > 0 && c.C > 0)) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld)", who, (long long)c.T, (long long)c.C);
    if (c.T >= (int64_t)1 << 31) return fail(pl, SD_ERR_INVALID, "%s: T = %lld steps, the counts are int32 (T < 2^31)", who, (long long)c.T);
    if (c.ld_a < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld_a = %lld is less than the %lld cells of a row", who, (long long)c.ld_a, (long long)c.C);
    if (c.ld_b < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld_b = %lld is less than the %lld cells of a row", who, (long long)c.ld_b, (long long)c.C);
    if (c.ld_out < c.C)
        return fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of every field stay far from the end of int64_t)
    if (c.M <= most / c.ld_out && c.stride_out < c.M * c.ld_out)
        return fail(pl, SD_ERR_INVALID, "%s: stride_out = %lld is less than the %lld elements of one statistic (%s * ld_out)", who,
                    (long long)c.stride_out, (long long)(c.M * c.ld_out), binned ? "M" : "G");
    if (c.T > most / c.ld_a || c.T > most / c.ld_b || c.M > most / c.ld_out || c.stride_out > most / c.nstat)
        return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    return pl;
}

// cols divides C and every leading dimension and stride: an access of cols cells is whole and aligned in every row of every field
inline bool skill_fits(const SkillCall& c, int cols) {
    const bool whole = c.C % cols == 0 && c.ld_a % cols == 0 && c.ld_b % cols == 0 && c.ld_out % cols == 0 && c.stride_out % cols == 0;
    return whole && c.a_aligned16 && c.b_aligned16 && c.out_aligned16;
}
}  // namespace sdsk

// offsets [M + 1]: a host array
inline SkillPlan skill_plan(const SkillCall& c, const int64_t* offsets) {
    using namespace sdsk;
    const char* const who = "sd_skill";
    SkillPlan pl = skill_check(SkillPlan(), c, who, true);
    pl = check_offsets(pl, who, offsets, c.M, "T", c.T);
    if (pl.error != SD_OK) return pl;
    return bins_plan(who, c.a_is_f32 && c.b_is_f32, c.C, c.M, [&](int cols) { return skill_fits(c, cols); });  // four cells per lane only where both sources are float32
}

// group [T]: a host array; c.M is the number of groups G
inline SkillGroupsPlan skill_groups_plan(const SkillCall& c, const int32_t* group) {
    using namespace sdsk;
    const char* const who = "sd_skill_groups";
    SkillGroupsPlan pl = skill_check(SkillGroupsPlan(), c, who, false);
    if (pl.error != SD_OK) return pl;
    if (c.M <= 0) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld)", who, (long long)c.M);
    pl = groupby_check_groups(pl, who, group, c.T, c.M);
    if (pl.error != SD_OK) return pl;
    return sdgb::geometry(pl, who, c.a_is_f32 && c.b_is_f32, c.C, c.M, c.M <= sdgb::kFewGroups ? 1 : kBinsPerWave,
                          [&](int cols) { return skill_fits(c, cols); });
}
