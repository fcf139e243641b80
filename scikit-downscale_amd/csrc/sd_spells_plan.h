// Launch plan of a threshold / spell index call (GridArray.where(op, threshold).resample(time=rule).count() / .longest_spell() / ...:
// a [T, C] field, cells fastest, compared per step with a threshold and summarised over runs of consecutive rows into nstat [M, C]
// fields), as pure host functions (no HIP header: tests/spells_plan_check.cpp compiles this file with g++ alone).
//
// The bins are not computed here: pandas makes them on the host (skdownscale_amd/resample.py: time_bins) and hands over the table
// offsets [M + 1], bin m = rows offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].  The threshold is a
// scalar, or row group[r] of a [G, C] table for row r of the field (group NULL with G == 1: row 0 for every row -- a per-cell
// threshold).
//
// spells_plan:  every refusal, in the order of the checks below -- codes, sizes, leading dimensions, the group ids
//               (groupby_check_groups), the table of bins (check_offsets, ending at T) -- then the geometry of spells_kernel
//               (sd_spells.hip) from sd_bins_plan.h.  The launcher takes all of it from here.  group and offsets are read only after
//               everything that depends on sizes and codes alone has passed.
#pragma once
#include "sd_bins_plan.h"
#include "sd_groupby_plan.h"

namespace sdsp {
using namespace sdbn;  // the constants of this plan are the shared ones
constexpr int kMaxStats = SD_SPELL_SPELL_COUNT + 1;  // statistics of one call at the most (a code may repeat)
}

struct SpellsCall {
    int op = SD_SPELL_GT;
    bool src_is_f32 = false;
    int64_t T = 0, C = 0;      // rows and cells of the source
    int64_t ld = 0;            // elements between two rows of the source (>= C)
    bool has_table = false;    // the threshold is a table [G, C] (else a scalar: ld_t and G are not read, group must not matter)
    int64_t G = 1, ld_t = 0;   // rows of the table and elements between two of them (>= C)
    bool has_group = false;    // group [T] is given (required where G > 1)
    int64_t M = 0;             // bins
    int64_t min_length = 1;    // L: steps a run of hits needs to count as a spell
    int nstat = 0;             // statistics asked for
    int stats[sdsp::kMaxStats] = {0, 0, 0, 0, 0, 0};  // their codes, the first nstat are read
    int64_t ld_out = 0;        // elements between two rows of an output field (>= C)
    int64_t stride_out = 0;    // elements between the output fields of two statistics (>= M * ld_out)
    bool src_aligned16 = true, table_aligned16 = true, out_aligned16 = true;  // the pointers are multiples of 16 bytes
};

using SpellsPlan = sdbn::BinsPlan;

// group [T] or NULL, offsets [M + 1]: host arrays
inline SpellsPlan spells_plan(const SpellsCall& c, const int32_t* group, const int64_t* offsets) {
    using namespace sdsp;
    const char* const who = "sd_spells";
    SpellsPlan pl;
    if (!(c.op == SD_SPELL_GT || c.op == SD_SPELL_GE || c.op == SD_SPELL_LT || c.op == SD_SPELL_LE))
        return fail(pl, SD_ERR_INVALID, "%s: unknown op code %d", who, c.op);
    for (int s = 0; s < c.nstat && s < kMaxStats; ++s)
        if (c.stats[s] < SD_SPELL_VALID || c.stats[s] > SD_SPELL_SPELL_COUNT)
            return fail(pl, SD_ERR_INVALID, "%s: unknown statistic code %d (stats[%d])", who, c.stats[s], s);
    if (c.nstat < 1 || c.nstat > kMaxStats) return fail(pl, SD_ERR_INVALID, "%s: nstat = %d, expected 1 to %d statistics", who, c.nstat, kMaxStats);
    if (c.min_length < 1) return fail(pl, SD_ERR_INVALID, "%s: min_length = %lld, expected at least 1", who, (long long)c.min_length);
    if (!(c.T > 0 && c.C > 0 && c.M > 0))
        return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld, M=%lld)", who, (long long)c.T, (long long)c.C, (long long)c.M);
    if (c.T >= (int64_t)1 << 31) return fail(pl, SD_ERR_INVALID, "%s: T = %lld steps, the counts are int32 (T < 2^31)", who, (long long)c.T);
    if (c.ld < c.C) return fail(pl, SD_ERR_INVALID, "%s: ld = %lld is less than the %lld cells of a row", who, (long long)c.ld, (long long)c.C);
    if (c.has_table && c.ld_t < c.C)
        return fail(pl, SD_ERR_INVALID, "%s: ld_t = %lld is less than the %lld cells of a row", who, (long long)c.ld_t, (long long)c.C);
    if (c.ld_out < c.C)
        return fail(pl, SD_ERR_INVALID, "%s: ld_out = %lld is less than the %lld cells of a row", who, (long long)c.ld_out, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of every field stay far from the end of int64_t)
    if (c.M <= most / c.ld_out && c.stride_out < c.M * c.ld_out)
        return fail(pl, SD_ERR_INVALID, "%s: stride_out = %lld is less than the %lld elements of one statistic (M * ld_out)", who,
                    (long long)c.stride_out, (long long)(c.M * c.ld_out));
    if (c.T > most / c.ld || c.M > most / c.ld_out || c.stride_out > most / c.nstat) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    if (c.has_table) {
        if (c.G < 1) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld)", who, (long long)c.G);
        if (c.G > most / c.ld_t) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
        if (c.G > 1 && !c.has_group) return fail(pl, SD_ERR_INVALID, "%s: a table of %lld rows needs group ids (group is NULL)", who, (long long)c.G);
        if (c.has_group) {
            const GroupbyPlan g = groupby_check_groups(GroupbyPlan(), who, group, c.T, c.G);
            if (g.error != SD_OK) return fail(pl, g.error, "%s", g.message);
        }
    }
    pl = check_offsets(pl, who, offsets, c.M, "T", c.T);
    if (pl.error != SD_OK) return pl;
    // cols divides C and every leading dimension and stride: an access of cols cells is whole and aligned in every row of every field
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld % cols == 0 && c.ld_out % cols == 0 && c.stride_out % cols == 0;
        const bool table = !c.has_table || (c.ld_t % cols == 0 && c.table_aligned16);
        return whole && table && c.src_aligned16 && c.out_aligned16;
    };
    return bins_plan(who, c.src_is_f32, c.C, c.M, fits);
}
