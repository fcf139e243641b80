// Launch plans of the two groupby calls (GridArray.groupby: a [T, C] field, cells fastest, whose rows carry a group id in [0, G)), as
// pure host functions (no HIP header: tests/groupby_plan_check.cpp compiles this file with g++ alone).
//   reduce: the rows of a group are added, in row order, onto row g of the accumulators sum / count [G, C]  (.mean() / .sum())
//   apply:  out[t, c] = src[t, c] (op) table[group[t], c]                                                    (gb - clim, gb / clim, ...)
//
// The labels are not computed here: pandas and NumPy make them on the host (skdownscale_amd/groupby.py: group_labels) and hand over
// group [T].
//
// groupby_reduce_plan:   every refusal that depends only on sizes and codes, then the geometry of groupby_reduce_kernel (sd_groupby.hip)
//                        from sd_bins_plan.h: a group is a bin whose rows are not consecutive.  With few groups a wave takes one bin
//                        instead of kBinsPerWave (bins_per_wave): G = 12 fills three workgroups per cell tile instead of one and a
//                        half.  The constants of sd_bins_plan.h stay what they are.
// groupby_apply_plan:    the same for groupby_apply_kernel, whose bins are runs of kApplyRun consecutive rows.
// groupby_check_groups:  the refusal of the table itself: every id lies in [0, G), so that every accumulator or table row a kernel
//                        touches lies inside its field.
// groupby_tables:        group [T] as a stable counting sort: rows [T], the row numbers grouped by id, in row order inside a group, and
//                        offsets [G + 1], the bin table over them.
#pragma once
#include "sd_bins_plan.h"

namespace sdgb {
using namespace sdbn;  // the constants of these plans are the shared ones
constexpr int64_t kFewGroups = 2 * kBinsPerGroup;  // up to here a wave takes one bin
constexpr int kApplyRun = 2 * kBatch;              // rows of one bin of groupby_apply_kernel
}  // namespace sdgb

struct GroupbyReduceCall {
    int op = SD_GROUPBY_MEAN;
    bool src_is_f32 = false;
    int64_t T = 0, C = 0;      // rows and cells of the source
    int64_t ld = 0;            // elements between two rows of the source (>= C)
    int64_t G = 0;             // groups: rows of the accumulators and of the output
    int64_t ld_acc = 0;        // elements between two rows of sum and of count (>= C)
    bool has_out = false;
    int64_t ld_out = 0;        // elements between two rows of the output (>= C; read only with has_out)
    // the source, sum, count and output pointers are multiples of 16 bytes
    bool src_aligned16 = true, sum_aligned16 = true, count_aligned16 = true, out_aligned16 = true;
};

struct GroupbyApplyCall {
    int op = SD_GROUPBY_SUB;
    bool src_is_f32 = false;
    int64_t T = 0, C = 0, ld = 0;  // the source, as above
    int64_t G = 0, ld_t = 0;       // rows of the table and elements between two of them (>= C)
    int64_t ld_out = 0;            // elements between two rows of the output (>= C)
    bool src_aligned16 = true, table_aligned16 = true, out_aligned16 = true;
};

struct GroupbyPlan : sdbn::BinsPlan {
    int bins_per_wave = 0;  // reduce: whole groups of one wave (1 or kBinsPerWave); apply: runs of kApplyRun rows of one wave
};

namespace sdgb {
struct NamedLd {
    const char* name;
    int64_t ld;
    bool used;
};

template <size_t N>
GroupbyPlan check_lds(GroupbyPlan pl, const char* who, int64_t C, const NamedLd (&lds)[N]) {
    for (const NamedLd& l : lds)
        if (l.used && l.ld < C && pl.error == SD_OK)
            pl = fail(pl, SD_ERR_INVALID, "%s: %s = %lld is less than the %lld cells of a row", who, l.name, (long long)l.ld, (long long)C);
    return pl;
}

// the geometry of sd_bins_plan.h for `bins` bins of which a wave takes `per_wave` (which divides kBinsPerWave)
template <class Fits>
GroupbyPlan geometry(GroupbyPlan pl, const char* who, bool src_is_f32, int64_t C, int64_t bins, int per_wave, Fits fits) {
    // a workgroup of kWaves * per_wave bins: as many workgroups as bins * (kBinsPerWave / per_wave) bins make at kBinsPerGroup each
    const int64_t scale = kBinsPerWave / per_wave;
    if (bins > INT64_MAX / scale) return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    const BinsPlan g = bins_plan(who, src_is_f32, C, bins * scale, fits);
    static_cast<BinsPlan&>(pl) = g;
    pl.bins_per_wave = per_wave;
    return pl;
}
}  // namespace sdgb

inline GroupbyPlan groupby_reduce_plan(const GroupbyReduceCall& c) {
    using namespace sdgb;
    const char* const who = "sd_groupby_reduce";
    GroupbyPlan pl;
    if (!(c.op == SD_GROUPBY_MEAN || c.op == SD_GROUPBY_SUM)) return fail(pl, SD_ERR_INVALID, "%s: unknown op code %d", who, c.op);
    if (!(c.T > 0 && c.C > 0)) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld)", who, (long long)c.T, (long long)c.C);
    if (c.G <= 0) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld)", who, (long long)c.G);
    const NamedLd lds[] = {{"ld", c.ld, true}, {"ld_acc", c.ld_acc, true}, {"ld_out", c.ld_out, c.has_out}};
    pl = check_lds(pl, who, c.C, lds);
    if (pl.error != SD_OK) return pl;
    const int64_t most = INT64_MAX / 8;  // (element indices of every field stay far from the end of int64_t)
    if (c.T > most / c.ld || c.G > most / c.ld_acc || (c.has_out && c.G > most / c.ld_out)) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    // cols divides C and every leading dimension: an access of cols cells is whole and aligned in every row (cols counts: 4 * cols bytes)
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld % cols == 0 && c.ld_acc % cols == 0 && (!c.has_out || c.ld_out % cols == 0);
        return whole && c.src_aligned16 && c.sum_aligned16 && c.count_aligned16 && (!c.has_out || c.out_aligned16);
    };
    return geometry(pl, who, c.src_is_f32, c.C, c.G, c.G <= kFewGroups ? 1 : kBinsPerWave, fits);
}

inline GroupbyPlan groupby_apply_plan(const GroupbyApplyCall& c) {
    using namespace sdgb;
    const char* const who = "sd_groupby_apply";
    GroupbyPlan pl;
    if (!(c.op == SD_GROUPBY_SUB || c.op == SD_GROUPBY_ADD || c.op == SD_GROUPBY_MUL || c.op == SD_GROUPBY_DIV))
        return fail(pl, SD_ERR_INVALID, "%s: unknown op code %d", who, c.op);
    if (!(c.T > 0 && c.C > 0)) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld)", who, (long long)c.T, (long long)c.C);
    if (c.G <= 0) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld)", who, (long long)c.G);
    const NamedLd lds[] = {{"ld", c.ld, true}, {"ld_t", c.ld_t, true}, {"ld_out", c.ld_out, true}};
    pl = check_lds(pl, who, c.C, lds);
    if (pl.error != SD_OK) return pl;
    const int64_t most = INT64_MAX / 8;
    if (c.T > most / c.ld || c.T > most / c.ld_out || c.G > most / c.ld_t) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld % cols == 0 && c.ld_t % cols == 0 && c.ld_out % cols == 0;
        return whole && c.src_aligned16 && c.table_aligned16 && c.out_aligned16;
    };
    // at most two cells per lane, float32 sources included: with four, a lane's 32 bytes of table and of output are two 16-byte accesses 32
    // bytes apart, and the float32 kernel measured 4.61 ms against 3.77 ms with two (profiles/groupby/)
    return geometry(pl, who, /*four cells per lane=*/false, c.C, (c.T - 1) / kApplyRun + 1, kBinsPerWave, fits);
}

// group [T] of a call that a plan accepted
inline GroupbyPlan groupby_check_groups(GroupbyPlan pl, const char* who, const int32_t* group, int64_t T, int64_t G) {
    if (pl.error != SD_OK) return pl;
    for (int64_t t = 0; t < T; ++t)
        if (group[t] < 0 || group[t] >= G)
            return sdbn::fail(pl, SD_ERR_INVALID, "%s: group[%lld] = %d lies outside the %lld groups", who, (long long)t, (int)group[t], (long long)G);
    return pl;
}

// group [T] with every id in [0, G) -> rows [T], offsets [G + 1]: the rows of group g are rows[offsets[g]] .. rows[offsets[g + 1] - 1],
// ascending (a stable counting sort)
inline void groupby_tables(const int32_t* group, int64_t T, int64_t G, int64_t* rows, int64_t* offsets) {
    for (int64_t g = 0; g <= G; ++g) offsets[g] = 0;
    for (int64_t t = 0; t < T; ++t) ++offsets[group[t] + 1];
    for (int64_t g = 0; g < G; ++g) offsets[g + 1] += offsets[g];
    for (int64_t t = 0; t < T; ++t) rows[offsets[group[t]]++] = t;  // (offsets[g] is now the end of group g: the start of g + 1)
    for (int64_t g = G; g > 0; --g) offsets[g] = offsets[g - 1];
    offsets[0] = 0;
}
