// Launch plan of a temporal disaggregation call (GridArray.disaggregate: a monthly [M, C] field turned into a daily [Tout, C] field by
// borrowing, for every output day, one row of the daily observations [To, C] and shifting or scaling the borrowed month so that its
// monthly statistic equals the target), as pure host functions (no HIP header: tests/disagg_plan_check.cpp compiles this file with g++
// alone).
//
// The calendar is not computed here: pandas makes it on the host (skdownscale_amd/disagg.py: time_map) and hands over two tables,
// src_row [Tout] -- the row of the observations every output row borrows -- and offsets [M + 1], bin m = output rows
// offsets[m] .. offsets[m + 1] - 1 (the rules of resample_check_offsets, with Tout for T).
//
// disagg_plan:          the geometry of disagg_kernel (sd_disagg.hip) from the sizes of the call -- grid, block, cells per lane, bins per
//                       workgroup -- and every refusal that depends only on sizes and codes.  The launcher takes all of it from here.
//                       The kernel keeps nothing in LDS and its grid does not depend on the CU count.
// disagg_check_tables:  the refusals of the tables themselves: offsets starts at 0, never decreases and ends at Tout; every src_row lies
//                       in [0, To) and every group id in [0, G), so that every row the kernel reads lies inside its field.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"

namespace sddg {
constexpr int kLanes = 64;
constexpr int kWaves = 4;         // waves of a workgroup: the same cells, consecutive runs of bins
constexpr int kBinsPerWave = 2;   // whole bins of one wave, one after the other
constexpr int kBatch = 8;         // rows whose loads are in flight before their arithmetic
constexpr int kBinsPerGroup = kWaves * kBinsPerWave;  // bins of a workgroup
constexpr int64_t kGridLimit = (int64_t)1 << 31;
}  // namespace sddg

struct DisaggCall {
    int op = SD_DISAGG_SHIFT;
    bool obs_is_f32 = false;
    int64_t To = 0, C = 0;     // rows and cells of the observations
    int64_t Tout = 0, M = 0;   // output rows and bins (rows of the target)
    int64_t ld_t = 0, ld_obs = 0, ld_out = 0;  // elements between two rows of the target, the observations and the output (>= C)
    bool has_climo = false, has_group = false;
    int64_t G = 0, ld_c = 0;   // rows of the climatology and elements between two of them (read only with has_climo)
    // the target, observation, output and climatology pointers are multiples of 16 bytes
    bool target_aligned16 = true, obs_aligned16 = true, out_aligned16 = true, climo_aligned16 = true;
};

struct DisaggPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int cols = 0;       // adjacent cells of a lane: one load of cols observations and one store of cols doubles per row
    int block = 0;      // threads of a workgroup
    int64_t ctiles = 0;      // cell tiles of kLanes * cols cells
    int64_t bin_groups = 0;  // runs of kBinsPerGroup bins
    int64_t blocks = 0;      // ctiles * bin_groups, cell tile fastest
};

namespace disagg_plan_detail {
template <class... A>
DisaggPlan fail(DisaggPlan pl, int code, const char* fmt, A... a) {
    snprintf(pl.message, sizeof pl.message, fmt, a...);
    pl.error = code;
    return pl;
}
}  // namespace disagg_plan_detail

inline DisaggPlan disagg_plan(const DisaggCall& c) {
    using namespace sddg;
    using disagg_plan_detail::fail;
    DisaggPlan pl;
    if (!(c.op == SD_DISAGG_SHIFT || c.op == SD_DISAGG_SCALE_MEAN || c.op == SD_DISAGG_SCALE_SUM))
        return fail(pl, SD_ERR_INVALID, "sd_disagg: unknown op code %d", c.op);
    if (!(c.To > 0 && c.C > 0 && c.Tout > 0 && c.M > 0))
        return fail(pl, SD_ERR_INVALID, "sd_disagg: bad sizes (To=%lld, C=%lld, Tout=%lld, M=%lld)", (long long)c.To, (long long)c.C,
                    (long long)c.Tout, (long long)c.M);
    if (c.has_climo != c.has_group)
        return fail(pl, SD_ERR_INVALID, "sd_disagg: %s", c.has_climo ? "climo without group" : "group without climo");
    if (c.has_climo && c.G <= 0) return fail(pl, SD_ERR_INVALID, "sd_disagg: bad sizes (G=%lld)", (long long)c.G);
    const struct {
        const char* name;
        int64_t ld;
        bool used;
    } lds[] = {{"ld_t", c.ld_t, true}, {"ld_obs", c.ld_obs, true}, {"ld_out", c.ld_out, true}, {"ld_c", c.ld_c, c.has_climo}};
    for (const auto& l : lds)
        if (l.used && l.ld < c.C)
            return fail(pl, SD_ERR_INVALID, "sd_disagg: %s = %lld is less than the %lld cells of a row", l.name, (long long)l.ld, (long long)c.C);
    const int64_t most = INT64_MAX / 8;  // (element indices of every field stay far from the end of int64_t)
    if (c.To > most / c.ld_obs || c.Tout > most / c.ld_out || c.M > most / c.ld_t || (c.has_climo && c.G > most / c.ld_c))
        return fail(pl, SD_ERR_INVALID, "%s", "sd_disagg: field too large");
    // cols cells per lane: every load of cols elements and every store of cols doubles is made of aligned accesses of up to 16 bytes
    // (four doubles go as two 16-byte halves), in every row -- so cols divides C and every leading dimension
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld_t % cols == 0 && c.ld_obs % cols == 0 && c.ld_out % cols == 0 && (!c.has_climo || c.ld_c % cols == 0);
        return whole && c.target_aligned16 && c.obs_aligned16 && c.out_aligned16 && (!c.has_climo || c.climo_aligned16);
    };
    pl.cols = (c.obs_is_f32 && fits(4)) ? 4 : fits(2) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.ctiles = (c.C - 1) / (kLanes * pl.cols) + 1;
    pl.bin_groups = (c.M - 1) / kBinsPerGroup + 1;
    if (pl.bin_groups > (kGridLimit - 1) / pl.ctiles)  // blocks < 2^31
        return fail(pl, SD_ERR_INVALID, "%s", "sd_disagg: grid too large");
    pl.blocks = pl.ctiles * pl.bin_groups;
    return pl;
}

// the tables of a call that disagg_plan accepted: src_row [Tout], offsets [M + 1], group [M] (NULL without a climatology)
inline DisaggPlan disagg_check_tables(DisaggPlan pl, const DisaggCall& c, const int64_t* src_row, const int64_t* offsets, const int32_t* group) {
    using disagg_plan_detail::fail;
    if (pl.error != SD_OK) return pl;
    if (offsets[0] != 0) return fail(pl, SD_ERR_INVALID, "sd_disagg: offsets[0] = %lld, expected 0", (long long)offsets[0]);
    for (int64_t m = 0; m < c.M; ++m)
        if (offsets[m + 1] < offsets[m])
            return fail(pl, SD_ERR_INVALID, "sd_disagg: offsets decrease at bin %lld (%lld after %lld)", (long long)m, (long long)offsets[m + 1],
                        (long long)offsets[m]);
    if (offsets[c.M] != c.Tout)
        return fail(pl, SD_ERR_INVALID, "sd_disagg: offsets[M] = %lld, expected Tout = %lld", (long long)offsets[c.M], (long long)c.Tout);
    for (int64_t t = 0; t < c.Tout; ++t)
        if (src_row[t] < 0 || src_row[t] >= c.To)
            return fail(pl, SD_ERR_INVALID, "sd_disagg: src_row[%lld] = %lld lies outside the %lld rows of obs", (long long)t, (long long)src_row[t],
                        (long long)c.To);
    if (c.has_group)
        for (int64_t m = 0; m < c.M; ++m)
            if (group[m] < 0 || group[m] >= c.G)
                return fail(pl, SD_ERR_INVALID, "sd_disagg: group[%lld] = %d lies outside the %lld rows of climo", (long long)m, (int)group[m],
                            (long long)c.G);
    return pl;
}
