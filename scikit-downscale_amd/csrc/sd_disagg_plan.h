// Launch plan of a temporal disaggregation call (GridArray.disaggregate: a monthly [M, C] field turned into a daily [Tout, C] field by
// borrowing, for every output day, one row of the daily observations [To, C] and shifting or scaling the borrowed month so that its
// monthly statistic equals the target), as pure host functions (no HIP header: tests/disagg_plan_check.cpp compiles this file with g++
// alone).
//
// The calendar is not computed here: pandas makes it on the host (skdownscale_amd/disagg.py: time_map) and hands over two tables,
// src_row [Tout] -- the row of the observations every output row borrows -- and offsets [M + 1], bin m = output rows
// offsets[m] .. offsets[m + 1] - 1.
//
// disagg_plan:          every refusal that depends only on sizes and codes, then the geometry of disagg_kernel (sd_disagg.hip) from
//                       sd_bins_plan.h.  The launcher takes all of it from here.
// disagg_check_tables:  the refusals of the tables themselves: offsets by sd_bins_plan.h's check_offsets, ending at Tout; every src_row
//                       lies in [0, To) and every group id in [0, G), so that every row the kernel reads lies inside its field.
#pragma once
#include "sd_bins_plan.h"

namespace sddg {
using namespace sdbn;  // the constants of this plan are the shared ones
}

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

using DisaggPlan = sdbn::BinsPlan;

inline DisaggPlan disagg_plan(const DisaggCall& c) {
    using sdbn::fail;
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
    // cols divides C and every leading dimension: an access of cols cells is whole and aligned in every row
    const auto fits = [&](int cols) {
        const bool whole = c.C % cols == 0 && c.ld_t % cols == 0 && c.ld_obs % cols == 0 && c.ld_out % cols == 0 && (!c.has_climo || c.ld_c % cols == 0);
        return whole && c.target_aligned16 && c.obs_aligned16 && c.out_aligned16 && (!c.has_climo || c.climo_aligned16);
    };
    return sdbn::bins_plan("sd_disagg", c.obs_is_f32, c.C, c.M, fits);
}

// the tables of a call that disagg_plan accepted: src_row [Tout], offsets [M + 1], group [M] (NULL without a climatology)
inline DisaggPlan disagg_check_tables(DisaggPlan pl, const DisaggCall& c, const int64_t* src_row, const int64_t* offsets, const int32_t* group) {
    using sdbn::fail;
    pl = sdbn::check_offsets(pl, "sd_disagg", offsets, c.M, "Tout", c.Tout);
    if (pl.error != SD_OK) return pl;
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
