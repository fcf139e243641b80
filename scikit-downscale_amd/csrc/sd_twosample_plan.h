// Launch plan of a two-sample call (GridArray.compare(other).ks() / .perkins(width): the Kolmogorov-Smirnov distance and the Perkins
// skill score of two [T, C] fields per cell and bin of consecutive rows), as pure host functions (no HIP header:
// tests/twosample_plan_check.cpp compiles this file with g++ alone).  The bins are those of sd_skill: pandas makes them on the host and
// hands over offsets [M + 1]; the table check is the shared one of sd_bins_plan.h.
//
// twosample_plan: every refusal, in this order -- statistic codes, nstat; width and origin (only where Perkins is asked for); sizes,
//                 T; leading dimensions, stride; field too large; the table of bins; a bin beyond the workgroup merge
//                 (SD_ERR_UNSUPPORTED); the LDS, the grids, the 32-bit row addressing -- then the path and the geometry.  offsets is read
//                 only after everything that depends on sizes and codes alone has passed.
//
// Segment path (n_max <= 64 * K for the widest K of kSegWidths): twosample_segment_kernel<SA, SB, K>, one 512-thread workgroup = 8
// adjacent cells x one bin, both fields' rows in two LDS rows per cell, both sorted by the wave that owns the cell.  Two fields double
// the tile of the quantile kernel: 2 * 8 * 8 * tile_sort_rs(K) + 8 * kHeadDoubles bytes have to fit the 160 KB of a CU, which K = 21
// (173 KB) does not; K = 19 does (156 608 B, one workgroup per CU), K = 13 takes 107 456 B (one per CU), K = 7 takes 58 304 B (two) and
// K = 5 takes 41 920 B (three).  The widths are odd for the stride-K reads of sort_row.  K = 7 is there for yearly bins (366 rows <=
// 448): the sorts are chains of LDS round trips that more resident waves hide, so two workgroups per CU instead of the one of K = 13,
// and 53 busy lanes of a wave instead of 29, are worth an instantiation.
//
// Series path (64 * 19 < n_max <= 19 456): quantile_runs_kernel<S, Kt> once per field, with the chunk tables of sd_quantile_plan.h
// (scratch 8 * C * run_slots bytes and 4 * C * chunks bytes per field), then twosample_select_kernel<Kt>, one 1 024-thread workgroup per
// (bin, cell): the two sorted series are never in LDS together, so its LDS is block_sort_lds_bytes(np_max), that of
// quantile_select_kernel.
#pragma once
#include <cmath>
#include <vector>

#include "sd_bins_plan.h"
#include "sd_quantile_plan.h"
#include "sd_wave_consts.h"

namespace sdts {
constexpr int kSegWidths[] = {5, 7, 13, 19};  // twosample_segment_kernel<SA, SB, K>
constexpr int kMaxStats = SD_TWOSAMPLE_NB + 1;  // statistics of one call at the most (a code may repeat)
constexpr int kSegment = 0, kSeries = 1;
using sdqt::kGridLimit;
using sdqt::kSeriesLimit;

inline int seg_width(int64_t n_max) {
    for (int K : kSegWidths)
        if (n_max <= (int64_t)sdw::kWave * K) return K;
    return 0;
}
// two tiles of 8 rows behind one head
inline size_t seg_lds_bytes(int K) { return sizeof(double) * ((size_t)2 * sdw::kW * sdw::tile_sort_rs(K) + sdw::kHeadDoubles); }
}  // namespace sdts

struct TwosampleCall {
    bool a_is_f32 = false, b_is_f32 = false;
    int64_t T = 0, C = 0;          // rows and cells of both sources
    int64_t ld_a = 0, ld_b = 0;    // elements between two rows of a source (>= C)
    int64_t M = 0;                 // bins
    int nstat = 0;                 // statistics asked for
    int stats[sdts::kMaxStats] = {0, 0, 0, 0};  // their codes, the first nstat are read
    double width = 0.0, origin = 0.0;  // the histogram of SD_TWOSAMPLE_PERKINS (read only where it is among the codes)
    int64_t ld_out = 0;            // elements between two rows of an output field (>= C)
    int64_t stride_out = 0;        // elements between the output fields of two statistics (>= M * ld_out)
    bool a_aligned16 = true, b_aligned16 = true;  // the source pointers are multiples of 16 bytes
    size_t lds_max = 160 * 1024;
    int cu_count = 256;
};

struct TwosamplePlan {
    int error = SD_OK;
    char message[256] = "";
    int64_t n_max = 0;      // rows of the longest bin
    int path = sdts::kSegment;
    int K = 0;              // width of the path's sort
    bool vec_a = false, vec_b = false;  // 16-byte loads of a source (8-byte ones of a float32 source)
    int rs = 0;             // doubles between two LDS rows
    size_t lds = 0;         // dynamic LDS bytes of a workgroup: twosample_segment_kernel, or quantile_runs_kernel of the series path
    int per_cu = 0;         // workgroups of a CU by LDS and by threads
    int64_t ntiles = 0;     // tiles of 8 cells
    int64_t blocks = 0;     // 8 * ceil(ntiles / 8) * (M | chunks)
    // series path
    int64_t chunks = 0;     // chunks of all bins
    int64_t run_slots = 0;  // slots per cell of one field's runs scratch
    int np_max = 0;
    size_t select_lds = 0;
    int64_t select_blocks = 0;
};

namespace sdts {
// the refusals that depend on codes and sizes alone; binned: M counts bins and belongs to the sizes (a grouped call refuses its G after
// these, in the words of the groupby plans)
inline TwosamplePlan twosample_check(const TwosampleCall& c, const char* who, bool binned) {
    using sdbn::fail;
    TwosamplePlan pl;
    bool perkins = false;
    for (int s = 0; s < c.nstat && s < kMaxStats; ++s) {
        if (c.stats[s] < SD_TWOSAMPLE_KS || c.stats[s] > SD_TWOSAMPLE_NB)
            return fail(pl, SD_ERR_INVALID, "%s: unknown statistic code %d (stats[%d])", who, c.stats[s], s);
        perkins = perkins || c.stats[s] == SD_TWOSAMPLE_PERKINS;
    }
    if (c.nstat < 1 || c.nstat > kMaxStats) return fail(pl, SD_ERR_INVALID, "%s: nstat = %d, expected 1 to %d statistics", who, c.nstat, kMaxStats);
    if (perkins && !(std::isfinite(c.width) && c.width > 0.0))
        return fail(pl, SD_ERR_INVALID, "%s: width = %g, expected a positive finite bin width", who, c.width);
    if (perkins && !std::isfinite(c.origin)) return fail(pl, SD_ERR_INVALID, "%s: origin = %g, expected a finite number", who, c.origin);
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

// offsets [M + 1] of a call that twosample_check accepted, a table that starts at 0, never decreases and ends at T: the longest bin (what:
// "bin" or "group" in the refusal) chooses the path and its width, then the refusals that depend on them
inline TwosamplePlan twosample_geometry(TwosamplePlan pl, const TwosampleCall& c, const int64_t* offsets, const char* who, const char* what) {
    using sdbn::fail;
    if (pl.error != SD_OK) return pl;
    for (int64_t m = 0; m < c.M; ++m)
        if (offsets[m + 1] - offsets[m] > pl.n_max) pl.n_max = offsets[m + 1] - offsets[m];
    if (pl.n_max > kSeriesLimit)
        return fail(pl, SD_ERR_UNSUPPORTED, "%s: a %s of %lld samples exceeds the workgroup merge (%lld)", who, what, (long long)pl.n_max,
                    (long long)kSeriesLimit);
    pl.vec_a = c.ld_a % 2 == 0 && c.a_aligned16;
    pl.vec_b = c.ld_b % 2 == 0 && c.b_aligned16;
    pl.ntiles = (c.C + sdw::kW - 1) / sdw::kW;
    const int64_t tx8 = 8 * ((pl.ntiles + 7) / 8);
    pl.K = seg_width(pl.n_max);
    int64_t items = c.M;
    if (pl.K != 0) {
        pl.path = kSegment;
        pl.lds = seg_lds_bytes(pl.K);
    } else {
        pl.path = kSeries;
        pl.K = sdqt::series_width(pl.n_max);
        const int chunk = sdw::kWave * pl.K;
        for (int64_t m = 0; m < c.M; ++m) {
            const int64_t nch = (offsets[m + 1] - offsets[m] + chunk - 1) / chunk;
            pl.chunks += nch, pl.run_slots += nch * chunk;
            if (nch * chunk > pl.np_max) pl.np_max = (int)(nch * chunk);
        }
        items = pl.chunks;
        pl.lds = sdw::tile_sort_lds_bytes(pl.K);
        pl.select_lds = sdw::block_sort_lds_bytes(pl.np_max);
    }
    pl.rs = sdw::tile_sort_rs(pl.K);
    pl.per_cu = sdqt::per_cu(pl.lds, c.lds_max, sdw::kThreads);
    if (pl.lds > c.lds_max)
        return pl.path == kSegment ? fail(pl, SD_ERR_UNSUPPORTED, "%s: two tiles of %d-row segments (%zu bytes) do not fit the LDS (%zu)", who,
                                          sdw::kWave * pl.K, pl.lds, c.lds_max)
                                   : fail(pl, SD_ERR_UNSUPPORTED, "%s: a tile of %d-row runs (%zu bytes) does not fit the LDS (%zu)", who,
                                          sdw::kWave * pl.K, pl.lds, c.lds_max);
    if (pl.select_lds > c.lds_max) return fail(pl, SD_ERR_UNSUPPORTED, "%s: the merge of %d slots does not fit the LDS", who, pl.np_max);
    if (pl.path == kSeries) {
        if (c.M > (kGridLimit - 1) / c.C) return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
        if (pl.run_slots > INT64_MAX / 8 / c.C) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
        const int64_t cap = (int64_t)c.cu_count * 4;
        pl.select_blocks = c.M * c.C < cap ? c.M * c.C : cap;
    }
    if (items > (kGridLimit - 1) / tx8) return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = tx8 * items;
    if (c.ld_a >= ((int64_t)1 << 29) || c.ld_b >= ((int64_t)1 << 29))
        return fail(pl, SD_ERR_INVALID, "%s: rows of %lld and %lld elements exceed the 32-bit row addressing", who, (long long)c.ld_a,
                    (long long)c.ld_b);
    return pl;
}
}  // namespace sdts

// offsets [M + 1]: a host array
inline TwosamplePlan twosample_plan(const TwosampleCall& c, const int64_t* offsets) {
    using namespace sdts;
    using sdbn::fail;
    const char* const who = "sd_twosample";
    TwosamplePlan pl = twosample_check(c, who, true);
    if (pl.error != SD_OK) return pl;
    const sdbn::BinsPlan table = sdbn::check_offsets(sdbn::BinsPlan(), who, offsets, c.M, "T", c.T);
    if (table.error != SD_OK) return fail(pl, table.error, "%s", table.message);
    return twosample_geometry(pl, c, offsets, who, "bin");
}

// group [T]: a host array; c.M is the number of groups G.  rows [T] and offsets [G + 1] receive the tables of groupby_tables (the row
// table of gather_tile and the bins over it) once the ids have passed; they are not written by a refused call before that.
inline TwosamplePlan twosample_groups_plan(const TwosampleCall& c, const int32_t* group, std::vector<int64_t>* rows, std::vector<int64_t>* offsets) {
    using namespace sdts;
    using sdbn::fail;
    const char* const who = "sd_twosample_groups";
    TwosamplePlan pl = twosample_check(c, who, false);
    if (pl.error != SD_OK) return pl;
    if (c.M <= 0) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld)", who, (long long)c.M);
    const GroupbyPlan ids = groupby_check_groups(GroupbyPlan(), who, group, c.T, c.M);
    if (ids.error != SD_OK) return fail(pl, ids.error, "%s", ids.message);
    rows->assign((size_t)c.T, 0), offsets->assign((size_t)c.M + 1, 0);
    groupby_tables(group, c.T, c.M, rows->data(), offsets->data());
    return twosample_geometry(pl, c, offsets->data(), who, "group");
}

// what the plan chose, in words (tests/twosample_plan_check.cpp prints it)
inline void twosample_describe(const TwosamplePlan& pl, char* buf, size_t size) {
    if (pl.path == sdts::kSegment)
        snprintf(buf, size, "segment path: n_max=%lld K=%d rs=%d lds=%zu per_cu=%d blocks=%lld vec_a=%d vec_b=%d", (long long)pl.n_max, pl.K, pl.rs,
                 pl.lds, pl.per_cu, (long long)pl.blocks, (int)pl.vec_a, (int)pl.vec_b);
    else
        snprintf(buf, size,
                 "series path: n_max=%lld K=%d chunks=%lld run_slots=%lld lds=%zu per_cu=%d blocks=%lld select_lds=%zu select_blocks=%lld vec_a=%d "
                 "vec_b=%d",
                 (long long)pl.n_max, pl.K, (long long)pl.chunks, (long long)pl.run_slots, pl.lds, pl.per_cu, (long long)pl.blocks, pl.select_lds,
                 (long long)pl.select_blocks, (int)pl.vec_a, (int)pl.vec_b);
}
