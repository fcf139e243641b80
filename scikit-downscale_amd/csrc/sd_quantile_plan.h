// Launch plan of a quantile call (GridArray.quantile / .median: np.nanquantile / np.nanmedian per cell and group of a [T, C] field,
// cells fastest, whose rows carry a group id in [0, G)), as pure host functions (no HIP header: tests/quantile_plan_check.cpp compiles
// this file with g++ alone).  The ids come from the host as for sd_groupby_plan.h, whose groupby_check_groups / groupby_tables make
// the row table here too.
//
// quantile_check:   every refusal that depends only on sizes and codes, in this order: method; sizes; G, Q; q range; leading
//                   dimensions; field too large.
// quantile_groups:  the refusal of the ids (groupby_check_groups).
// quantile_plan:    from the group table offsets [G + 1]: the longest group n_max chooses the path and its width, then the refusals
//                   that depend on them: n_max beyond the series path (SD_ERR_UNSUPPORTED); the 2^31 grid limits; 8 * ld < 2^32 and
//                   T < 2^31 (the row addresses of the kernels are one 32 x 32 -> 64 bit multiply, sdw::row_of).
//
// Segment path (n_max <= 64 * K for the widest width K of kSegWidths): quantile_segment_kernel<S, K>, one 512-thread workgroup = 8
// adjacent cells x one group, one wave sorts one cell (sdw::sort_segment<K>) and its lanes evaluate the Q quantiles.  The narrowest
// width that holds n_max serves the call: 366 day-of-year groups of ~40 samples run at K = 5 (21 KB of LDS, 7 workgroups per CU by
// LDS), monthly groups of 40 years of daily data (1 240 samples) at K = 21 (84 KB, one workgroup per CU).  The widths are odd: a lane
// reads its K consecutive samples from the LDS row at a stride of K doubles, which is free of bank conflicts for odd K only.
//
// Series path (64 * 21 < n_max <= 19 456): quantile_runs_kernel<S, Kt> sorts chunks of 64 * Kt rows of a group's row table per wave
// (the tile shape of the segment path) into runs [group][cell][np_g] of device scratch, NaN counted per (chunk, cell);
// quantile_select_kernel<Kt>, one 1 024-thread workgroup per (group, cell), merges the at most 16 runs (sdsort::block_merge_rounds from
// round 6) and evaluates the quantiles.  The scratch is 8 * C * sum of np_g bytes: the source as float64, each group padded to whole
// chunks.
#pragma once
#include <vector>

#include "sd_groupby_plan.h"
#include "sd_wave_consts.h"

namespace sdqt {
constexpr int kSegWidths[] = {5, 13, 21};      // quantile_segment_kernel<S, K>
constexpr int kSeriesWidths[] = {13, 17, 19};  // quantile_runs_kernel<S, K> / quantile_select_kernel<K>
constexpr int kMaxRuns = 16;                   // runs of 64 * K samples a 1 024-thread workgroup merges
constexpr int kSelectThreads = 1024;
constexpr int64_t kSeriesLimit = (int64_t)kSelectThreads * 19;  // 19 456
constexpr int64_t kGridLimit = (int64_t)1 << 31;
constexpr int kSegment = 0, kSeries = 1;

// workgroup b of the tile-shaped kernels -> (cell tile, item): sdw::xcd_tile_of_block as a function both sides compile
constexpr int64_t tile_of_block(int64_t b, int64_t ntiles) { return (b & 7) * ((ntiles + 7) / 8) + (b >> 3) % ((ntiles + 7) / 8); }
constexpr int64_t item_of_block(int64_t b, int64_t ntiles) { return (b >> 3) / ((ntiles + 7) / 8); }
}  // namespace sdqt

struct QuantileCall {
    int method = SD_QUANTILE_LINEAR;
    bool skipna = true, src_is_f32 = false;
    int64_t T = 0, C = 0, ld = 0;  // the source: rows, cells, elements between two rows (>= C)
    int64_t G = 0;                 // groups
    int64_t Q = 0;                 // quantiles (not read with SD_QUANTILE_MEDIAN: one)
    const double* q = nullptr;     // host [Q] (not read with SD_QUANTILE_MEDIAN)
    int64_t ld_out = 0;            // elements between two rows of the output [Q * G, C] (>= C)
    bool src_aligned16 = true;
    size_t lds_max = 160 * 1024;
    int cu_count = 256;
};

// one chunk of the series path: rows[start .. start + len) of the row table -> slots [local, local + 64 * K) of the run of its group
struct QuantileChunk {
    int64_t base;  // first slot of the group's runs: cell c starts at base + c * np
    int32_t np, local, start, len;
};
// one group of the series path
struct QuantileGroup {
    int64_t base;
    int32_t np, n, chunk0, nchunks;
};

struct QuantilePlan {
    int error = SD_OK;
    char message[256] = "";
    int64_t Q = 0;          // quantiles evaluated (1 for the median)
    int64_t n_max = 0;      // rows of the longest group
    int path = sdqt::kSegment;
    int K = 0;              // width of the path's sort
    bool vec = false;       // 16-byte loads of the source (8-byte ones of a float32 source)
    // segment path, and the runs kernel of the series path
    int rs = 0;             // doubles between two LDS rows
    size_t lds = 0;         // dynamic LDS bytes of a workgroup
    int per_cu = 0;         // workgroups of a CU by LDS and by threads
    int64_t ntiles = 0;     // tiles of 8 cells
    int64_t blocks = 0;     // 8 * ceil(ntiles / 8) * (G | chunks)
    // series path
    int64_t chunks = 0;     // chunks of all groups
    int64_t run_slots = 0;  // sum of np_g: slots per cell of the runs scratch
    int np_max = 0;
    size_t select_lds = 0;
    int64_t select_blocks = 0;
};

namespace sdqt {
inline int seg_width(int64_t n_max) {
    for (int K : kSegWidths)
        if (n_max <= (int64_t)sdw::kWave * K) return K;
    return 0;
}
inline int series_width(int64_t n_max) {
    for (int K : kSeriesWidths)
        if (n_max <= (int64_t)kMaxRuns * sdw::kWave * K) return K;
    return 0;
}
inline int per_cu(size_t lds, size_t lds_max, int threads) {
    const int by_lds = (int)(lds_max / (lds > 0 ? lds : 1)), by_threads = 2048 / threads;
    return by_lds < by_threads ? by_lds : by_threads;
}
}  // namespace sdqt

inline QuantilePlan quantile_check(const QuantileCall& c) {
    using sdbn::fail;
    const char* const who = "sd_quantile";
    QuantilePlan pl;
    if (!(c.method >= SD_QUANTILE_LINEAR && c.method <= SD_QUANTILE_MEDIAN)) return fail(pl, SD_ERR_INVALID, "%s: unknown method code %d", who, c.method);
    if (!(c.T > 0 && c.C > 0)) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (T=%lld, C=%lld)", who, (long long)c.T, (long long)c.C);
    const bool median = c.method == SD_QUANTILE_MEDIAN;
    pl.Q = median ? 1 : c.Q;
    if (c.G <= 0 || pl.Q <= 0) return fail(pl, SD_ERR_INVALID, "%s: bad sizes (G=%lld, Q=%lld)", who, (long long)c.G, (long long)pl.Q);
    if (!median)
        for (int64_t i = 0; i < c.Q; ++i)
            if (!(c.q[i] >= 0.0 && c.q[i] <= 1.0))  // (NaN fails both comparisons)
                return fail(pl, SD_ERR_INVALID, "%s: Quantiles must be in the range [0, 1] (q[%lld] = %g)", who, (long long)i, c.q[i]);
    for (const sdgb::NamedLd& l : {sdgb::NamedLd{"ld", c.ld, true}, sdgb::NamedLd{"ld_out", c.ld_out, true}})
        if (l.ld < c.C) return fail(pl, SD_ERR_INVALID, "%s: %s = %lld is less than the %lld cells of a row", who, l.name, (long long)l.ld, (long long)c.C);
    const int64_t most = INT64_MAX / 8;
    if (c.T > most / c.ld || pl.Q > most / c.G || pl.Q * c.G > most / c.ld_out) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
    return pl;
}

inline QuantilePlan quantile_groups(QuantilePlan pl, const int32_t* group, int64_t T, int64_t G) {
    if (pl.error != SD_OK || group == nullptr) return pl;
    const GroupbyPlan g = groupby_check_groups(GroupbyPlan(), "sd_quantile", group, T, G);
    return g.error == SD_OK ? pl : sdbn::fail(pl, g.error, "%s", g.message);
}

// chunks of the groups of the series path, in group order
inline void quantile_series_tables(const int64_t* offsets, int64_t G, int K, std::vector<QuantileChunk>* chunks, std::vector<QuantileGroup>* groups,
                                   int64_t C) {
    const int chunk = sdw::kWave * K;
    int64_t slots = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = offsets[g + 1] - offsets[g], nch = (n + chunk - 1) / chunk;
        QuantileGroup gr;
        gr.base = slots * C, gr.np = (int32_t)(nch * chunk), gr.n = (int32_t)n, gr.chunk0 = (int32_t)chunks->size(), gr.nchunks = (int32_t)nch;
        groups->push_back(gr);
        for (int64_t j = 0; j < nch; ++j) {
            QuantileChunk ch;
            ch.base = gr.base, ch.np = gr.np, ch.local = (int32_t)(j * chunk), ch.start = (int32_t)(offsets[g] + j * chunk);
            ch.len = (int32_t)(n - j * chunk < chunk ? n - j * chunk : chunk);
            chunks->push_back(ch);
        }
        slots += nch * chunk;
    }
}

// 8 * ld < 2^32 and T < 2^31: the last refusal of quantile_plan (an entry point asks it first for a T whose tables it could not build)
inline QuantilePlan quantile_row_limits(QuantilePlan pl, const QuantileCall& c) {
    if (pl.error == SD_OK && (c.ld >= ((int64_t)1 << 29) || c.T >= sdqt::kGridLimit))
        return sdbn::fail(pl, SD_ERR_INVALID, "sd_quantile: rows of %lld elements or %lld rows exceed the 32-bit row addressing", (long long)c.ld,
                          (long long)c.T);
    return pl;
}

// offsets [G + 1]: the group table of a call that quantile_check and quantile_groups accepted
inline QuantilePlan quantile_plan(QuantilePlan pl, const QuantileCall& c, const int64_t* offsets) {
    using namespace sdqt;
    using sdbn::fail;
    const char* const who = "sd_quantile";
    if (pl.error != SD_OK) return pl;
    pl.n_max = 0;
    for (int64_t g = 0; g < c.G; ++g)
        if (offsets[g + 1] - offsets[g] > pl.n_max) pl.n_max = offsets[g + 1] - offsets[g];
    if (pl.n_max > kSeriesLimit)
        return fail(pl, SD_ERR_UNSUPPORTED, "%s: a group of %lld samples exceeds the workgroup merge (%lld)", who, (long long)pl.n_max,
                    (long long)kSeriesLimit);
    pl.vec = c.ld % 2 == 0 && c.src_aligned16;
    pl.ntiles = (c.C + sdw::kW - 1) / sdw::kW;
    const int64_t tx8 = 8 * ((pl.ntiles + 7) / 8);
    pl.K = seg_width(pl.n_max);
    int64_t items = c.G;
    if (pl.K != 0) {
        pl.path = kSegment;
    } else {
        pl.path = kSeries;
        pl.K = series_width(pl.n_max);
        const int chunk = sdw::kWave * pl.K;
        pl.chunks = 0, pl.run_slots = 0, pl.np_max = 0;
        for (int64_t g = 0; g < c.G; ++g) {
            const int64_t nch = (offsets[g + 1] - offsets[g] + chunk - 1) / chunk;
            pl.chunks += nch, pl.run_slots += nch * chunk;
            if (nch * chunk > pl.np_max) pl.np_max = (int)(nch * chunk);
        }
        items = pl.chunks;
        pl.select_lds = sdw::block_sort_lds_bytes(pl.np_max);
        if (pl.select_lds > c.lds_max) return fail(pl, SD_ERR_UNSUPPORTED, "%s: the merge of %d slots does not fit the LDS", who, pl.np_max);
        if (c.G > (kGridLimit - 1) / c.C) return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
        if (pl.run_slots > INT64_MAX / 8 / c.C) return fail(pl, SD_ERR_INVALID, "%s: field too large", who);
        const int64_t cap = (int64_t)c.cu_count * 4;
        pl.select_blocks = c.G * c.C < cap ? c.G * c.C : cap;
    }
    pl.rs = sdw::tile_sort_rs(pl.K);
    pl.lds = sdw::tile_sort_lds_bytes(pl.K);
    pl.per_cu = per_cu(pl.lds, c.lds_max, sdw::kThreads);
    if (items > (kGridLimit - 1) / tx8) return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = tx8 * items;
    return quantile_row_limits(pl, c);
}

// what the plan chose, in words (tests/quantile_plan_check.cpp prints it)
inline void quantile_describe(const QuantilePlan& pl, char* buf, size_t size) {
    if (pl.path == sdqt::kSegment)
        snprintf(buf, size, "segment path: n_max=%lld K=%d rs=%d lds=%zu per_cu=%d blocks=%lld vec=%d", (long long)pl.n_max, pl.K, pl.rs, pl.lds,
                 pl.per_cu, (long long)pl.blocks, (int)pl.vec);
    else
        snprintf(buf, size, "series path: n_max=%lld K=%d chunks=%lld run_slots=%lld lds=%zu per_cu=%d blocks=%lld select_lds=%zu select_blocks=%lld vec=%d",
                 (long long)pl.n_max, pl.K, (long long)pl.chunks, (long long)pl.run_slots, pl.lds, pl.per_cu, (long long)pl.blocks, pl.select_lds,
                 (long long)pl.select_blocks, (int)pl.vec);
}
