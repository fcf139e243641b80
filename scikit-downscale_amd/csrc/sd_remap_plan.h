// Launch plan and axis tables of a conservative remapping call (GridArray.remap_like: a fine [T, ny, nx] field onto a coarse
// [Ny, Nx] rectilinear grid by area overlap, first order), as pure host functions (no HIP header: tests/remap_plan_check.cpp compiles
// this file with g++ alone).
//
// remap_axis:  the separable table of one dimension from the cell bounds of the source (n + 1) and of the target (n_dst + 1), each
//              strictly ascending or descending as stored.  The overlap of source cell k with target cell j is
//              w = min(sb_hi, db_hi) - max(sb_lo, db_lo) on the ascending-ordered bounds, one IEEE subtraction; only overlaps > 0
//              enter.  The source cells of target j are one contiguous run in stored order: first[j], count[j], the weights at
//              start[j] .. start[j] + count[j] - 1 in stored order, and full[j], their running sum from +0.0.  At most
//              n + n_dst - 1 entries; never a per-cell table.  A target cell outside the source hull has an empty run (first = 0).
// remap_plan:  the geometry of remap_kernel (sd_remap.hip) -- source columns per lane, column tiles, time chunks, LDS bytes, grid --
//              and every refusal that depends only on sizes.  A column tile is a run of consecutive target columns whose combined
//              source span fits kLanes * cols source columns; the tiles are made greedily from the x table, and a single target
//              column whose run alone is wider gets a tile of its own, whose span the kernel walks in strips.  The launcher takes all
//              of it from here.  Nothing depends on the CU count.
//
// The value (sd_remap.hip restates it): cn[x] = sum_y wy * (v is NaN ? 0 : v), cd[x] = sum_y wy * (v is NaN ? 0 : 1) over the rows of
// the run in stored order, num = sum_x wx * cn[x], den = sum_x wx * cd[x] over the columns of the run in stored order, every product
// rounded on its own; out = num / den where den > 0 and den >= min_valid * (full_y * full_x) * (1 - 2^-30), else NaN.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "sd_bins_plan.h"

namespace sdrm {
constexpr int kLanes = 64;
constexpr int kWaves = 4;           // waves of a workgroup: same target row and column tile, consecutive runs of time steps
constexpr int kStepsPerWave = 16;   // time steps of one wave
constexpr int kBatch = 4;           // time steps whose loads are in flight before their arithmetic, and whose sums share an LDS pass
constexpr int kTimeChunk = kWaves * kStepsPerWave;  // time steps of a workgroup
constexpr int kMaxCols = 4;         // source columns of a lane: at most one 16-byte load of float32
constexpr int64_t kGridLimit = (int64_t)1 << 31;
static_assert(kStepsPerWave % kBatch == 0, "whole batches");
// LDS of a workgroup: (cn, cd) per source column of the tile, step of the batch and wave
constexpr int64_t lds_bytes(int cols) { return (int64_t)kWaves * kBatch * kLanes * cols * 2 * (int64_t)sizeof(double); }
static_assert(lds_bytes(kMaxCols) <= 64 * 1024, "at least two workgroups share the 160 KB of a CU");
}  // namespace sdrm

// ---- the table of one dimension ---------------------------------------------------------------------------------------------
struct RemapAxis {
    int error = SD_OK;
    char message[256] = "";
    int64_t n_src = 0, n_dst = 0;
    std::vector<int32_t> first, count;  // [n_dst] the run of target j: source cells first[j] .. first[j] + count[j] - 1 as stored
    std::vector<int32_t> start;         // [n_dst + 1] where the weights of run j begin in w
    std::vector<double> w;              // the overlaps, run by run, each run in stored order
    std::vector<double> full;           // [n_dst] running sum from +0.0 of the run's weights
};

inline RemapAxis remap_axis(const char* name, const double* sb, int64_t n, const double* db, int64_t n_dst) {
    RemapAxis ax;
    const auto fail = [&](const char* what) {
        snprintf(ax.message, sizeof ax.message, "sd_remap: %s '%s'", what, name);
        ax.error = SD_ERR_INVALID;
        return ax;
    };
    if (n < 1) return fail("no source cell along");
    if (n_dst < 1) return fail("no target cell along");
    if (n > std::numeric_limits<int32_t>::max() - n_dst) return fail("too many cells along");
    for (int64_t i = 0; i <= n; ++i)
        if (std::isnan(sb[i])) return fail("NaN in the source bounds of");
    for (int64_t i = 0; i <= n_dst; ++i)
        if (std::isnan(db[i])) return fail("NaN in the target bounds of");
    const auto monotonic = [](const double* b, int64_t cells) {
        const bool up = b[cells] > b[0];
        for (int64_t i = 0; i < cells; ++i)
            if (!(up ? b[i + 1] > b[i] : b[i + 1] < b[i])) return false;
        return true;
    };
    if (!monotonic(sb, n)) return fail("non-monotonic or duplicated source bounds of");
    if (!monotonic(db, n_dst)) return fail("non-monotonic or duplicated target bounds of");
    const bool asc = sb[n] > sb[0];
    std::vector<double> a(sb, sb + n + 1);  // ascending: cell i of it is [a[i], a[i + 1]], stored as cell asc ? i : n - 1 - i
    if (!asc) std::reverse(a.begin(), a.end());
    ax.n_src = n, ax.n_dst = n_dst;
    ax.first.assign((size_t)n_dst, 0), ax.count.assign((size_t)n_dst, 0), ax.full.assign((size_t)n_dst, 0.0);
    ax.start.assign((size_t)n_dst + 1, 0);
    for (int64_t j = 0; j < n_dst; ++j) {
        const double lo = std::min(db[j], db[j + 1]), hi = std::max(db[j], db[j + 1]);
        // cells whose upper bound lies above lo and whose lower bound lies below hi: their overlap is the difference of two
        // different numbers, the larger first, which never rounds to zero
        const int64_t i0 = std::upper_bound(a.begin() + 1, a.end(), lo) - (a.begin() + 1);
        const int64_t i1 = std::lower_bound(a.begin(), a.begin() + n, hi) - a.begin();
        ax.start[(size_t)j] = (int32_t)ax.w.size();
        if (i1 <= i0) continue;
        ax.first[(size_t)j] = (int32_t)(asc ? i0 : n - i1);
        double full = 0.0;
        for (int64_t k = ax.first[(size_t)j]; k < ax.first[(size_t)j] + (i1 - i0); ++k) {
            const int64_t i = asc ? k : n - 1 - k;
            const double w = std::min(a[(size_t)i + 1], hi) - std::max(a[(size_t)i], lo);
            if (!(w > 0)) continue;  // (not reached for finite bounds, see above)
            ax.w.push_back(w);
            full += w;
        }
        ax.count[(size_t)j] = (int32_t)((int64_t)ax.w.size() - ax.start[(size_t)j]);
        ax.full[(size_t)j] = full;
    }
    ax.start[(size_t)n_dst] = (int32_t)ax.w.size();
    return ax;
}

// ---- the launch plan ----------------------------------------------------------------------------------------------------------
struct RemapCall {
    int64_t T = 0, ny = 0, nx = 0, Ny = 0, Nx = 0;
    int64_t ld = 0;             // elements between two time steps of the source (>= ny * nx)
    int64_t ld_out = 0;         // elements between two time steps of the output (>= Ny * Nx)
    double min_valid = 0.5;
    bool src_is_f32 = false;
    bool src_aligned16 = true;  // the source pointer is a multiple of 16 bytes
};

struct RemapTile {
    int32_t c0, nc;  // target columns c0 .. c0 + nc - 1
    int32_t s0, ns;  // their combined source span: columns s0 .. s0 + ns - 1 (s0 and ns multiples of cols; ns = 0: no source column)
};

struct RemapPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int cols = 0;          // adjacent source columns of a lane: one load of cols source elements per row
    int block = 0;         // threads of a workgroup
    int tile_width = 0;    // source columns of a strip: kLanes * cols
    int64_t lds_bytes = 0;
    std::vector<RemapTile> tiles;
    int64_t ntiles = 0;
    int64_t nchunks = 0;   // time chunks of kTimeChunk steps
    int64_t blocks = 0;    // ntiles * Ny * nchunks, column tile fastest, then the target row, then the time chunk
};

inline RemapPlan remap_plan(const RemapCall& c, const RemapAxis& ay, const RemapAxis& ax) {
    using namespace sdrm;
    RemapPlan pl;
    const auto fail = [&](int code, const char* fmt, auto... a) {
        snprintf(pl.message, sizeof pl.message, fmt, a...);
        pl.error = code;
        pl.tiles.clear();
        return pl;
    };
    if (!(c.T > 0 && c.ny > 0 && c.nx > 0 && c.Ny > 0 && c.Nx > 0))
        return fail(SD_ERR_INVALID, "sd_remap: bad sizes (T=%lld, source %lld x %lld, target %lld x %lld)", (long long)c.T, (long long)c.ny,
                    (long long)c.nx, (long long)c.Ny, (long long)c.Nx);
    const int64_t last = kGridLimit - 1, most = std::numeric_limits<int64_t>::max();
    // (the kernel indexes rows, columns and table entries with int, a plane and the field with int64_t)
    if (c.ny > last - c.Ny || c.nx > last - c.Nx || c.ny > most / c.nx || c.Ny > most / c.Nx)
        return fail(SD_ERR_INVALID, "%s", "sd_remap: grid too large");
    if (c.ld < c.ny * c.nx)
        return fail(SD_ERR_INVALID, "sd_remap: ld = %lld is less than the %lld cells of the source grid", (long long)c.ld,
                    (long long)(c.ny * c.nx));
    if (c.ld_out < c.Ny * c.Nx)
        return fail(SD_ERR_INVALID, "sd_remap: ld_out = %lld is less than the %lld cells of the target grid", (long long)c.ld_out,
                    (long long)(c.Ny * c.Nx));
    if (!(c.min_valid >= 0.0 && c.min_valid <= 1.0))
        return fail(SD_ERR_INVALID, "sd_remap: min_valid = %g lies outside [0, 1]", c.min_valid);
    if (c.T > most / c.ld || c.T > most / c.ld_out) return fail(SD_ERR_INVALID, "%s", "sd_remap: grid too large");
    if (ay.n_src != c.ny || ay.n_dst != c.Ny || ax.n_src != c.nx || ax.n_dst != c.Nx)
        return fail(SD_ERR_INVALID, "%s", "sd_remap: the axis tables are not those of this grid");
    // cols adjacent source columns of a lane need every group of a row aligned to its load, and pay only where a row is wider than
    // one wave: four for float32 (16 bytes), two (16 bytes of float64, 8 of float32), one
    const auto fits = [&](int v) { return c.nx % v == 0 && c.ld % v == 0 && c.src_aligned16 && c.nx > kLanes; };
    pl.cols = (c.src_is_f32 && fits(4)) ? 4 : fits(2) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.tile_width = kLanes * pl.cols;
    pl.lds_bytes = lds_bytes(pl.cols);
    // the column tiles, greedily
    const int64_t V = pl.cols, W = pl.tile_width;
    RemapTile cur{0, 0, 0, 0};
    for (int64_t i = 0; i < c.Nx; ++i) {
        const bool has = ax.count[(size_t)i] > 0;
        const int64_t lo = has ? ax.first[(size_t)i] / V * V : 0;
        const int64_t hi = has ? (ax.first[(size_t)i] + ax.count[(size_t)i] + V - 1) / V * V : 0;  // (nx is a multiple of V: inside the row)
        if (cur.nc > 0) {
            const int64_t l = !has ? cur.s0 : cur.ns == 0 ? lo : std::min<int64_t>(cur.s0, lo);
            const int64_t h = !has ? cur.s0 + cur.ns : cur.ns == 0 ? hi : std::max<int64_t>(cur.s0 + cur.ns, hi);
            if (cur.nc < W && h - l <= W) {
                cur.nc += 1, cur.s0 = (int32_t)l, cur.ns = (int32_t)(h - l);
                continue;
            }
            pl.tiles.push_back(cur);
        }
        cur = RemapTile{(int32_t)i, 1, (int32_t)lo, (int32_t)(hi - lo)};
    }
    pl.tiles.push_back(cur);
    pl.ntiles = (int64_t)pl.tiles.size();
    pl.nchunks = (c.T - 1) / kTimeChunk + 1;
    if (c.Ny > last / pl.ntiles || pl.nchunks > last / (pl.ntiles * c.Ny))  // blocks < 2^31
        return fail(SD_ERR_INVALID, "%s", "sd_remap: grid too large");
    pl.blocks = pl.ntiles * c.Ny * pl.nchunks;
    return pl;
}
