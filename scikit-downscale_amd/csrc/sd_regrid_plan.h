// Launch plan and axis tables of a regridding call (GridArray.interp_like: a [T, ny, nx] field onto an [Ny, Nx] rectilinear grid),
// as pure host functions (no HIP header: tests/regrid_plan_check.cpp compiles this file with g++ alone).
//
// regrid_plan:  the geometry of regrid_kernel (sd_regrid.hip) from the sizes of the call -- grid, block, time chunk, columns per
//               lane -- and every refusal that depends only on sizes and codes.  The launcher takes all of it from here.  The kernel
//               keeps nothing in LDS and its grid does not depend on the CU count, so neither is an input.
// regrid_axis:  the separable table of one dimension, n_dst entries (never a per-cell table): per target coordinate the two source
//               nodes of its bracket, the distance to the lower one and the reciprocal of the bracket's width.  It restates
//               scipy.interpolate.interp1d(kind='linear' | 'nearest', bounds_error=False, fill_value=nan, assume_sorted=False), which
//               is what xarray's interp_like evaluates per dimension for 1-D coordinates:
//                 linear   hi = clip(searchsorted(x ascending, xn, side='left'), 1, n - 1), lo = hi - 1
//                 nearest  index = clip(searchsorted((x[1:] / 2 + x[:-1] / 2), xn, side='left'), 0, n - 1): a midpoint goes to the
//                          lower neighbour
//                 both     NaN outside [x[0], x[n - 1]]: the table carries it as a NaN distance, which the arithmetic passes on
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "sd_bins_plan.h"

namespace sdrg {
constexpr int kLanes = 64;
constexpr int kWaves = 4;            // waves of a workgroup: same target row and columns, consecutive runs of time steps
constexpr int kStepsPerWave = 16;    // time steps of one wave
constexpr int kBatch = 4;            // time steps whose loads are in flight before their arithmetic
constexpr int kTimeChunk = kWaves * kStepsPerWave;  // time steps of a workgroup
constexpr int64_t kGridLimit = (int64_t)1 << 31;
static_assert(kStepsPerWave % kBatch == 0, "whole batches");
}  // namespace sdrg

struct RegridCall {
    int method = SD_REGRID_LINEAR;
    int64_t T = 0, ny = 0, nx = 0, Ny = 0, Nx = 0;
    int64_t ld_out = 0;        // elements between two time steps of the output (>= Ny * Nx)
    bool out_aligned16 = true;  // the output pointer is a multiple of 16 bytes
};

struct RegridPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int cols = 0;       // adjacent target columns of a lane: 2 (one 16-byte store per lane and step) or 1 (8-byte stores)
    int block = 0;      // threads of a workgroup
    int64_t xtiles = 0;   // column tiles of kLanes * cols columns per target row
    int64_t nchunks = 0;  // time chunks of kTimeChunk steps
    int64_t blocks = 0;   // xtiles * Ny * nchunks, column tile fastest, then the target row, then the time chunk
};

inline RegridPlan regrid_plan(const RegridCall& c) {
    using namespace sdrg;
    using sdbn::fail;
    RegridPlan pl;
    if (!(c.method == SD_REGRID_LINEAR || c.method == SD_REGRID_NEAREST))
        return fail(pl, SD_ERR_INVALID, "sd_regrid: unknown method code %d", c.method);
    if (!(c.T > 0 && c.ny > 0 && c.nx > 0 && c.Ny > 0 && c.Nx > 0))
        return fail(pl, SD_ERR_INVALID, "sd_regrid: bad sizes (T=%lld, source %lld x %lld, target %lld x %lld)", (long long)c.T,
                    (long long)c.ny, (long long)c.nx, (long long)c.Ny, (long long)c.Nx);
    if (c.ny < 2 || c.nx < 2)
        return fail(pl, SD_ERR_INVALID, "sd_regrid: a source dimension of length 1 cannot be interpolated (source %lld x %lld)",
                    (long long)c.ny, (long long)c.nx);
    const int64_t last = kGridLimit - 1;  // the largest count an int holds
    // (the kernel indexes a source plane and a target row with int; the cells of the target grid with int64_t)
    if (c.ny > last / c.nx || c.Nx > last || c.Ny > std::numeric_limits<int64_t>::max() / c.Nx)
        return fail(pl, SD_ERR_INVALID, "%s", "sd_regrid: grid too large");
    if (c.ld_out < c.Ny * c.Nx)
        return fail(pl, SD_ERR_INVALID, "sd_regrid: ld_out = %lld is less than the %lld cells of the target grid", (long long)c.ld_out,
                    (long long)(c.Ny * c.Nx));
    // two columns per lane need every pair of a row 16-byte aligned, and pay only where a row is wider than one wave
    pl.cols = (c.Nx % 2 == 0 && c.ld_out % 2 == 0 && c.out_aligned16 && c.Nx > kLanes) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.xtiles = (c.Nx + kLanes * pl.cols - 1) / (kLanes * pl.cols);
    pl.nchunks = (c.T - 1) / kTimeChunk + 1;
    if (c.Ny > last / pl.xtiles || pl.nchunks > last / (pl.xtiles * c.Ny))  // blocks < 2^31
        return fail(pl, SD_ERR_INVALID, "%s", "sd_regrid: grid too large");
    pl.blocks = pl.xtiles * c.Ny * pl.nchunks;
    return pl;
}

// ---- the table of one dimension ---------------------------------------------------------------------------------------------
struct RegridAxis {
    int error = SD_OK;
    char message[256] = "";
    std::vector<int32_t> lo, hi;  // [n_dst] positions of the bracket's nodes in the source as it is stored (nearest: lo = hi = the node)
    std::vector<double> t, r;     // [n_dst] xn - x[lo] (NaN outside the source range; nearest: 0 or NaN) and 1 / (x[hi] - x[lo])
};

inline RegridAxis regrid_axis(int method, const char* name, const double* src, int64_t n, const double* dst, int64_t n_dst) {
    RegridAxis ax;
    const auto fail = [&](const char* what) {
        snprintf(ax.message, sizeof ax.message, "sd_regrid: %s coordinate '%s'", what, name);
        ax.error = SD_ERR_INVALID;
        return ax;
    };
    for (int64_t i = 0; i < n; ++i)
        if (std::isnan(src[i])) return fail("NaN in the source");
    for (int64_t i = 0; i < n_dst; ++i)
        if (std::isnan(dst[i])) return fail("NaN in the target");
    const bool asc = src[n - 1] > src[0];
    std::vector<double> x(src, src + n);  // ascending, as interp1d(assume_sorted=False) sorts it
    if (!asc) std::reverse(x.begin(), x.end());
    for (int64_t i = 1; i < n; ++i)
        if (!(x[i] > x[i - 1])) return fail("non-monotonic or duplicated source");
    const auto stored = [&](int64_t i) { return (int32_t)(asc ? i : n - 1 - i); };
    std::vector<double> mid;
    if (method == SD_REGRID_NEAREST)
        for (int64_t i = 0; i + 1 < n; ++i) mid.push_back(x[i + 1] / 2.0 + x[i] / 2.0);
    ax.lo.resize((size_t)n_dst), ax.hi.resize((size_t)n_dst), ax.t.resize((size_t)n_dst), ax.r.resize((size_t)n_dst);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t k = 0; k < n_dst; ++k) {
        const double xn = dst[k];
        const bool outside = xn < x[0] || xn > x[n - 1];
        if (method == SD_REGRID_NEAREST) {
            const int64_t i = std::min<int64_t>(std::lower_bound(mid.begin(), mid.end(), xn) - mid.begin(), n - 1);
            ax.lo[k] = ax.hi[k] = stored(i);
            ax.t[k] = outside ? nan : 0.0;
            ax.r[k] = 0.0;
        } else {
            const int64_t hi = std::clamp<int64_t>(std::lower_bound(x.begin(), x.end(), xn) - x.begin(), 1, n - 1), lo = hi - 1;
            ax.lo[k] = stored(lo), ax.hi[k] = stored(hi);
            ax.t[k] = outside ? nan : xn - x[lo];
            ax.r[k] = 1.0 / (x[hi] - x[lo]);
        }
    }
    return ax;
}
