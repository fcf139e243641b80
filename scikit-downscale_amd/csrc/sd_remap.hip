// First-order conservative (area-overlap) remapping of a fine [T, ny, nx] field onto a coarse [Ny, Nx] rectilinear grid
// (GridArray.remap_like: step 1 of the BCSD of Wood et al. 2004, the observations aggregated to the GCM's grid).  The rule, the two
// separable axis tables and the launch plan are in sd_remap_plan.h.
//
// remap_kernel<S, V>: a workgroup of four waves owns one target row j, one column tile and one chunk of 64 time steps; each wave
// takes 16 consecutive steps of it, in batches of 4.  The lanes of a wave map to consecutive *source* columns of the tile's span, V
// columns each (one load of V * sizeof(S) bytes, 16 where the plan allows), so every source row of run j is one coalesced load per wave
// and step; the loads of the 4 steps of a batch are issued before their arithmetic.  A lane forms cn = sum_y wy * value and
// cd = sum_y wy * (value is not NaN) for its columns in registers, over the rows of the run in stored order (wy and the row are
// wave-uniform: scalar loads), and writes them to its wave's part of the LDS.  Then one lane per (step of the batch, target column of
// the tile) adds its run from LDS serially in stored order, multiplied by wx, applies the rule and stores one double.  A tile wider
// than 64 * V source columns is a single target column (the plan): its span is walked in strips, the lane of a step carrying num and den
// from strip to strip.  No atomics, nothing depends on the CU count, and the order of every sum is fixed, so the result does not depend
// on the launch geometry or on how the time axis is cut.
//
// LDS: 2 doubles per source column of a strip, step of the batch and wave: 16 / 32 / 64 KB for V = 1 / 2 / 4.  Algorithmic bytes:
// sizeof(S) * T * ny * nx read, 8 * T * Ny * Nx written; a source row that straddles two target rows is read by both workgroups (the
// second read is an L2 hit at best), as are the few columns that straddle two tiles.
#include <vector>

#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_remap_plan.h"
#include "sd_state.h"

struct sd_remap {
    sd_ctx* ctx = nullptr;
    int64_t ny = 0, nx = 0, Ny = 0, Nx = 0;
    RemapAxis ay, ax;          // host copies: the plan of a call makes its column tiles from the x table
    int32_t* idx = nullptr;    // device: y first [Ny], y count [Ny], y start [Ny], x first [Nx], x count [Nx], x start [Nx]
    double* wgt = nullptr;     // device: y full [Ny], x full [Nx], y weights [y_entries], x weights [x_entries]
};

namespace {
using namespace sdrm;

template <typename S, int V>
__global__ void __launch_bounds__(kLanes* kWaves) remap_kernel(const S* __restrict__ src, int64_t ld, int64_t T, int nx, int64_t Ny, int Nx,
                                                              int64_t ntiles, const RemapTile* __restrict__ tiles,
                                                              const int32_t* __restrict__ idx, const double* __restrict__ wgt,
                                                              int64_t y_entries, double min_valid, double* __restrict__ out, int64_t ld_out) {
    constexpr int W = kLanes * V;
    __shared__ double2 sums[kWaves][kBatch][W];  // (cn, cd) of the strip's columns
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t tile_id = blockIdx.x % ntiles, rest = blockIdx.x / ntiles;
    const int64_t j = rest % Ny, chunk = rest / Ny;
    const RemapTile tile = tiles[tile_id];
    // the row's run: wave-uniform
    const int fy = idx[j], ky = idx[Ny + j];
    const double* const wy = wgt + Ny + Nx + idx[2 * Ny + j];
    const double full_y = wgt[j];
    const int32_t* const xfirst = idx + 3 * Ny;
    const int32_t* const xcount = xfirst + Nx;
    const int32_t* const xstart = xcount + Nx;
    const double* const xfull = wgt + Ny;
    const double* const wxs = wgt + Ny + Nx + y_entries;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double slack = 1.0 - 1.0 / 1073741824.0;  // 1 - 2^-30
    const int64_t tend = min((chunk + 1) * kTimeChunk, T);
    // every wave runs the same number of batches and strips (the barriers); a wave past the end of the field does nothing in them
    for (int b = 0; b < kStepsPerWave; b += kBatch) {
        const int64_t tb = chunk * kTimeChunk + (int64_t)wave * kStepsPerWave + b;
        const bool active = tb < tend;
        double num = 0.0, den = 0.0;  // (of a one-column tile: carried from strip to strip)
        for (int64_t s = 0; s == 0 || s < tile.ns; s += W) {
            const int64_t x0 = s + lane * V;  // the lane's first column within the span
            if (active && x0 < tile.ns) {
                double cn[kBatch][V], cd[kBatch][V];
#pragma unroll
                for (int u = 0; u < kBatch; ++u)
#pragma unroll
                    for (int v = 0; v < V; ++v) cn[u][v] = 0.0, cd[u][v] = 0.0;
                const S* const col = src + tile.s0 + x0;
                for (int r = 0; r < ky; ++r) {
                    const double w = wy[r];
                    const int64_t row = (int64_t)(fy + r) * nx;
                    sdbn::Cells<S, V> q[kBatch];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u)  // (a step past the end reads the last one again and is not stored)
                        q[u] = *reinterpret_cast<const sdbn::Cells<S, V>*>(col + min(tb + u, tend - 1) * ld + row);
#pragma unroll
                    for (int u = 0; u < kBatch; ++u)
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const double x = (double)q[u].v[v];
                            const bool valid = x == x;
                            cn[u][v] += w * (valid ? x : 0.0);
                            cd[u][v] += w * (valid ? 1.0 : 0.0);
                        }
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u)
#pragma unroll
                    for (int v = 0; v < V; ++v) sums[wave][u][lane * V + v] = make_double2(cn[u][v], cd[u][v]);
            }
            __syncthreads();
            if (active) {
                const bool last_strip = s + W >= tile.ns;
                for (int p = lane; p < tile.nc * kBatch; p += kLanes) {
                    const int u = p / tile.nc, i = tile.c0 + p % tile.nc;
                    if (s == 0) num = 0.0, den = 0.0;
                    const int fx = xfirst[i], kx = xcount[i];
                    const double* const wx = wxs + xstart[i];
                    // the columns of the run that lie in this strip, in stored order
                    const int64_t lo = max((int64_t)fx, tile.s0 + s), hi = min((int64_t)fx + kx, tile.s0 + s + W);
                    for (int64_t x = lo; x < hi; ++x) {
                        const double2 c = sums[wave][u][x - tile.s0 - s];
                        const double w = wx[x - fx];
                        num += w * c.x;
                        den += w * c.y;
                    }
                    if (last_strip && tb + u < tend) {
                        const double need = min_valid * (full_y * xfull[i]) * slack;
                        out[(tb + u) * ld_out + j * Nx + i] = (den > 0.0 && den >= need) ? num / den : nan;
                    }
                }
            }
            __syncthreads();
        }
    }
}

RemapCall call_of(const sd_remap* rm, int64_t T, int64_t ld, int64_t ld_out, double min_valid, int src_is_f32, const void* src) {
    RemapCall c;
    c.T = T, c.ny = rm->ny, c.nx = rm->nx, c.Ny = rm->Ny, c.Nx = rm->Nx, c.ld = ld, c.ld_out = ld_out, c.min_valid = min_valid;
    c.src_is_f32 = src_is_f32 != 0;
    c.src_aligned16 = ((uintptr_t)src & 15) == 0;
    return c;
}

std::vector<sd_buf> remap_bufs(const sd_remap* rm) {
    return {sd_buf_of(rm->idx, 3 * (size_t)(rm->Ny + rm->Nx)), sd_buf_of(rm->wgt, (size_t)(rm->Ny + rm->Nx) + rm->ay.w.size() + rm->ax.w.size())};
}

}  // namespace

extern "C" {

int sd_remap_destroy(sd_remap* rm) { return sd_state_destroy(rm, remap_bufs); }

int sd_remap_info(const sd_remap* rm, int64_t* ny, int64_t* nx, int64_t* Ny, int64_t* Nx, int64_t* y_entries, int64_t* x_entries) {
    SD_CHECK_ARG(rm, "state is NULL");
    if (ny) *ny = rm->ny;
    if (nx) *nx = rm->nx;
    if (Ny) *Ny = rm->Ny;
    if (Nx) *Nx = rm->Nx;
    if (y_entries) *y_entries = (int64_t)rm->ay.w.size();
    if (x_entries) *x_entries = (int64_t)rm->ax.w.size();
    return SD_OK;
}

int sd_remap_create(sd_ctx* ctx, int64_t ny, int64_t nx, const double* src_yb, const double* src_xb, int64_t Ny, int64_t Nx,
                    const double* dst_yb, const double* dst_xb, sd_remap** out) {
    SD_CHECK_ARG(ctx && src_yb && src_xb && dst_yb && dst_xb && out, "sd_remap_create: NULL argument");
    *out = nullptr;
    sd_remap* rm = new sd_remap();
    rm->ctx = ctx, rm->ny = ny, rm->nx = nx, rm->Ny = Ny, rm->Nx = Nx;
    return sd_state_build(rm, sd_remap_destroy, out, [&]() -> int {
        rm->ay = remap_axis("y", src_yb, ny, dst_yb, Ny);
        if (rm->ay.error != SD_OK) return sd_set_error(rm->ay.error, "%s", rm->ay.message);
        rm->ax = remap_axis("x", src_xb, nx, dst_xb, Nx);
        if (rm->ax.error != SD_OK) return sd_set_error(rm->ax.error, "%s", rm->ax.message);
        RemapCall c;  // the refusals by size, on a call of one time step
        c.T = 1, c.ny = ny, c.nx = nx, c.Ny = Ny, c.Nx = Nx;
        c.ld = ny <= INT64_MAX / nx ? ny * nx : 0, c.ld_out = Ny <= INT64_MAX / Nx ? Ny * Nx : 0;
        const RemapPlan pl = remap_plan(c, rm->ay, rm->ax);
        if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
        std::vector<int32_t> idx;
        std::vector<double> wgt;
        for (const RemapAxis* a : {&rm->ay, &rm->ax})
            for (const std::vector<int32_t>* v : {&a->first, &a->count, &a->start}) idx.insert(idx.end(), v->begin(), v->begin() + a->n_dst);
        for (const std::vector<double>* v : {&rm->ay.full, &rm->ax.full, &rm->ay.w, &rm->ax.w}) wgt.insert(wgt.end(), v->begin(), v->end());
        SD_HIP(hipSetDevice(ctx->device));
        SD_TRY(sd_state_alloc(ctx, remap_bufs(rm)));
        SD_TRY(sd_state_copy(ctx, remap_bufs(rm), {idx.data(), wgt.data()}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the host tables go away on return)
        return SD_OK;
    });
}

int sd_remap_apply_dev(sd_ctx* ctx, const sd_remap* rm, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, double min_valid,
                       double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && rm && src_dev && out_dev, "sd_remap_apply: NULL argument");
    SD_CHECK_ARG(rm->ctx == ctx, "sd_remap_apply: the state belongs to another context");
    const RemapPlan pl = remap_plan(call_of(rm, T, ld, ld_out, min_valid, src_is_f32, src_dev), rm->ay, rm->ax);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch tiles;
    SD_TRY(upload(ctx, tiles, pl.tiles));
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    const int64_t y_entries = (int64_t)rm->ay.w.size();
    SD_TRY(sdbn::with_cells(src_is_f32 != 0, pl.cols, src_dev, [&](auto* src, auto cols) -> int {
        using S = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        SD_LAUNCH(ctx, "remap_kernel", (remap_kernel<S, decltype(cols)::value>), grid, block, 0, src, ld, T, (int)rm->nx, rm->Ny, (int)rm->Nx,
                  pl.ntiles, (const RemapTile*)tiles.p, (const int32_t*)rm->idx, (const double*)rm->wgt, y_entries, min_valid, out_dev, ld_out);
        return SD_OK;
    }));
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the tile table goes away on return)
    return SD_OK;
}

int sd_remap_apply(sd_ctx* ctx, const sd_remap* rm, const void* src_host, int src_is_f32, int64_t T, double min_valid, double* out_host) {
    SD_CHECK_ARG(ctx && rm && src_host && out_host, "sd_remap_apply: NULL argument");
    const int64_t plane = rm->ny * rm->nx, C = rm->Ny * rm->Nx;
    const RemapPlan pl = remap_plan(call_of(rm, T, plane, C, min_valid, src_is_f32, nullptr), rm->ay, rm->ax);  // (before the upload)
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * plane;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_out(out_host, sizeof(double) * (size_t)T * C)};
    return with_device_copies(ctx, f, [&](void* const* d) { return sd_remap_apply_dev(ctx, rm, d[0], src_is_f32, plane, T, min_valid, (double*)d[1], C); });
}

}  // extern "C"
