// Regridding of a coarse [T, ny, nx] field onto an [Ny, Nx] rectilinear grid (GridArray.interp_like; xarray's interp_like with 1-D
// coordinates = scipy's interp1d per dimension, the first spatial dimension before the second).  The rule, the two separable axis
// tables and the launch plan are in sd_regrid_plan.h.
//
// regrid_kernel<S, V, NEAREST>: a workgroup of four waves owns one target row, one tile of 64 * V target columns and one chunk of
// 64 time steps; each wave takes 16 consecutive steps of it.  A lane owns V adjacent target columns: their brackets and weights stay
// in registers for the kernel's lifetime, the row's bracket and weights are the same in every lane (scalar registers).  Per batch of
// four time steps the 4 * V source reads of every step are issued before any arithmetic; the source plane of a step is a few KB to
// ~100 KB and every read is shared with the neighbouring lanes, rows and tiles, so the reads are served by L1 / L2 and what reaches
// HBM is the store: one full row segment per wave and step, 16 bytes per lane with V = 2 (1 KB per store instruction), 8 with V = 1.
// Algorithmic bytes: 8 * T * C written + the source read once.
//
// Arithmetic: slope = (v[hi] - v[lo]) * (1 / (x[hi] - x[lo])), value = slope * (xn - x[lo]) + v[lo], rows first, then columns, without
// contraction (-ffp-contract=off).  The reciprocal of the bracket width comes from the table (one rounding more than scipy's
// division: a few ulp of the bracket's magnitude); a division per pass would make the kernel compute bound (three float64 divisions per
// 8-byte store).  A NaN node gives a NaN slope and a target outside the source range a NaN distance: no branch.
#include <vector>

#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_regrid_plan.h"
#include "sd_state.h"

struct sd_regrid {
    sd_ctx* ctx = nullptr;
    int method = SD_REGRID_LINEAR;
    int64_t ny = 0, nx = 0, Ny = 0, Nx = 0;
    int32_t* idx = nullptr;  // device: y lo [Ny], y hi [Ny], x lo [Nx], x hi [Nx]
    double* wgt = nullptr;   // device: y t [Ny], y r [Ny], x t [Nx], x r [Nx]
};

namespace {
using namespace sdrg;

template <typename S, int V, bool NEAREST>
__global__ void __launch_bounds__(kLanes* kWaves) regrid_kernel(const S* __restrict__ src, int64_t T, int nx, int64_t plane, int64_t Ny,
                                                               int Nx, int64_t xtiles, const int32_t* __restrict__ idx,
                                                               const double* __restrict__ wgt, double* __restrict__ out, int64_t ld_out) {
    const int lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
    const int64_t xtile = blockIdx.x % xtiles, rest = blockIdx.x / xtiles;
    const int64_t iy = rest % Ny, chunk = rest / Ny;
    const int64_t t0 = chunk * kTimeChunk + (int64_t)wave * kStepsPerWave;
    const int64_t ix0 = (xtile * kLanes + lane) * V;  // (V == 2: Nx is even, both columns are inside or outside)
    if (t0 >= T || ix0 >= Nx) return;
    const int64_t t1 = min(t0 + kStepsPerWave, T);
    // the row: wave-uniform
    const int r0 = idx[iy] * nx, r1 = idx[Ny + iy] * nx;
    const double ty = wgt[iy], ry = wgt[Ny + iy];
    // the lane's columns
    int c0[V], c1[V];
    double tx[V], rx[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        c0[v] = idx[2 * Ny + ix0 + v];
        c1[v] = idx[2 * Ny + Nx + ix0 + v];
        tx[v] = wgt[2 * Ny + ix0 + v];
        rx[v] = wgt[2 * Ny + Nx + ix0 + v];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* const orow = out + iy * Nx + ix0;
    for (int64_t tb = t0; tb < t1; tb += kBatch) {
        double res[kBatch][V];
        if constexpr (NEAREST) {
            S q[kBatch][V];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const S* p = src + min(tb + u, t1 - 1) * plane;  // (a step past the end reads the last one again and is not stored)
#pragma unroll
                for (int v = 0; v < V; ++v) q[u][v] = p[r0 + c0[v]];
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) res[u][v] = (ty != ty || tx[v] != tx[v]) ? nan : (double)q[u][v];
        } else {
            S q[kBatch][V][4];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const S* p = src + min(tb + u, t1 - 1) * plane;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    q[u][v][0] = p[r0 + c0[v]];
                    q[u][v][1] = p[r1 + c0[v]];
                    q[u][v][2] = p[r0 + c1[v]];
                    q[u][v][3] = p[r1 + c1[v]];
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double v00 = (double)q[u][v][0], v10 = (double)q[u][v][1], v01 = (double)q[u][v][2], v11 = (double)q[u][v][3];
                    const double a0 = (v10 - v00) * ry * ty + v00;  // the first spatial dimension, at the two source columns
                    const double a1 = (v11 - v01) * ry * ty + v01;
                    res[u][v] = (a1 - a0) * rx[v] * tx[v] + a0;     // then the second
                }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
            if (tb + u < t1) sdbn::store_doubles<V>(orow + (tb + u) * ld_out, res[u]);
    }
}

template <typename S, int V>
int launch_method(sd_ctx* ctx, const sd_regrid* rg, const RegridPlan& pl, const S* src, int64_t T, double* out, int64_t ld_out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    const int64_t plane = rg->ny * rg->nx;
    if (rg->method == SD_REGRID_NEAREST)
        SD_LAUNCH(ctx, "regrid_kernel", (regrid_kernel<S, V, true>), grid, block, 0, src, T, (int)rg->nx, plane, rg->Ny, (int)rg->Nx, pl.xtiles,
                  (const int32_t*)rg->idx, (const double*)rg->wgt, out, ld_out);
    else
        SD_LAUNCH(ctx, "regrid_kernel", (regrid_kernel<S, V, false>), grid, block, 0, src, T, (int)rg->nx, plane, rg->Ny, (int)rg->Nx, pl.xtiles,
                  (const int32_t*)rg->idx, (const double*)rg->wgt, out, ld_out);
    return SD_OK;
}

template <typename S>
int launch(sd_ctx* ctx, const sd_regrid* rg, const RegridPlan& pl, const void* src, int64_t T, double* out, int64_t ld_out) {
    return pl.cols == 2 ? launch_method<S, 2>(ctx, rg, pl, (const S*)src, T, out, ld_out)
                        : launch_method<S, 1>(ctx, rg, pl, (const S*)src, T, out, ld_out);
}

RegridCall call_of(const sd_regrid* rg, int64_t T, int64_t ld_out, const void* out) {
    RegridCall c;
    c.method = rg->method;
    c.T = T, c.ny = rg->ny, c.nx = rg->nx, c.Ny = rg->Ny, c.Nx = rg->Nx, c.ld_out = ld_out;
    c.out_aligned16 = ((uintptr_t)out & 15) == 0;
    return c;
}

std::vector<sd_buf> regrid_bufs(const sd_regrid* rg) {
    const size_t n = 2 * (size_t)(rg->Ny + rg->Nx);
    return {sd_buf_of(rg->idx, n), sd_buf_of(rg->wgt, n)};
}

}  // namespace

extern "C" {

int sd_regrid_destroy(sd_regrid* rg) { return sd_state_destroy(rg, regrid_bufs); }

int sd_regrid_info(const sd_regrid* rg, int* method, int64_t* ny, int64_t* nx, int64_t* Ny, int64_t* Nx) {
    SD_CHECK_ARG(rg, "state is NULL");
    if (method) *method = rg->method;
    if (ny) *ny = rg->ny;
    if (nx) *nx = rg->nx;
    if (Ny) *Ny = rg->Ny;
    if (Nx) *Nx = rg->Nx;
    return SD_OK;
}

int sd_regrid_create(sd_ctx* ctx, int method, int64_t ny, int64_t nx, const double* src_y, const double* src_x, int64_t Ny, int64_t Nx,
                     const double* dst_y, const double* dst_x, sd_regrid** out) {
    SD_CHECK_ARG(ctx && src_y && src_x && dst_y && dst_x && out, "sd_regrid_create: NULL argument");
    *out = nullptr;
    RegridCall c;  // the refusals by size and method, on a call of one time step
    c.method = method, c.T = 1, c.ny = ny, c.nx = nx, c.Ny = Ny, c.Nx = Nx;
    c.ld_out = Ny > 0 && Nx > 0 && Ny <= INT64_MAX / Nx ? Ny * Nx : 0;
    const RegridPlan pl = regrid_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const RegridAxis ay = regrid_axis(method, "y", src_y, ny, dst_y, Ny), ax = regrid_axis(method, "x", src_x, nx, dst_x, Nx);
    for (const RegridAxis* a : {&ay, &ax})
        if (a->error != SD_OK) return sd_set_error(a->error, "%s", a->message);
    std::vector<int32_t> idx;
    std::vector<double> wgt;
    for (const std::vector<int32_t>* v : {&ay.lo, &ay.hi, &ax.lo, &ax.hi}) idx.insert(idx.end(), v->begin(), v->end());
    for (const std::vector<double>* v : {&ay.t, &ay.r, &ax.t, &ax.r}) wgt.insert(wgt.end(), v->begin(), v->end());
    SD_HIP(hipSetDevice(ctx->device));
    sd_regrid* rg = new sd_regrid();
    rg->ctx = ctx, rg->method = method, rg->ny = ny, rg->nx = nx, rg->Ny = Ny, rg->Nx = Nx;
    return sd_state_build(rg, sd_regrid_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, regrid_bufs(rg)));
        SD_TRY(sd_state_copy(ctx, regrid_bufs(rg), {idx.data(), wgt.data()}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the host tables go away on return)
        return SD_OK;
    });
}

int sd_regrid_apply_dev(sd_ctx* ctx, const sd_regrid* rg, const void* src_dev, int src_is_f32, int64_t T, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && rg && src_dev && out_dev, "sd_regrid_apply: NULL argument");
    SD_CHECK_ARG(rg->ctx == ctx, "sd_regrid_apply: the state belongs to another context");
    const RegridPlan pl = regrid_plan(call_of(rg, T, ld_out, out_dev));
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(src_is_f32 ? launch<float>(ctx, rg, pl, src_dev, T, out_dev, ld_out) : launch<double>(ctx, rg, pl, src_dev, T, out_dev, ld_out));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_regrid_apply(sd_ctx* ctx, const sd_regrid* rg, const void* src_host, int src_is_f32, int64_t T, double* out_host) {
    SD_CHECK_ARG(ctx && rg && src_host && out_host, "sd_regrid_apply: NULL argument");
    const int64_t C = rg->Ny * rg->Nx;
    const RegridPlan pl = regrid_plan(call_of(rg, T, C, nullptr));  // (before the upload)
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * rg->ny * rg->nx;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_out(out_host, sizeof(double) * (size_t)T * C)};
    return with_device_copies(ctx, f, [&](void* const* d) { return sd_regrid_apply_dev(ctx, rg, d[0], src_is_f32, T, (double*)d[1], C); });
}

}  // extern "C"
