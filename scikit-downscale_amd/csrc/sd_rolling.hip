// Rolling windows over the time axis of a [T, C] field (GridArray.rolling(time=w, center=..., min_periods=...).mean() / .sum() /
// .var() / .std(); pandas' fixed integer window per cell): output row t is a statistic of the rows t - back .. t - back + window - 1 of
// its own cell, clipped to the block or, with wrap, taken modulo T.  The launch plan and the refusals are in sd_rolling_plan.h.
//
// rolling_kernel<S, V, STAGED>: the cell tiling of sd_bins.h -- a workgroup of kWaves waves owns a tile of 64 * V adjacent cells -- and a
// run of `run` consecutive output rows; wave k takes the rows k, k + kWaves, ... of the run and a lane evaluates the windows of its V
// cells.  A window is evaluated directly and in time order: NaN samples are skipped by a select, s is their plain running sum from
// +0.0 and n the number of the others; var / std take a second pass over the same samples, q the running sum of (x - s / n)^2.  One IEEE
// operation per step (-ffp-contract=off).  A result depends on its own window only: neither the geometry, nor the cells per lane, nor a
// cut of the time axis changes a bit of it.  The price is O(window) work per output.
//
// The rows come through an accessor of unwrapped positions p (p = row, or row + / - T under wrap):
//   STAGED:  the workgroup first loads the run + window - 1 rows of its windows into LDS, kBatch loads in flight per wave, stored as S
//            with one row of the tile contiguous: a lane reads V * sizeof(S) bytes at lane * V * sizeof(S) of a row, so the column reads
//            of a wave are one contiguous row and conflict-free.  A position outside [0, T) is loaded from p mod T with wrap; without,
//            no window reads it (it holds the nearest row, so that the staging has no branch).
//   else:    the same loop reads row p (mod T) from global memory, kBatch loads in flight.
// Row arithmetic is wave-uniform.  No atomics, no scratch.  Algorithmic bytes: sizeof(S) * T * C read + 8 * T * C written; the staged
// path reads (run + window - 1) / run of that, mostly from L2.
#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_rolling_plan.h"
#include "sd_state.h"

namespace {
using namespace sdbn;

struct RollingArgs {
    int64_t ld, T, C, window, back, t0, n_out, ctiles, ld_out;
    int min_periods, ddof, op, wrap, run;
};

// row of the unwrapped position p in [-T, 2 T)
__device__ __forceinline__ int64_t row_mod(int64_t p, int64_t T) { return p < 0 ? p + T : p >= T ? p - T : p; }

// the statistic of the positions p0 .. p1 - 1 of the lane's cells, in that order; get(p) -> Cells<S, V>
template <typename S, int V, class Get>
__device__ __forceinline__ void window_statistic(Get get, int64_t p0, int64_t p1, const RollingArgs& a, double (&res)[V]) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double s[V], mean[V], q[V];
    int n[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0.0, q[v] = 0.0, n[v] = 0;
    for (int64_t p = p0; p < p1; p += kBatch) {
        Cells<S, V> x[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) x[u] = get(min(p + u, p1 - 1));
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const bool inside = p + u < p1;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double y = (double)x[u].v[v];
                const bool take = inside && y == y;
                s[v] += take ? y : 0.0;
                n[v] += take ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) mean[v] = n[v] > 0 ? s[v] / (double)n[v] : nan;
    if (a.op == SD_ROLLING_VAR || a.op == SD_ROLLING_STD) {  // wave-uniform
        for (int64_t p = p0; p < p1; p += kBatch) {
            Cells<S, V> x[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) x[u] = get(min(p + u, p1 - 1));
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool inside = p + u < p1;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double y = (double)x[u].v[v];
                    const double d = y - mean[v];
                    const double dd = d * d;
                    q[v] += (inside && y == y) ? dd : 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        double r;
        if (a.op == SD_ROLLING_SUM) {
            r = s[v];
        } else if (a.op == SD_ROLLING_MEAN) {
            r = mean[v];
        } else {
            const int dof = n[v] - a.ddof;
            r = dof > 0 ? q[v] / (double)dof : nan;
            if (a.op == SD_ROLLING_STD) r = sqrt(r);
        }
        res[v] = n[v] >= a.min_periods ? r : nan;
    }
}

template <typename S, int V, bool STAGED>
__global__ void __launch_bounds__(kLanes* kWaves) rolling_kernel(const S* __restrict__ src, double* __restrict__ out, RollingArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Cells<S, V>* const lds = reinterpret_cast<Cells<S, V>*>(lds_raw);
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t ctile = blockIdx.x % a.ctiles, rgroup = blockIdx.x / a.ctiles;
    const int64_t c0 = (ctile * kLanes + lane) * V;
    const bool mine = c0 < a.C;  // (V divides C: the V cells are inside or outside together; the same lanes in every wave)
    const int64_t ta = a.t0 + rgroup * a.run, tb = min(a.t0 + a.n_out, ta + a.run);  // the output rows of the workgroup, wave-uniform
    const int64_t first = ta - a.back;                                              // the first position of its windows
    const S* const col = src + (mine ? c0 : 0);  // (a lane past C stages cell 0 again, into its own slot, and leaves after the barrier)
    if constexpr (STAGED) {
        // staged row j holds position first + j; without wrap a position outside [0, T) holds the nearest row and is never read
        const int64_t staged = (tb - ta) + a.window - 1;
        const auto row_of = [&](int64_t j) { return a.wrap ? row_mod(first + j, a.T) : min(max(first + j, (int64_t)0), a.T - 1); };
        for (int64_t j0 = (int64_t)wave * kBatch; j0 < staged; j0 += kWaves * kBatch) {
            Cells<S, V> x[kBatch];
            load_batch(x, col, a.ld, j0, staged, row_of);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) lds[min(j0 + u, staged - 1) * kLanes + lane] = x[u];  // (past the end: the last row again)
        }
        __syncthreads();
    }
    if (!mine) return;
    for (int64_t t = ta + wave; t < tb; t += kWaves) {
        int64_t p0 = t - a.back, p1 = p0 + a.window;
        if (!a.wrap) p0 = max(p0, (int64_t)0), p1 = min(p1, a.T);
        double res[V];
        if constexpr (STAGED)
            window_statistic<S, V>([&](int64_t p) { return lds[(int)(p - first) * kLanes + lane]; }, p0, p1, a, res);
        else
            window_statistic<S, V>(
                [&](int64_t p) { return *reinterpret_cast<const Cells<S, V>*>(col + (a.wrap ? row_mod(p, a.T) : p) * a.ld); }, p0, p1, a, res);
        store_doubles<V>(out + (t - a.t0) * a.ld_out + c0, res);
    }
}

int launch(sd_ctx* ctx, const RollingCall& c, const RollingPlan& pl, const void* src, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    RollingArgs a;
    a.ld = c.ld, a.T = c.T, a.C = c.C, a.window = c.window, a.back = c.back, a.t0 = c.t0, a.n_out = c.n_out, a.ctiles = pl.ctiles, a.ld_out = c.ld_out;
    a.min_periods = (int)(c.min_periods < INT32_MAX ? c.min_periods : INT32_MAX), a.ddof = (int)(c.ddof < INT32_MAX ? c.ddof : INT32_MAX), a.op = c.op, a.wrap = c.wrap, a.run = pl.run;
    return with_cells(c.src_is_f32, pl.cols, src, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
        if (pl.staged)
            SD_LAUNCH(ctx, "rolling_kernel", (rolling_kernel<S, V, true>), grid, block, (size_t)pl.lds_bytes, s, out, a);
        else
            SD_LAUNCH(ctx, "rolling_unstaged_kernel", (rolling_kernel<S, V, false>), grid, block, 0, s, out, a);
        return (int)SD_OK;
    });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

RollingCall rolling_call(int op, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t window, int64_t back, int64_t min_periods, int64_t ddof,
                         int wrap, int64_t t0, int64_t n_out, int64_t ld_out, const void* src, const void* out) {
    RollingCall c;
    c.op = op, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.window = window, c.back = back, c.min_periods = min_periods, c.ddof = ddof, c.wrap = wrap != 0;
    c.t0 = t0, c.n_out = n_out, c.ld_out = ld_out;
    c.src_aligned16 = aligned16(src), c.out_aligned16 = aligned16(out);
    return c;
}

}  // namespace

extern "C" {

int sd_rolling_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t window, int64_t back,
                   int64_t min_periods, int64_t ddof, int wrap, int64_t t0, int64_t n_out, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && src_dev && out_dev, "sd_rolling: NULL argument");
    const RollingCall c = rolling_call(op, src_is_f32, ld, T, C, window, back, min_periods, ddof, wrap, t0, n_out, ld_out, src_dev, out_dev);
    const RollingPlan pl = rolling_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(launch(ctx, c, pl, src_dev, out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_rolling(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, int64_t window, int64_t back,
               int64_t min_periods, int64_t ddof, int wrap, double* out_host) {
    SD_CHECK_ARG(ctx && src_host && out_host, "sd_rolling: NULL argument");
    const RollingCall c = rolling_call(op, src_is_f32, C, T, C, window, back, min_periods, ddof, wrap, 0, T, C, nullptr, nullptr);  // (before the upload)
    const RollingPlan pl = rolling_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t cells = (size_t)T * C;
    const sd_host_field f[] = {sd_in(src_host, (src_is_f32 ? sizeof(float) : sizeof(double)) * cells), sd_out(out_host, sizeof(double) * cells)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_rolling_dev(ctx, op, d[0], src_is_f32, C, T, C, window, back, min_periods, ddof, wrap, 0, T, (double*)d[1], C);
    });
}

}  // extern "C"
