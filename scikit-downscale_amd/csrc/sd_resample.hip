// Resampling of the time axis of a [T, C] field (GridArray.resample(time=rule).mean() / .sum(); pandas' DataFrame.resample(rule)
// .mean() / .sum() per cell): bin m is the run of rows offsets[m] .. offsets[m + 1] - 1, made by pandas on the host.  The launch plan
// and the refusals are in sd_resample_plan.h.
//
// resample_kernel<S, V, OP>: a workgroup of four waves owns one tile of 64 * V adjacent cells and a run of kBinsPerGroup consecutive
// bins; each wave takes kBinsPerWave whole bins, one after the other.  A lane owns its V cells for the whole bin and adds their
// samples in time order, so a result depends neither on the launch geometry nor on how a caller cuts the time axis into blocks of
// whole bins.  One row of the tile is one coalesced load per wave (V * sizeof(S) bytes per lane, 16 where the plan allows); the loads
// of a batch of kBatch rows are issued before any of their arithmetic.  A row past the end of the bin reads the bin's last row again
// and is not counted, so a bin of any length -- 1 and a partial batch included -- runs the same code; an empty bin runs no batch at
// all.  NaN samples are skipped by a select, the count is an int per cell.  One store of V doubles per lane and bin; no LDS, no
// atomics.  Algorithmic bytes: sizeof(S) * T * C read + 8 * M * C written.
//
// mean: sum / count, NaN without a sample (an empty bin and an all-NaN bin alike).  sum: 0 without a sample (pandas' min_count=0).
// inf follows IEEE arithmetic.  Plain summation (pandas compensates; both stay within n * 2^-53 * sum|x| of the exact sum).
//
// A bin is never split across lanes: one very long bin over few cells has little parallelism.  That is the price of the fixed order.
#include <vector>

#include "sd_internal.h"
#include "sd_resample_plan.h"
#include "sd_state.h"

namespace {
using namespace sdrs;

template <typename S, int V>
struct alignas(sizeof(S) * V) Cells {
    S v[V];
};

template <typename S, int V, int OP>
__global__ void __launch_bounds__(kLanes* kWaves) resample_kernel(const S* __restrict__ src, int64_t ld, int64_t C,
                                                                 const int64_t* __restrict__ offsets, int64_t M, int64_t ctiles,
                                                                 double* __restrict__ out, int64_t ld_out) {
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t ctile = blockIdx.x % ctiles, group = blockIdx.x / ctiles;
    const int64_t c0 = (ctile * kLanes + lane) * V;  // (V divides C: the V cells are inside or outside together)
    if (c0 >= C) return;
    const int64_t m0 = group * kBinsPerGroup + (int64_t)wave * kBinsPerWave;
    const S* const col = src + c0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int b = 0; b < kBinsPerWave; ++b) {
        const int64_t m = m0 + b;
        if (m >= M) break;  // wave-uniform
        const int64_t r0 = offsets[m], r1 = offsets[m + 1];
        double acc[V];
        int cnt[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0, cnt[v] = 0;
        for (int64_t r = r0; r < r1; r += kBatch) {
            Cells<S, V> q[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) q[u] = *reinterpret_cast<const Cells<S, V>*>(col + min(r + u, r1 - 1) * ld);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool inside = r + u < r1;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double x = (double)q[u].v[v];
                    const bool take = inside && x == x;
                    acc[v] += take ? x : 0.0;
                    cnt[v] += take ? 1 : 0;
                }
            }
        }
        double res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if constexpr (OP == SD_RESAMPLE_MEAN)
                res[v] = cnt[v] > 0 ? acc[v] / (double)cnt[v] : nan;
            else
                res[v] = acc[v];
        }
        double* const o = out + m * ld_out + c0;
        if constexpr (V == 1) {
            *o = res[0];
        } else {
#pragma unroll
            for (int v = 0; v < V; v += 2) *reinterpret_cast<double2*>(o + v) = make_double2(res[v], res[v + 1]);
        }
    }
}

template <typename S, int V>
int launch_op(sd_ctx* ctx, const ResampleCall& c, const ResamplePlan& pl, const S* src, const int64_t* offsets, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    if (c.op == SD_RESAMPLE_MEAN)
        SD_LAUNCH(ctx, "resample_kernel", (resample_kernel<S, V, SD_RESAMPLE_MEAN>), grid, block, 0, src, c.ld, c.C, offsets, c.M, pl.ctiles, out,
                  c.ld_out);
    else
        SD_LAUNCH(ctx, "resample_kernel", (resample_kernel<S, V, SD_RESAMPLE_SUM>), grid, block, 0, src, c.ld, c.C, offsets, c.M, pl.ctiles, out,
                  c.ld_out);
    return SD_OK;
}

int launch(sd_ctx* ctx, const ResampleCall& c, const ResamplePlan& pl, const void* src, const int64_t* offsets, double* out) {
    if (c.src_is_f32) {
        const float* s = (const float*)src;
        return pl.cols == 4 ? launch_op<float, 4>(ctx, c, pl, s, offsets, out)
               : pl.cols == 2 ? launch_op<float, 2>(ctx, c, pl, s, offsets, out)
                              : launch_op<float, 1>(ctx, c, pl, s, offsets, out);
    }
    const double* s = (const double*)src;
    return pl.cols == 2 ? launch_op<double, 2>(ctx, c, pl, s, offsets, out) : launch_op<double, 1>(ctx, c, pl, s, offsets, out);
}

ResampleCall call_of(int op, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t M, int64_t ld_out, const void* src, const void* out) {
    ResampleCall c;
    c.op = op, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.M = M, c.ld_out = ld_out;
    c.src_aligned16 = ((uintptr_t)src & 15) == 0;
    c.out_aligned16 = ((uintptr_t)out & 15) == 0;
    return c;
}

}  // namespace

extern "C" {

int sd_resample_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int64_t* offsets,
                    int64_t M, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && src_dev && offsets && out_dev, "sd_resample: NULL argument");
    const ResampleCall c = call_of(op, src_is_f32, ld, T, C, M, ld_out, src_dev, out_dev);
    const ResamplePlan pl = resample_check_offsets(resample_plan(c), c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch table;
    SD_TRY(upload(ctx, table, std::vector<int64_t>(offsets, offsets + M + 1)));
    SD_TRY(launch(ctx, c, pl, src_dev, table.as<int64_t>(), out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_resample(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int64_t* offsets, int64_t M,
                double* out_host) {
    SD_CHECK_ARG(ctx && src_host && offsets && out_host, "sd_resample: NULL argument");
    const ResampleCall c = call_of(op, src_is_f32, C, T, C, M, C, nullptr, nullptr);  // (before the upload)
    const ResamplePlan pl = resample_check_offsets(resample_plan(c), c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_out(out_host, sizeof(double) * (size_t)M * C)};
    return with_device_copies(ctx, f, [&](void* const* d) { return sd_resample_dev(ctx, op, d[0], src_is_f32, C, T, C, offsets, M, (double*)d[1], C); });
}

}  // extern "C"
