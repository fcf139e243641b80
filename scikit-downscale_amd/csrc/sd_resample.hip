// Resampling of the time axis of a [T, C] field (GridArray.resample(time=rule).mean() / .sum(); pandas' DataFrame.resample(rule)
// .mean() / .sum() per cell): bin m is the run of rows offsets[m] .. offsets[m + 1] - 1, made by pandas on the host.  The launch plan
// and the refusals are in sd_resample_plan.h.
//
// resample_kernel<S, V, OP>: the geometry, the batched loads and the statistic of a bin are those of sd_bins.h.  A lane adds the
// samples of its V cells in time order, so a result depends neither on the launch geometry nor on how a caller cuts the time axis
// into blocks of whole bins.  One store of V doubles per lane and bin; no LDS, no atomics.  Algorithmic bytes: sizeof(S) * T * C read
// + 8 * M * C written.
//
// mean: sum / count, NaN without a sample (an empty bin and an all-NaN bin alike).  sum: 0 without a sample (pandas' min_count=0).
// inf follows IEEE arithmetic.  Plain summation (pandas compensates; both stay within n * 2^-53 * sum|x| of the exact sum).
//
// A bin is never split across lanes: one very long bin over few cells has little parallelism.  That is the price of the fixed order.
#include <vector>

#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_resample_plan.h"
#include "sd_state.h"

namespace {
using namespace sdbn;

template <typename S, int V, int OP>
__global__ void __launch_bounds__(kLanes* kWaves) resample_kernel(const S* __restrict__ src, int64_t ld, int64_t C,
                                                                 const int64_t* __restrict__ offsets, int64_t M, int64_t ctiles,
                                                                 double* __restrict__ out, int64_t ld_out) {
    int64_t c0, m0;
    if (!lane_place<V>(ctiles, C, c0, m0)) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int b = 0; b < kBinsPerWave; ++b) {
        const int64_t m = m0 + b;
        if (m >= M) break;  // wave-uniform
        double acc[V], res[V];
        int cnt[V];
        bin_statistic<S, V>(src + c0, ld, offsets[m], offsets[m + 1], [](int64_t r) { return r; }, acc, cnt);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if constexpr (OP == SD_RESAMPLE_MEAN)
                res[v] = cnt[v] > 0 ? acc[v] / (double)cnt[v] : nan;
            else
                res[v] = acc[v];
        }
        store_doubles<V>(out + m * ld_out + c0, res);
    }
}

int launch(sd_ctx* ctx, const ResampleCall& c, const ResamplePlan& pl, const void* src, const int64_t* offsets, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    return with_cells(c.src_is_f32, pl.cols, src, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
        if (c.op == SD_RESAMPLE_MEAN)
            SD_LAUNCH(ctx, "resample_kernel", (resample_kernel<S, V, SD_RESAMPLE_MEAN>), grid, block, 0, s, c.ld, c.C, offsets, c.M, pl.ctiles, out,
                      c.ld_out);
        else
            SD_LAUNCH(ctx, "resample_kernel", (resample_kernel<S, V, SD_RESAMPLE_SUM>), grid, block, 0, s, c.ld, c.C, offsets, c.M, pl.ctiles, out,
                      c.ld_out);
        return (int)SD_OK;
    });
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
