// Step 1 of the constructed-analog rule (include/sd_downscale.h), shared by sd_constructed.hip and sd_localized.hip: which coarse
// columns are used.  ca_columns_kernel: one thread per coarse column walks the library rows and says whether the column is used (finite
// throughout and wc > 0).  The flags come back to the host (at most 2^16 ints; the only host round trip of a call).  Everything has
// internal linkage: each unit that includes this file gets its own copy of the kernel.
#pragma once
#include <vector>

#include "sd_internal.h"
#include "sd_state.h"

namespace {

__device__ __forceinline__ double ca_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double ca_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ bool ca_finite(double v) { return fabs(v) < ca_inf(); }  // (false for NaN)

__global__ void __launch_bounds__(256) ca_columns_kernel(const double* __restrict__ L, int64_t ld_l, int64_t Tl, int Cc,
                                                         const double* __restrict__ wc, int32_t* __restrict__ used) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cc) return;
    bool ok = wc[c] > 0.0;
    for (int64_t t = 0; t < Tl; ++t) ok = ok && ca_finite(L[t * ld_l + c]);
    used[c] = ok ? 1 : 0;
}

// used[c] != 0 for the used columns of a call, on the host; SD_ERR_INVALID where none is
int ca_column_flags(sd_ctx* ctx, const char* who, const double* L_dev, int64_t ld_l, int64_t Tl, int64_t Cc, const double* wc,
                    std::vector<int32_t>& used) {
    sd_scratch wc_dev, flags;
    SD_TRY(upload(ctx, wc_dev, std::vector<double>(wc, wc + Cc)));
    SD_HIP(flags.alloc(ctx, sizeof(int32_t) * Cc));
    const dim3 grid((unsigned)((Cc + 255) / 256)), block(256);
    SD_LAUNCH(ctx, "ca_columns_kernel", ca_columns_kernel, grid, block, 0, L_dev, ld_l, Tl, (int)Cc, (const double*)wc_dev.p, flags.as<int32_t>());
    used.assign((size_t)Cc, 0);
    SD_HIP(hipMemcpyAsync(used.data(), flags.p, sizeof(int32_t) * Cc, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t c = 0; c < Cc; ++c)
        if (used[(size_t)c] != 0) return SD_OK;
    return sd_set_error(SD_ERR_INVALID, "%s: no column is used (a column needs a library that is finite in every row and wc > 0)", who);
}

}  // namespace
