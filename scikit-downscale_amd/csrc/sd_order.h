// Device code the order-statistic units share (sd_quantile.hip, sd_twosample.hip): the gather of a group's rows into one LDS row per
// cell, the wave's sort of such a row, the runs stage of the series path and the launch helpers.  Everything here sits in an unnamed
// namespace: each unit has its own copy of the kernels, launched under the profiler names it gives them.
#pragma once
#include <iterator>
#include <type_traits>
#include <utility>

#include "sd_internal.h"
#include "sd_quantile_plan.h"
#include "sd_sortnet.h"
#include "sd_wave.h"

namespace {
using namespace sdw;

template <typename S>
struct pair_of;
template <>
struct pair_of<double> {
    using type = double2;
};
template <>
struct pair_of<float> {
    using type = float2;
};

// rows ord[0 .. n) of the field for the 8 cells from c0 -> the LDS rows tile[cell * RS + r] (cell-major), widened to float64.  A
// thread owns the cell pair (tid & 3) of the rows tid >> 2, + 128, ...; n <= 64 * K.
template <typename S, int K>
__device__ __forceinline__ void gather_tile(const S* __restrict__ src, int64_t ld, const int32_t* __restrict__ ord, int n, int64_t c0, int64_t C,
                                            bool vec, double* tile) {
    constexpr int NR = (kWave * K + kRowsPerPass - 1) / kRowsPerPass;
    constexpr int RS = tile_sort_rs(K);
    const int tid = tid_now();
    const int cp = tid & 3, rr = tid >> 2;
    const int64_t c = c0 + 2 * cp;
    const bool full = vec && c + 1 < C;
    const char* const col = reinterpret_cast<const char*>(src + c);
    const uint32_t pitch = (uint32_t)ld * (uint32_t)sizeof(S);  // (the plan: 8 * ld < 2^32)
    int ti[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int r = rr + k * kRowsPerPass;
        ti[k] = ord[r < n ? r : 0];
    }
    double v0[NR], v1[NR];
    if (full) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const auto v = *reinterpret_cast<const typename pair_of<S>::type*>(col + (uint64_t)(uint32_t)ti[k] * (uint64_t)pitch);
            v0[k] = (double)v.x;
            v1[k] = (double)v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const S* p = reinterpret_cast<const S*>(col + (uint64_t)(uint32_t)ti[k] * (uint64_t)pitch);
            v0[k] = c < C ? (double)p[0] : 0.0;
            v1[k] = c + 1 < C ? (double)p[1] : 0.0;
        }
    }
    double* const d0 = tile + (2 * cp) * RS;
    double* const d1 = d0 + RS;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int r = rr + k * kRowsPerPass;
        if (r < n) {
            d0[r] = v0[k];
            d1[r] = v1[k];
        }
    }
}

// the wave's commit step: row[0 .. n) -> K consecutive samples per lane, NaN and the slots from n on as +inf; row[0 .. nsort) sorted
// in place (nsort >= n slots are elements: the pads sort behind the data).  Returns the number of non-NaN samples, wave-uniform.
template <int K>
__device__ __forceinline__ int sort_row(double* row, int n, int nsort, int lane) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double v[K];
    int bad = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int j = K * lane + i;  // (lane stride K is odd: conflict-free)
        const double t = row[j < n ? j : 0];
        const bool nan = t != t;
        bad += (j < n && nan) ? 1 : 0;
        v[i] = (j < n && !nan) ? t : inf;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad += __shfl_xor(bad, o, kWave);
    wave_fence();
    sort_segment<K>(v, row, nsort, lane);
    return n - bad;
}

template <typename S, int K>
__global__ void __launch_bounds__(kThreads)
    quantile_runs_kernel(const S* __restrict__ src, int64_t ld, int64_t C, const int32_t* __restrict__ rows, const QuantileChunk* __restrict__ chunks,
                         int64_t nchunks, int64_t ntiles, int vec, double* __restrict__ runs, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = tile_sort_rs(K);
    constexpr int CHUNK = kWave * K;
    double* const tile = reinterpret_cast<double*>(smem_raw) + kHeadDoubles;
    const int64_t tile_id = sdqt::tile_of_block(blockIdx.x, ntiles), item = sdqt::item_of_block(blockIdx.x, ntiles);
    if (tile_id >= ntiles || item >= nchunks) return;
    const int64_t c0 = tile_id * kW;
    const QuantileChunk ch = chunks[item];  // workgroup-uniform
    const int tid = tid_now();
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave;
    double* const row = tile + wave * RS;
    gather_tile<S, K>(src, ld, rows + ch.start, ch.len, c0, C, vec != 0, tile);
    __syncthreads();
    const int nv = sort_row<K>(row, ch.len, CHUNK, lane);
    const int64_t c = c0 + wave;
    if (c >= C) return;
    double* const dst = runs + ch.base + c * (int64_t)ch.np + ch.local;
#pragma unroll
    for (int i = 0; i < K; ++i) dst[lane + i * kWave] = row[lane + i * kWave];
    if (lane == 0) counts[item * C + c] = nv;
}

template <class Kernel>
int allow_lds(Kernel kernel, size_t lds) {
    SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return SD_OK;
}

template <const auto& Widths, class F, size_t... I>
int dispatch_width(int K, F& f, const char* who, std::index_sequence<I...>) {
    int rc = SD_OK;
    const bool found = ((K == Widths[I] && ((rc = f(std::integral_constant<int, Widths[I]>{})), true)) || ...);
    return found ? rc : sd_set_error(SD_ERR_INVALID, "%s: width %d not instantiated", who, K);
}
template <const auto& Widths, class F>
int dispatch_width(int K, F f, const char* who = "sd_quantile") {
    return dispatch_width<Widths>(K, f, who, std::make_index_sequence<std::size(Widths)>{});
}

// profiler names: the width is part of the name, so that a profile (and a test) tells which instantiation served a call
template <int K>
constexpr const char* runs_name() {
    static_assert(K == 13 || K == 17 || K == 19, "name the new width");
    return K == 13 ? "quantile_runs_kernel<13>" : K == 17 ? "quantile_runs_kernel<17>" : "quantile_runs_kernel<19>";
}

}  // namespace
