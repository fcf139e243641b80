// Device side of the binned time-axis kernels (resample_kernel: sd_resample.hip, disagg_kernel: sd_disagg.hip, groupby_reduce_kernel
// and groupby_apply_kernel: sd_groupby.hip); the geometry is that of sd_bins_plan.h.  A workgroup of kWaves waves owns one tile of 64 * V adjacent cells and a run of kBinsPerGroup consecutive bins;
// each wave takes kBinsPerWave whole bins, one after the other, and a lane owns its V cells for the whole bin.  One row of the tile
// is one coalesced load per wave (V * sizeof(S) bytes per lane, 16 where the plan allows); the loads of a batch of kBatch rows are
// issued before any of their arithmetic.  A row past the end of the bin reads the bin's last row again and is not counted, so a bin
// of any length -- 1 and a partial batch included -- runs the same code; an empty bin runs no batch at all.
//
// bin_statistic is the one statistic of both kernels: the samples of a cell in time order, NaN samples skipped by a select, acc
// their plain running sum and cnt the number of the others.  resample then disaggregate(years='same') gives the observations back
// bit for bit because both kernels call it.  bin_accumulate is its seeded form: acc and cnt continue from what the caller put there
// (groupby_reduce_kernel carries them from one block of the time axis to the next).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sd_bins_plan.h"

namespace sdbn {

template <typename S, int V>
struct alignas(sizeof(S) * V) Cells {
    S v[V];
};

// V doubles at a multiple of min(V, 2) * 8 bytes: 16-byte accesses where V allows
template <int V>
__device__ __forceinline__ void load_doubles(const double* p, double (&x)[V]) {
    if constexpr (V == 1) {
        x[0] = *p;
    } else {
#pragma unroll
        for (int v = 0; v < V; v += 2) {
            const double2 q = *reinterpret_cast<const double2*>(p + v);
            x[v] = q.x, x[v + 1] = q.y;
        }
    }
}

template <int V>
__device__ __forceinline__ void store_doubles(double* p, const double (&x)[V]) {
    if constexpr (V == 1) {
        *p = x[0];
    } else {
#pragma unroll
        for (int v = 0; v < V; v += 2) *reinterpret_cast<double2*>(p + v) = make_double2(x[v], x[v + 1]);
    }
}

// the place of a lane in a grid of ctiles cell tiles by runs of bins: its first cell c0 and its wave's first bin m0 (wave-uniform).
// false: the lane's cells lie past C (V divides C: the V cells are inside or outside together)
// (BPW: the whole bins of a wave, kBinsPerWave unless a plan chose otherwise)
template <int V, int BPW = kBinsPerWave>
__device__ __forceinline__ bool lane_place(int64_t ctiles, int64_t C, int64_t& c0, int64_t& m0) {
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t ctile = blockIdx.x % ctiles, bins = blockIdx.x / ctiles;
    c0 = (ctile * kLanes + lane) * V;
    m0 = bins * (kWaves * BPW) + (int64_t)wave * BPW;
    return c0 < C;
}

// the batch of rows r .. r + kBatch - 1 of the bin that ends before r1, of the lane's cells at col: row i of the bin is row
// row_of(i) of the field (rows ld apart)
template <typename S, int V, class Row>
__device__ __forceinline__ void load_batch(Cells<S, V> (&q)[kBatch], const S* col, int64_t ld, int64_t r, int64_t r1, Row row_of) {
#pragma unroll
    for (int u = 0; u < kBatch; ++u) q[u] = *reinterpret_cast<const Cells<S, V>*>(col + row_of(min(r + u, r1 - 1)) * ld);
}

template <typename S, int V, class Row>
__device__ __forceinline__ void bin_accumulate(const S* col, int64_t ld, int64_t r0, int64_t r1, Row row_of, double (&acc)[V], int (&cnt)[V]) {
    for (int64_t r = r0; r < r1; r += kBatch) {
        Cells<S, V> q[kBatch];
        load_batch(q, col, ld, r, r1, row_of);
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
}

template <typename S, int V, class Row>
__device__ __forceinline__ void bin_statistic(const S* col, int64_t ld, int64_t r0, int64_t r1, Row row_of, double (&acc)[V], int (&cnt)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0, cnt[v] = 0;
    bin_accumulate<S, V>(col, ld, r0, r1, row_of, acc, cnt);
}

// f(the source as const float* or const double*, std::integral_constant<int, cols>) for the (is_f32, cols) of a plan
template <class F>
int with_cells(bool is_f32, int cols, const void* src, F f) {
    using std::integral_constant;
    if (is_f32) {
        const float* s = (const float*)src;
        return cols == 4 ? f(s, integral_constant<int, 4>()) : cols == 2 ? f(s, integral_constant<int, 2>()) : f(s, integral_constant<int, 1>());
    }
    const double* s = (const double*)src;
    return cols == 2 ? f(s, integral_constant<int, 2>()) : f(s, integral_constant<int, 1>());
}

}  // namespace sdbn
