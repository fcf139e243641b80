// Order statistics over the time axis of a [T, C] field (GridArray.quantile / .median: np.nanquantile(method=...) / np.nanmedian per
// cell and group): the per-cell sorts of the BCSD and quantile-mapping kernels with another last step.  The launch plan, the
// refusals and the tables of the series path are in sd_quantile_plan.h; the group table is the counting sort of sd_groupby_plan.h.
//
// quantile_segment_kernel<S, K>: one 512-thread workgroup = 8 adjacent cells x one group of at most 64 * K rows.  The rows of the
// group are gathered through its row table as 64-byte fragments (4 lanes x 16 bytes; 4 x 8 bytes of a float32 source; scalar loads
// where ld or the pointer do not allow them), all loads of a thread issued before the first use, and transposed into one LDS row per
// cell.  The wave that owns a cell takes K consecutive samples per lane; a NaN becomes the +inf pad there and is counted (NaN never
// enters a min / max network), sdw::sort_segment<K> sorts the row in place, and lane i evaluates quantiles i, i + 64, ... from it and
// stores out[q * G + g, c].  Algorithmic bytes: sizeof(S) * T * C read, 8 * Q * G * C written.
//
// quantile_runs_kernel<S, K> + quantile_select_kernel<K> (groups longer than the widest segment): the first is the segment kernel on
// chunks of 64 * K rows of a group, whose sorted runs go to scratch as [group][cell][np_g] (512 consecutive bytes per wave store)
// with the count of the chunk's non-NaN samples beside them; the second, one 1 024-thread workgroup per (group, cell), merges the at
// most 16 runs in LDS (sdsort::block_merge_rounds from round 6) and evaluates the quantiles.  Pads and NaN are +inf: they sort behind
// (or among) the data, and the first `count` slots are the valid samples.
//
// Every result is one fixed sequence of IEEE operations on the sorted samples (-ffp-contract=off): it depends neither on the order
// of a group's rows, nor on the layout, nor on the path.
//
// gather_tile, sort_row, quantile_runs_kernel and the launch helpers are in sd_order.h, shared with sd_twosample.hip.
#include <vector>

#include "sd_groupby_plan.h"
#include "sd_internal.h"
#include "sd_order.h"
#include "sd_quantile_plan.h"
#include "sd_sortnet.h"
#include "sd_state.h"
#include "sd_wave.h"

namespace {
using namespace sdw;

// one quantile of the sorted samples v[0 .. nv) of a group of n rows (sd_downscale.h: sd_quantile)
__device__ __forceinline__ double quantile_eval(const double* v, int nv, int n, int method, int skipna, double q) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (nv == 0 || (!skipna && nv < n)) return nan;
    if (method == SD_QUANTILE_MEDIAN) {
        const int m = nv >> 1;
        return (nv & 1) ? v[m] : (v[m - 1] + v[m]) / 2.0;
    }
    const double h = (double)(nv - 1) * q;
    const int lo = (int)h;  // floor: h >= 0
    const double g = h - (double)lo;
    const int hi = lo + 1 < nv - 1 ? lo + 1 : nv - 1;
    if (method == SD_QUANTILE_LOWER) return v[lo];
    if (method == SD_QUANTILE_HIGHER) return v[g > 0.0 ? hi : lo];
    if (method == SD_QUANTILE_NEAREST) return v[(int)__builtin_rint(h)];
    const double a = v[lo], b = v[hi], d = b - a;
    if (method == SD_QUANTILE_MIDPOINT) return g == 0.0 ? a : b - d * 0.5;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

template <typename S, int K>
__global__ void __launch_bounds__(kThreads)
    quantile_segment_kernel(const S* __restrict__ src, int64_t ld, int64_t C, const int32_t* __restrict__ rows, const int32_t* __restrict__ offsets,
                            int64_t G, int64_t ntiles, int vec, int method, int skipna, const double* __restrict__ q, int Q,
                            double* __restrict__ out, int64_t ld_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = tile_sort_rs(K);
    double* const tile = reinterpret_cast<double*>(smem_raw) + kHeadDoubles;  // (no row at LDS address 0: sd_wave_consts.h)
    const int64_t tile_id = sdqt::tile_of_block(blockIdx.x, ntiles), g = sdqt::item_of_block(blockIdx.x, ntiles);
    if (tile_id >= ntiles || g >= G) return;
    const int64_t c0 = tile_id * kW;
    const int beg = offsets[g], n = offsets[g + 1] - beg;  // workgroup-uniform
    const int tid = tid_now();
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave;
    double* const row = tile + wave * RS;
    int nv = 0;
    if (n > 0) {
        gather_tile<S, K>(src, ld, rows + beg, n, c0, C, vec != 0, tile);
        __syncthreads();
        nv = sort_row<K>(row, n, n, lane);
    }
    const int64_t c = c0 + wave;
    if (c >= C) return;
    for (int i = lane; i < Q; i += kWave) out[((int64_t)i * G + g) * ld_out + c] = quantile_eval(row, nv, n, method, skipna, q[i]);
}

template <int K>
__global__ void __launch_bounds__(sdqt::kSelectThreads)
    quantile_select_kernel(const double* __restrict__ runs, const int32_t* __restrict__ counts, const QuantileGroup* __restrict__ groups, int64_t G,
                           int64_t C, int method, int skipna, const double* __restrict__ q, int Q, double* __restrict__ out, int64_t ld_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* const buf = reinterpret_cast<double*>(smem_raw);  // np + 1 keys, then nthr + 1 co-ranks
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int64_t item = blockIdx.x; item < G * C; item += gridDim.x) {
        const int64_t g = item / C, c = item % C;
        const QuantileGroup gr = groups[g];  // workgroup-uniform
        const int np = gr.np;
        int nv = 0;
        __syncthreads();  // the keys of the last item have been read
        if (np > 0) {
            const double* const rc = runs + gr.base + c * (int64_t)np;
            for (int i = tid; i <= np; i += nthr) buf[i] = i < np ? rc[i] : inf;
            for (int j = 0; j < gr.nchunks; ++j) nv += counts[(int64_t)(gr.chunk0 + j) * C + c];
            __syncthreads();
            sdsort::block_merge_rounds<K>(buf, np, reinterpret_cast<int*>(buf + np + 1), tid, nthr, 6);
        }
        for (int i = tid; i < Q; i += nthr) out[((int64_t)i * G + g) * ld_out + c] = quantile_eval(buf, nv, gr.n, method, skipna, q[i]);
    }
}

// profiler names: the width is part of the name, so that a profile (and a test) tells which instantiation served a call
template <int K>
constexpr const char* segment_name() {
    static_assert(K == 5 || K == 13 || K == 21, "name the new width");
    return K == 5 ? "quantile_segment_kernel<5>" : K == 13 ? "quantile_segment_kernel<13>" : "quantile_segment_kernel<21>";
}
template <int K>
constexpr const char* select_name() {
    return K == 13 ? "quantile_select_kernel<13>" : K == 17 ? "quantile_select_kernel<17>" : "quantile_select_kernel<19>";
}

struct QuantileArgs {
    const void* src;
    const int32_t* rows;     // device [T]
    const int32_t* offsets;  // device [G + 1]
    const double* q;         // device [Q]
    double* out;
};

template <typename S>
int launch_segment(sd_ctx* ctx, const QuantileCall& c, const QuantilePlan& pl, const QuantileArgs& a) {
    return dispatch_width<sdqt::kSegWidths>(pl.K, [&](auto k) -> int {
        SD_TRY(allow_lds(&quantile_segment_kernel<S, k>, pl.lds));
        SD_LAUNCH(ctx, segment_name<k>(), (quantile_segment_kernel<S, k>), dim3((unsigned)pl.blocks), dim3(kThreads), pl.lds, (const S*)a.src,
                  c.ld, c.C, a.rows, a.offsets, c.G, pl.ntiles, (int)pl.vec, c.method, (int)c.skipna, a.q, (int)pl.Q, a.out, c.ld_out);
        return SD_OK;
    });
}

template <typename S>
int launch_series(sd_ctx* ctx, const QuantileCall& c, const QuantilePlan& pl, const QuantileArgs& a, const QuantileChunk* chunks,
                  const QuantileGroup* groups, double* runs, int32_t* counts) {
    return dispatch_width<sdqt::kSeriesWidths>(pl.K, [&](auto k) -> int {
        SD_TRY(allow_lds(&quantile_runs_kernel<S, k>, pl.lds));
        SD_LAUNCH(ctx, runs_name<k>(), (quantile_runs_kernel<S, k>), dim3((unsigned)pl.blocks), dim3(kThreads), pl.lds, (const S*)a.src, c.ld,
                  c.C, a.rows, chunks, pl.chunks, pl.ntiles, (int)pl.vec, runs, counts);
        SD_TRY(allow_lds(&quantile_select_kernel<k>, pl.select_lds));
        SD_LAUNCH(ctx, select_name<k>(), (quantile_select_kernel<k>), dim3((unsigned)pl.select_blocks), dim3(sdqt::kSelectThreads),
                  pl.select_lds, (const double*)runs, (const int32_t*)counts, groups, c.G, c.C, c.method, (int)c.skipna, a.q, (int)pl.Q, a.out,
                  c.ld_out);
        return SD_OK;
    });
}

QuantileCall quantile_call(const sd_ctx* ctx, int method, int skipna, int src_is_f32, int64_t ld, int64_t T, int64_t C, bool grouped, int64_t G,
                           const double* q, int64_t Q, int64_t ld_out, const void* src) {
    QuantileCall c;
    c.method = method, c.skipna = skipna != 0, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.G = grouped ? G : 1, c.Q = Q, c.q = q, c.ld_out = ld_out;
    c.src_aligned16 = ((uintptr_t)src & 15) == 0;
    c.lds_max = ctx->lds_max, c.cu_count = ctx->cu_count;
    return c;
}

}  // namespace

extern "C" {

int sd_quantile_dev(sd_ctx* ctx, int method, int skipna, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C,
                    const int32_t* group, int64_t G, const double* q, int64_t Q, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && src_dev && out_dev && (q || method == SD_QUANTILE_MEDIAN), "sd_quantile: NULL argument");
    const QuantileCall c = quantile_call(ctx, method, skipna, src_is_f32, ld, T, C, group != nullptr, G, q, Q, ld_out, src_dev);
    QuantilePlan pl = quantile_groups(quantile_check(c), group, T, c.G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    if (T >= sdqt::kGridLimit) pl = quantile_row_limits(pl, c);  // (no table of 2^31 rows is built)
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    std::vector<int64_t> rows64((size_t)T), offsets64((size_t)c.G + 1);
    if (group != nullptr) {
        groupby_tables(group, T, c.G, rows64.data(), offsets64.data());
    } else {
        for (int64_t t = 0; t < T; ++t) rows64[t] = t;
        offsets64[0] = 0, offsets64[1] = T;
    }
    pl = quantile_plan(pl, c, offsets64.data());
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const std::vector<int32_t> rows(rows64.begin(), rows64.end()), offsets(offsets64.begin(), offsets64.end());
    const std::vector<double> qs = method == SD_QUANTILE_MEDIAN ? std::vector<double>{0.5} : std::vector<double>(q, q + Q);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch drows, doffsets, dq;
    SD_TRY(upload(ctx, drows, rows));
    SD_TRY(upload(ctx, doffsets, offsets));
    SD_TRY(upload(ctx, dq, qs));
    const QuantileArgs a = {src_dev, drows.as<int32_t>(), doffsets.as<int32_t>(), dq.as<double>(), out_dev};
    if (pl.path == sdqt::kSegment) {
        SD_TRY(c.src_is_f32 ? launch_segment<float>(ctx, c, pl, a) : launch_segment<double>(ctx, c, pl, a));
    } else {
        std::vector<QuantileChunk> chunks;
        std::vector<QuantileGroup> groups;
        quantile_series_tables(offsets64.data(), c.G, pl.K, &chunks, &groups, C);
        sd_scratch dchunks, dgroups, runs, counts;
        SD_TRY(upload(ctx, dchunks, chunks));
        SD_TRY(upload(ctx, dgroups, groups));
        SD_HIP(runs.alloc(ctx, sizeof(double) * (size_t)pl.run_slots * (size_t)C));
        SD_HIP(counts.alloc(ctx, sizeof(int32_t) * (size_t)pl.chunks * (size_t)C));
        const int rc = c.src_is_f32 ? launch_series<float>(ctx, c, pl, a, dchunks.as<QuantileChunk>(), dgroups.as<QuantileGroup>(), runs.as<double>(),
                                                           counts.as<int32_t>())
                                    : launch_series<double>(ctx, c, pl, a, dchunks.as<QuantileChunk>(), dgroups.as<QuantileGroup>(), runs.as<double>(),
                                                            counts.as<int32_t>());
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool)
        SD_TRY(rc);
    }
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_quantile(sd_ctx* ctx, int method, int skipna, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group, int64_t G,
                const double* q, int64_t Q, double* out_host) {
    SD_CHECK_ARG(ctx && src_host && out_host && (q || method == SD_QUANTILE_MEDIAN), "sd_quantile: NULL argument");
    const QuantileCall c = quantile_call(ctx, method, skipna, src_is_f32, C, T, C, group != nullptr, G, q, Q, C, nullptr);  // (before the upload)
    const QuantilePlan pl = quantile_groups(quantile_check(c), group, T, c.G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_out(out_host, sizeof(double) * (size_t)pl.Q * c.G * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_quantile_dev(ctx, method, skipna, d[0], src_is_f32, C, T, C, group, G, q, Q, (double*)d[1], C);
    });
}

}  // extern "C"
