// Distribution scores of two [T, C] fields per cell and bin of consecutive rows (GridArray.compare(other).ks() / .perkins(width) /
// .distribution(names)): the two-sample Kolmogorov-Smirnov distance and the Perkins skill score.  The rule is stated in
// include/sd_downscale.h; the launch plan and the refusals are in sd_twosample_plan.h.  A two-sample score is the sorts of sd_quantile.hip
// done twice (sd_order.h: gather_tile, sort_row, quantile_runs_kernel) with another last step: one rank search per sample of a in the
// sorted samples of b in place of a quantile evaluation.
//
// twosample_segment_kernel<SA, SB, K>: one 512-thread workgroup = 8 adjacent cells x one bin of at most 64 * K rows.  The bin's rows of
// both fields are gathered into two LDS rows per cell; the wave that owns the cell sorts both (NaN become the +inf pads and are
// counted: the first na / nb slots are the valid samples).  KS: lane l takes a[l + 64 * i] (consecutive doubles: conflict-free) and
// finds lt by a binary search in b's row and le from there; the wave reduces the integer maximum.  Perkins, after that: both rows are
// overwritten by their bin numbers k(x) (one division per sample; k is monotone, the rows stay sorted), then a lane whose sample is the
// first of its histogram bin in a counts ca_k and cb_k by searches on k and adds min(ca_k * nb, cb_k * na); the wave's integer sum does
// not depend on the order.  Lane 0 stores the nstat values.  An empty bin stores its values before any load.
//
// Series path (bins longer than the widest segment, up to 19 456 rows): quantile_runs_kernel<S, K> once per field, then
// twosample_select_kernel<K>, one 1 024-thread workgroup per (bin, cell) in a grid-stride loop: merge a's runs in LDS, write the sorted
// a back over its own scratch slots, barrier, merge b's runs in LDS, then every thread streams a_i from scratch (coalesced, written a
// moment ago by this workgroup) and searches b in LDS; the integer maximum and sum are reduced over the workgroup and one thread
// stores.  The two sorted series are never in LDS together.  For Perkins both series are overwritten by their bin numbers where they
// are (a in its scratch slots, b in LDS); the count ca_k of a bin's first sample is a search in a's scratch slots: one chain of global
// loads per occupied histogram bin, not per sample.
//
// Groups (sd_twosample_groups: compare(other).groupby("time.season").ks()): the same kernels under the same profiler names.  Every kernel
// reads its rows through the row table only -- gather_tile(rows + beg) in the segment kernel, rows + ch.start in quantile_runs_kernel;
// twosample_select_kernel sees runs and counts, no rows -- so the group-sorted table of groupby_tables takes the place of the identity
// and the offsets over it the place of the bins; the plan (twosample_groups_plan) chooses the path by the longest group.
//
// Algorithmic bytes: sizeof(SA) * T * C + sizeof(SB) * T * C read, 8 * nstat * M * C written; the series path adds a write and two
// reads of 8 * C * run_slots bytes of scratch per field (three reads of a's).  Everything after the sorts is integer arithmetic and
// one division: the bits depend neither on the layout, nor on the path, nor on the launch geometry.
#include <vector>

#include "sd_internal.h"
#include "sd_order.h"
#include "sd_state.h"
#include "sd_twosample_plan.h"

namespace {
using sdts::kMaxStats;

// samples of v[0 .. n) (ascending) below x
__device__ __forceinline__ int count_lt(const double* v, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool below = v[mid] < x;
        lo = below ? mid + 1 : lo;
        hi = below ? hi : mid;
    }
    return lo;
}
// ... not above x, from: a position known to be at or before the answer (count_lt's: for untied data the first probe ends the search)
__device__ __forceinline__ int count_le(const double* v, int from, int n, double x) {
    if (from >= n || v[from] > x) return from;
    int lo = from + 1, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool below = v[mid] <= x;
        lo = below ? mid + 1 : lo;
        hi = below ? hi : mid;
    }
    return lo;
}
// the histogram bin of a sample (sd_downscale.h): monotone in x, so a sorted row of samples becomes a sorted row of bin numbers
__device__ __forceinline__ double hist_bin(double x, double width, double origin) { return floor((x - origin) / width); }

struct Wants {
    bool ks, perkins;
};
__device__ __forceinline__ Wants wants_of(int stats, int nstat) {
    Wants w = {false, false};
    for (int s = 0; s < nstat; ++s) {
        const int code = (stats >> (4 * s)) & 15;
        w.ks |= code == SD_TWOSAMPLE_KS;
        w.perkins |= code == SD_TWOSAMPLE_PERKINS;
    }
    return w;
}

// the KS term of sample i of a (sorted, na of them) against b (sorted, nb of them)
__device__ __forceinline__ void ks_term(const double* sa, const double* sb, int i, int na, int nb, long long& kmax) {
    const double x = sa[i];
    const int below = count_lt(sb, nb, x);
    const long long lt = below, le = count_le(sb, below, nb, x);
    const long long up = (long long)(i + 1) * nb - le * na, down = lt * na - (long long)i * nb;
    const long long t = up > down ? up : down;
    kmax = t > kmax ? t : kmax;
}
// the Perkins term of sample i of a; ka, kb: the rows as bin numbers (hist_bin of the sorted samples, written over them: one division
// per sample, none per probe)
__device__ __forceinline__ void perkins_term(const double* ka, const double* kb, int i, int na, int nb, long long& psum) {
    const double k = ka[i];
    if (i == 0 || ka[i - 1] != k) {  // the first sample of its bin in a
        const long long ca = count_le(ka, i + 1, na, k) - i;
        const int b0 = count_lt(kb, nb, k);
        const long long cb = count_le(kb, b0, nb, k) - b0;
        const long long ta = ca * nb, tb = cb * na;
        psum += ta < tb ? ta : tb;
    }
}

__device__ __forceinline__ long long wave_max_i64(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long u = __shfl_xor(v, o, kWave);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the nstat values of one (bin, cell), by one thread
__device__ __forceinline__ void store_stats(double* o, int64_t stride_out, int stats, int nstat, int na, int nb, long long kmax, long long psum) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double denom = (double)na * (double)nb;
    const bool none = na == 0 || nb == 0;
#pragma unroll 1
    for (int s = 0; s < nstat; ++s) {
        const int code = (stats >> (4 * s)) & 15;
        double r;
        switch (code) {
            case SD_TWOSAMPLE_KS: r = none ? nan : (double)kmax / denom; break;
            case SD_TWOSAMPLE_PERKINS: r = none ? nan : (double)psum / denom; break;
            case SD_TWOSAMPLE_NA: r = (double)na; break;
            default: r = (double)nb; break;  // SD_TWOSAMPLE_NB
        }
        o[s * stride_out] = r;
    }
}

template <typename SA, typename SB, int K>
__global__ void __launch_bounds__(kThreads)
    twosample_segment_kernel(const SA* __restrict__ a, int64_t ld_a, const SB* __restrict__ b, int64_t ld_b, int64_t C, const int32_t* __restrict__ rows,
                             const int32_t* __restrict__ offsets, int64_t M, int64_t ntiles, int vec_a, int vec_b, int stats, int nstat, double width,
                             double origin, double* __restrict__ out, int64_t ld_out, int64_t stride_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = tile_sort_rs(K);
    double* const tile_a = reinterpret_cast<double*>(smem_raw) + kHeadDoubles;  // (no row at LDS address 0: sd_wave_consts.h)
    double* const tile_b = tile_a + kW * RS;
    const int64_t tile_id = sdqt::tile_of_block(blockIdx.x, ntiles), m = sdqt::item_of_block(blockIdx.x, ntiles);
    if (tile_id >= ntiles || m >= M) return;
    const int64_t c0 = tile_id * kW;
    const int beg = offsets[m], n = offsets[m + 1] - beg;  // workgroup-uniform
    const int tid = tid_now();
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave;
    double* const row_a = tile_a + wave * RS;
    double* const row_b = tile_b + wave * RS;
    int na = 0, nb = 0;
    if (n > 0) {
        gather_tile<SA, K>(a, ld_a, rows + beg, n, c0, C, vec_a != 0, tile_a);
        gather_tile<SB, K>(b, ld_b, rows + beg, n, c0, C, vec_b != 0, tile_b);
        __syncthreads();
        na = sort_row<K>(row_a, n, n, lane);
        nb = sort_row<K>(row_b, n, n, lane);
    }
    const int64_t c = c0 + wave;
    if (c >= C) return;
    long long kmax = 0, psum = 0;  // (the last sample of a alone gives (na * nb - le * na) >= 0: the maximum is never negative)
    if (na > 0 && nb > 0) {        // wave-uniform
        const Wants w = wants_of(stats, nstat);
        if (w.ks)
            for (int i = lane; i < na; i += kWave) ks_term(row_a, row_b, i, na, nb, kmax);
        if (w.perkins) {
            wave_fence();  // the samples have been read
            for (int i = lane; i < na; i += kWave) row_a[i] = hist_bin(row_a[i], width, origin);
            for (int i = lane; i < nb; i += kWave) row_b[i] = hist_bin(row_b[i], width, origin);
            wave_fence();
            for (int i = lane; i < na; i += kWave) perkins_term(row_a, row_b, i, na, nb, psum);
        }
        kmax = wave_max_i64(kmax);
        psum = wave_sum_i64(psum);
    }
    if (lane == 0) store_stats(out + m * ld_out + c, stride_out, stats, nstat, na, nb, kmax, psum);
}

template <int K>
__global__ void __launch_bounds__(sdqt::kSelectThreads)
    twosample_select_kernel(double* runs_a, const double* __restrict__ runs_b, const int32_t* __restrict__ counts_a,
                            const int32_t* __restrict__ counts_b, const QuantileGroup* __restrict__ groups, int64_t M, int64_t C, int stats, int nstat,
                            double width, double origin, double* __restrict__ out, int64_t ld_out, int64_t stride_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* const buf = reinterpret_cast<double*>(smem_raw);  // np + 1 keys, then nthr + 1 co-ranks (the partial results after the merges)
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const Wants w = wants_of(stats, nstat);
    for (int64_t item = blockIdx.x; item < M * C; item += gridDim.x) {
        const int64_t m = item / C, c = item % C;
        const QuantileGroup gr = groups[m];  // workgroup-uniform
        const int np = gr.np;
        int na = 0, nb = 0;
        long long kmax = 0, psum = 0;
        __syncthreads();  // the keys and the partial results of the last item have been read
        if (np > 0) {
            double* const ra = runs_a + gr.base + c * (int64_t)np;
            const double* const rb = runs_b + gr.base + c * (int64_t)np;
            long long* const part = reinterpret_cast<long long*>(buf + np + 1);  // 2 per wave, over the co-ranks
            for (int j = 0; j < gr.nchunks; ++j) {
                na += counts_a[(int64_t)(gr.chunk0 + j) * C + c];
                nb += counts_b[(int64_t)(gr.chunk0 + j) * C + c];
            }
            for (int i = tid; i <= np; i += nthr) buf[i] = i < np ? ra[i] : inf;
            __syncthreads();
            sdsort::block_merge_rounds<K>(buf, np, reinterpret_cast<int*>(buf + np + 1), tid, nthr, 6);
            for (int i = tid; i < np; i += nthr) ra[i] = buf[i];
            __syncthreads();  // the sorted a is visible to the workgroup, and its keys in LDS have been read
            for (int i = tid; i <= np; i += nthr) buf[i] = i < np ? rb[i] : inf;
            __syncthreads();
            sdsort::block_merge_rounds<K>(buf, np, reinterpret_cast<int*>(buf + np + 1), tid, nthr, 6);
            if (na > 0 && nb > 0) {  // workgroup-uniform
                if (w.ks)
                    for (int i = tid; i < na; i += nthr) ks_term(ra, buf, i, na, nb, kmax);
                if (w.perkins) {
                    __syncthreads();  // the samples have been read
                    for (int i = tid; i < na; i += nthr) ra[i] = hist_bin(ra[i], width, origin);
                    for (int i = tid; i < nb; i += nthr) buf[i] = hist_bin(buf[i], width, origin);
                    __syncthreads();
                    for (int i = tid; i < na; i += nthr) perkins_term(ra, buf, i, na, nb, psum);
                }
            }
            kmax = wave_max_i64(kmax);
            psum = wave_sum_i64(psum);
            if (tid % kWave == 0) part[2 * (tid / kWave)] = kmax, part[2 * (tid / kWave) + 1] = psum;
            __syncthreads();
            if (tid == 0) {
                kmax = 0, psum = 0;
                for (int v = 0; v < nthr / kWave; ++v) {
                    kmax = part[2 * v] > kmax ? part[2 * v] : kmax;
                    psum += part[2 * v + 1];
                }
            }
        }
        if (tid == 0) store_stats(out + m * ld_out + c, stride_out, stats, nstat, na, nb, kmax, psum);
    }
}

// profiler names: the width is part of the name, so that a profile (and a test) tells which instantiation served a call
template <int K>
constexpr const char* segment_name() {
    static_assert(K == 5 || K == 7 || K == 13 || K == 19, "name the new width");
    return K == 5 ? "twosample_segment_kernel<5>" : K == 7 ? "twosample_segment_kernel<7>" : K == 13 ? "twosample_segment_kernel<13>" : "twosample_segment_kernel<19>";
}
template <int K>
constexpr const char* select_name() {
    return K == 13 ? "twosample_select_kernel<13>" : K == 17 ? "twosample_select_kernel<17>" : "twosample_select_kernel<19>";
}

struct TwosampleArgs {
    const void *a, *b;
    const int32_t* rows;     // device [T]: the row table of gather_tile (the identity for bins, the group-sorted rows for groups)
    const int32_t* offsets;  // device [M + 1]
    int stats;               // the codes, four bits each
    double* out;
};

template <typename SA, typename SB>
int launch_segment(sd_ctx* ctx, const TwosampleCall& c, const TwosamplePlan& pl, const TwosampleArgs& g) {
    return dispatch_width<sdts::kSegWidths>(
        pl.K,
        [&](auto k) -> int {
            SD_TRY(allow_lds(&twosample_segment_kernel<SA, SB, k>, pl.lds));
            SD_LAUNCH(ctx, segment_name<k>(), (twosample_segment_kernel<SA, SB, k>), dim3((unsigned)pl.blocks), dim3(kThreads), pl.lds, (const SA*)g.a,
                      c.ld_a, (const SB*)g.b, c.ld_b, c.C, g.rows, g.offsets, c.M, pl.ntiles, (int)pl.vec_a, (int)pl.vec_b, g.stats, c.nstat, c.width,
                      c.origin, g.out, c.ld_out, c.stride_out);
            return SD_OK;
        },
        "sd_twosample");
}

// the runs of one field
template <typename S>
int launch_runs(sd_ctx* ctx, const TwosamplePlan& pl, const void* src, int64_t ld, bool vec, int64_t C, const int32_t* rows, const QuantileChunk* chunks,
                double* runs, int32_t* counts) {
    return dispatch_width<sdqt::kSeriesWidths>(
        pl.K,
        [&](auto k) -> int {
            SD_TRY(allow_lds(&quantile_runs_kernel<S, k>, pl.lds));
            SD_LAUNCH(ctx, runs_name<k>(), (quantile_runs_kernel<S, k>), dim3((unsigned)pl.blocks), dim3(kThreads), pl.lds, (const S*)src, ld, C, rows,
                      chunks, pl.chunks, pl.ntiles, (int)vec, runs, counts);
            return SD_OK;
        },
        "sd_twosample");
}

int launch_select(sd_ctx* ctx, const TwosampleCall& c, const TwosamplePlan& pl, const TwosampleArgs& g, const QuantileGroup* groups, double* runs_a,
                  const double* runs_b, const int32_t* counts_a, const int32_t* counts_b) {
    return dispatch_width<sdqt::kSeriesWidths>(
        pl.K,
        [&](auto k) -> int {
            SD_TRY(allow_lds(&twosample_select_kernel<k>, pl.select_lds));
            SD_LAUNCH(ctx, select_name<k>(), (twosample_select_kernel<k>), dim3((unsigned)pl.select_blocks), dim3(sdqt::kSelectThreads), pl.select_lds,
                      runs_a, runs_b, counts_a, counts_b, groups, c.M, c.C, g.stats, c.nstat, c.width, c.origin, g.out, c.ld_out, c.stride_out);
            return SD_OK;
        },
        "sd_twosample");
}

int launch_series(sd_ctx* ctx, const TwosampleCall& c, const TwosamplePlan& pl, const TwosampleArgs& g, const QuantileChunk* chunks,
                  const QuantileGroup* groups, double* runs_a, double* runs_b, int32_t* counts_a, int32_t* counts_b) {
    SD_TRY(c.a_is_f32 ? launch_runs<float>(ctx, pl, g.a, c.ld_a, pl.vec_a, c.C, g.rows, chunks, runs_a, counts_a)
                      : launch_runs<double>(ctx, pl, g.a, c.ld_a, pl.vec_a, c.C, g.rows, chunks, runs_a, counts_a));
    SD_TRY(c.b_is_f32 ? launch_runs<float>(ctx, pl, g.b, c.ld_b, pl.vec_b, c.C, g.rows, chunks, runs_b, counts_b)
                      : launch_runs<double>(ctx, pl, g.b, c.ld_b, pl.vec_b, c.C, g.rows, chunks, runs_b, counts_b));
    return launch_select(ctx, c, pl, g, groups, runs_a, runs_b, counts_a, counts_b);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

TwosampleCall call_of(const sd_ctx* ctx, int a_is_f32, int64_t ld_a, int b_is_f32, int64_t ld_b, int64_t T, int64_t C, int64_t M, const int* stats,
                      int nstat, double width, double origin, int64_t ld_out, int64_t stride_out, const void* a, const void* b) {
    TwosampleCall c;
    c.a_is_f32 = a_is_f32 != 0, c.b_is_f32 = b_is_f32 != 0;
    c.T = T, c.C = C, c.ld_a = ld_a, c.ld_b = ld_b, c.M = M;
    c.nstat = nstat;
    for (int s = 0; s < nstat && s < kMaxStats; ++s) c.stats[s] = stats[s];
    c.width = width, c.origin = origin;
    c.ld_out = ld_out, c.stride_out = stride_out;
    c.a_aligned16 = aligned16(a), c.b_aligned16 = aligned16(b);
    c.lds_max = ctx->lds_max, c.cu_count = ctx->cu_count;
    return c;
}

// a planned call over the bins offsets [M + 1] (host) of the row table rows [T] (host): the identity for bins of consecutive rows, the
// group-sorted rows of groupby_tables for groups.  Every kernel reads its rows through the table only.
int run_planned(sd_ctx* ctx, const TwosampleCall& c, const TwosamplePlan& pl, const std::vector<int32_t>& rows, const int64_t* offsets, const void* a,
                const void* b, double* out) {
    const std::vector<int32_t> offsets32(offsets, offsets + c.M + 1);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch drows, doffsets;
    SD_TRY(upload(ctx, drows, rows));
    SD_TRY(upload(ctx, doffsets, offsets32));
    TwosampleArgs g = {a, b, drows.as<int32_t>(), doffsets.as<int32_t>(), 0, out};
    for (int s = 0; s < c.nstat; ++s) g.stats |= c.stats[s] << (4 * s);
    if (pl.path == sdts::kSegment) {
        int rc;
        if (c.a_is_f32)
            rc = c.b_is_f32 ? launch_segment<float, float>(ctx, c, pl, g) : launch_segment<float, double>(ctx, c, pl, g);
        else
            rc = c.b_is_f32 ? launch_segment<double, float>(ctx, c, pl, g) : launch_segment<double, double>(ctx, c, pl, g);
        SD_TRY(rc);
    } else {
        std::vector<QuantileChunk> chunks;
        std::vector<QuantileGroup> groups;
        quantile_series_tables(offsets, c.M, pl.K, &chunks, &groups, c.C);
        sd_scratch dchunks, dgroups, runs_a, runs_b, counts_a, counts_b;
        SD_TRY(upload(ctx, dchunks, chunks));
        SD_TRY(upload(ctx, dgroups, groups));
        SD_HIP(runs_a.alloc(ctx, sizeof(double) * (size_t)pl.run_slots * (size_t)c.C));
        SD_HIP(runs_b.alloc(ctx, sizeof(double) * (size_t)pl.run_slots * (size_t)c.C));
        SD_HIP(counts_a.alloc(ctx, sizeof(int32_t) * (size_t)pl.chunks * (size_t)c.C));
        SD_HIP(counts_b.alloc(ctx, sizeof(int32_t) * (size_t)pl.chunks * (size_t)c.C));
        const int rc = launch_series(ctx, c, pl, g, dchunks.as<QuantileChunk>(), dgroups.as<QuantileGroup>(), runs_a.as<double>(), runs_b.as<double>(),
                                     counts_a.as<int32_t>(), counts_b.as<int32_t>());
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool)
        SD_TRY(rc);
    }
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

}  // namespace

extern "C" {

int sd_twosample_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T, int64_t C,
                     const int64_t* offsets, int64_t M, const int* stats, int nstat, double width, double origin, double* out_dev, int64_t ld_out,
                     int64_t stride_out) {
    SD_CHECK_ARG(ctx && a_dev && b_dev && offsets && stats && out_dev, "sd_twosample: NULL argument");
    const TwosampleCall c = call_of(ctx, a_is_f32, ld_a, b_is_f32, ld_b, T, C, M, stats, nstat, width, origin, ld_out, stride_out, a_dev, b_dev);
    const TwosamplePlan pl = twosample_plan(c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    std::vector<int32_t> rows((size_t)T);
    for (int64_t t = 0; t < T; ++t) rows[t] = (int32_t)t;
    return run_planned(ctx, c, pl, rows, offsets, a_dev, b_dev, out_dev);
}

int sd_twosample(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C, const int64_t* offsets,
                 int64_t M, const int* stats, int nstat, double width, double origin, double* out_host) {
    SD_CHECK_ARG(ctx && a_host && b_host && offsets && stats && out_host, "sd_twosample: NULL argument");
    const int64_t stride = M > 0 && C > 0 && M <= INT64_MAX / 8 / C ? M * C : 0;
    const TwosampleCall c = call_of(ctx, a_is_f32, C, b_is_f32, C, T, C, M, stats, nstat, width, origin, C, stride, nullptr, nullptr);  // (before the upload)
    const TwosamplePlan pl = twosample_plan(c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t a_bytes = (a_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const size_t b_bytes = (b_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(a_host, a_bytes), sd_in(b_host, b_bytes), sd_out(out_host, sizeof(double) * (size_t)nstat * M * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_twosample_dev(ctx, d[0], a_is_f32, C, d[1], b_is_f32, C, T, C, offsets, M, stats, nstat, width, origin, (double*)d[2], C, stride);
    });
}

int sd_twosample_groups_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T,
                            int64_t C, const int32_t* group, int64_t G, const int* stats, int nstat, double width, double origin, double* out_dev,
                            int64_t ld_out, int64_t stride_out) {
    SD_CHECK_ARG(ctx && a_dev && b_dev && group && stats && out_dev, "sd_twosample_groups: NULL argument");
    const TwosampleCall c = call_of(ctx, a_is_f32, ld_a, b_is_f32, ld_b, T, C, G, stats, nstat, width, origin, ld_out, stride_out, a_dev, b_dev);
    std::vector<int64_t> rows64, offsets;
    const TwosamplePlan pl = twosample_groups_plan(c, group, &rows64, &offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const std::vector<int32_t> rows(rows64.begin(), rows64.end());  // (T < 2^31)
    return run_planned(ctx, c, pl, rows, offsets.data(), a_dev, b_dev, out_dev);
}

int sd_twosample_groups(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C, const int32_t* group,
                        int64_t G, const int* stats, int nstat, double width, double origin, double* out_host) {
    SD_CHECK_ARG(ctx && a_host && b_host && group && stats && out_host, "sd_twosample_groups: NULL argument");
    const int64_t stride = G > 0 && C > 0 && G <= INT64_MAX / 8 / C ? G * C : 0;
    const TwosampleCall c = call_of(ctx, a_is_f32, C, b_is_f32, C, T, C, G, stats, nstat, width, origin, C, stride, nullptr, nullptr);  // (before the upload)
    std::vector<int64_t> rows64, offsets;
    const TwosamplePlan pl = twosample_groups_plan(c, group, &rows64, &offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t a_bytes = (a_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const size_t b_bytes = (b_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(a_host, a_bytes), sd_in(b_host, b_bytes), sd_out(out_host, sizeof(double) * (size_t)nstat * G * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_twosample_groups_dev(ctx, d[0], a_is_f32, C, d[1], b_is_f32, C, T, C, group, G, stats, nstat, width, origin, (double*)d[2], C, stride);
    });
}

}  // extern "C"
