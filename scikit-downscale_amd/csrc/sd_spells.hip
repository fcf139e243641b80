// Threshold and spell indices per period of a [T, C] field (GridArray.where(op, threshold).resample(time=rule).count() / .fraction() /
// .longest_spell() / .spell_days(L) / .spell_count(L): frost days, R1mm, CDD / CWD, WSDI, TX90p): bin m is the run of rows offsets[m] ..
// offsets[m + 1] - 1, made by pandas on the host; the threshold is a scalar or row group[r] of a [G, C] table (a per-cell threshold is
// the table with G = 1 and no group array).  The rule is stated in include/sd_downscale.h; the launch plan and the refusals are in
// sd_spells_plan.h.
//
// spells_kernel<S, V, TABLE>: the geometry and the batched loads are those of sd_bins.h (lane_place, load_batch): a lane owns V adjacent
// cells for a whole bin, a wave takes kBinsPerWave whole bins, the loads of a batch of kBatch rows -- the source row and, with TABLE, its
// row of the table, whose group id is wave-uniform and read through a scalar load -- are issued before their arithmetic.  The per-step
// body is the run-length state (valid, hits, run, longest, days, spells) of the cell, all int32 in registers.  load_batch reads the
// bin's last row again for rows past its end: such a row is no hit (`inside` gates the hit itself, so it ends the run and adds
// nothing; the bin is over anyway).  '<' and '<=' are '>' and '>=' of the exactly negated operands (a flip of the sign bit: NaN stays
// NaN, +-inf and +-0 keep their order), so the comparison is the two wave-uniform flags (flip, strict) and not a template parameter.
// A bin ends with nstat stores of V doubles per lane, selected by wave-uniform codes: several indices of one threshold cost one pass
// over the field.  No LDS, no atomics.  Algorithmic bytes: sizeof(S) * T * C read (+ 8 * T * C of table rows with a group array, 8 * C
// without) + 8 * nstat * M * C written.
//
// A bin is never split across lanes: one very long bin over few cells has little parallelism.  That is the price of the sequential
// state.  (Run summaries with their prefix and suffix runs form a monoid, so segments of a long bin could be merged; that is not done
// here.)
#include <vector>

#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_spells_plan.h"
#include "sd_state.h"

namespace {
using namespace sdbn;
using sdsp::kMaxStats;

// x with its sign bit flipped where sign is 0x80000000 (exact negation: NaN stays NaN), x itself where it is 0
__device__ __forceinline__ double flip_sign(double x, int sign) { return __hiloint2double(__double2hiint(x) ^ sign, __double2loint(x)); }

template <typename S, int V, bool TABLE>
__global__ void __launch_bounds__(kLanes* kWaves)
    spells_kernel(const S* __restrict__ src, int64_t ld, int64_t C, const int64_t* __restrict__ offsets, int64_t M, int64_t ctiles, double thr,
                  const double* __restrict__ table, int64_t ld_t, const int32_t* __restrict__ group, int flip, int strict, int L, int stats,
                  int nstat, double* __restrict__ out, int64_t ld_out, int64_t stride_out) {
    int64_t c0, m0;
    if (!lane_place<V>(ctiles, C, c0, m0)) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int sign = flip ? (int)0x80000000u : 0, loose = strict ? 0 : 1;  // wave-uniform
    const S* const col = src + c0;
    double tc[V];  // the threshold of the lane's cells where it is the same for every row: the scalar, or row 0 of a table without groups
    if constexpr (TABLE) {
        if (group == nullptr) load_doubles<V>(table + c0, tc);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) tc[v] = thr;
    }
    for (int b = 0; b < kBinsPerWave; ++b) {
        const int64_t m = m0 + b;
        if (m >= M) break;  // wave-uniform
        const int64_t r0 = offsets[m], r1 = offsets[m + 1];
        int valid[V], hits[V], run[V], longest[V], days[V], spells[V];
#pragma unroll
        for (int v = 0; v < V; ++v) valid[v] = hits[v] = run[v] = longest[v] = days[v] = spells[v] = 0;
        for (int64_t r = r0; r < r1; r += kBatch) {
            Cells<S, V> q[kBatch];
            double t[kBatch][V];
            load_batch(q, col, ld, r, r1, [](int64_t i) { return i; });
            if (TABLE && group != nullptr) {  // wave-uniform
#pragma unroll
                for (int u = 0; u < kBatch; ++u) load_doubles<V>(table + c0 + (int64_t)group[min(r + u, r1 - 1)] * ld_t, t[u]);
            } else {
#pragma unroll
                for (int u = 0; u < kBatch; ++u)
#pragma unroll
                    for (int v = 0; v < V; ++v) t[u][v] = tc[v];
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int inside = r + u < r1;  // wave-uniform: a row past the bin's end is the clamped last row, not a step
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    // (plain integer arithmetic on the comparisons: no short-circuit, nothing for the compiler to branch on)
                    const double x = (double)q[u].v[v], th = t[u][v];
                    const double xs = flip_sign(x, sign), ts = flip_sign(th, sign);
                    const int ok = inside & (int)(x == x) & (int)(th == th);
                    const int hit = inside & ((int)(xs > ts) | ((int)(xs == ts) & loose));  // false with a NaN on either side
                    valid[v] += ok;
                    hits[v] += hit;
                    run[v] = (run[v] + 1) & -hit;
                    longest[v] = max(longest[v], run[v]);
                    const int at = run[v] == L, past = run[v] > L;
                    days[v] += (L & -at) + past;
                    spells[v] += at;
                }
            }
        }
        double* const o = out + m * ld_out + c0;
#pragma unroll
        for (int s = 0; s < kMaxStats; ++s) {
            if (s >= nstat) break;  // wave-uniform
            const int code = (stats >> (4 * s)) & 15;  // wave-uniform, as are the masks: all ones for the statistic asked for
            const int mv = -(int)(code == SD_SPELL_VALID), mh = -(int)(code == SD_SPELL_COUNT), ml = -(int)(code == SD_SPELL_LONGEST_SPELL),
                      md = -(int)(code == SD_SPELL_SPELL_DAYS), ms = -(int)(code == SD_SPELL_SPELL_COUNT);
            double res[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int n = (valid[v] & mv) | (hits[v] & mh) | (longest[v] & ml) | (days[v] & md) | (spells[v] & ms);
                res[v] = code == SD_SPELL_FRACTION ? (valid[v] > 0 ? (double)hits[v] / (double)valid[v] : nan) : (double)n;
            }
            store_doubles<V>(o + s * stride_out, res);
        }
    }
}

int launch(sd_ctx* ctx, const SpellsCall& c, const SpellsPlan& pl, const void* src, double thr, const double* table, const int32_t* group,
           const int64_t* offsets, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    const int flip = c.op == SD_SPELL_LT || c.op == SD_SPELL_LE, strict = c.op == SD_SPELL_GT || c.op == SD_SPELL_LT;
    // a run is at most T < 2^31 steps long: a longer minimum is never reached (min_length above INT32_MAX counts as INT32_MAX)
    const int L = (int)std::min<int64_t>(c.min_length, INT32_MAX);
    int stats = 0;  // the codes, four bits each
    for (int s = 0; s < c.nstat; ++s) stats |= c.stats[s] << (4 * s);
    return with_cells(c.src_is_f32, pl.cols, src, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
        if (c.has_table)
            SD_LAUNCH(ctx, "spells_kernel", (spells_kernel<S, V, true>), grid, block, 0, s, c.ld, c.C, offsets, c.M, pl.ctiles, thr, table, c.ld_t, group,
                      flip, strict, L, stats, c.nstat, out, c.ld_out, c.stride_out);
        else
            SD_LAUNCH(ctx, "spells_kernel", (spells_kernel<S, V, false>), grid, block, 0, s, c.ld, c.C, offsets, c.M, pl.ctiles, thr, table, c.ld_t,
                      group, flip, strict, L, stats, c.nstat, out, c.ld_out, c.stride_out);
        return (int)SD_OK;
    });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

SpellsCall call_of(int src_is_f32, int64_t ld, int64_t T, int64_t C, int op, bool has_table, int64_t ld_t, bool has_group, int64_t G, int64_t M,
                   int64_t min_length, const int* stats, int nstat, int64_t ld_out, int64_t stride_out, const void* src, const void* table,
                   const void* out) {
    SpellsCall c;
    c.op = op, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.M = M, c.min_length = min_length;
    c.has_table = has_table, c.ld_t = ld_t, c.G = has_table ? G : 1, c.has_group = has_table && has_group;
    c.nstat = nstat;
    for (int s = 0; s < nstat && s < kMaxStats; ++s) c.stats[s] = stats[s];
    c.ld_out = ld_out, c.stride_out = stride_out;
    c.src_aligned16 = aligned16(src), c.table_aligned16 = aligned16(table), c.out_aligned16 = aligned16(out);
    return c;
}

}  // namespace

extern "C" {

int sd_spells_dev(sd_ctx* ctx, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, int op, double threshold,
                  const double* table_dev, int64_t ld_t, const int32_t* group, int64_t G, const int64_t* offsets, int64_t M, int64_t min_length,
                  const int* stats, int nstat, double* out_dev, int64_t ld_out, int64_t stride_out) {
    SD_CHECK_ARG(ctx && src_dev && offsets && stats && out_dev, "sd_spells: NULL argument");
    const SpellsCall c = call_of(src_is_f32, ld, T, C, op, table_dev != nullptr, ld_t, group != nullptr, G, M, min_length, stats, nstat, ld_out,
                                 stride_out, src_dev, table_dev, out_dev);
    const SpellsPlan pl = spells_plan(c, group, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch bins, groups;
    SD_TRY(upload(ctx, bins, std::vector<int64_t>(offsets, offsets + M + 1)));
    if (c.has_group) SD_TRY(upload(ctx, groups, std::vector<int32_t>(group, group + T)));
    SD_TRY(launch(ctx, c, pl, src_dev, threshold, table_dev, c.has_group ? groups.as<int32_t>() : nullptr, bins.as<int64_t>(), out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_spells(sd_ctx* ctx, const void* src_host, int src_is_f32, int64_t T, int64_t C, int op, double threshold, const double* table_host,
              const int32_t* group, int64_t G, const int64_t* offsets, int64_t M, int64_t min_length, const int* stats, int nstat,
              double* out_host) {
    SD_CHECK_ARG(ctx && src_host && offsets && stats && out_host, "sd_spells: NULL argument");
    const int64_t stride = M > 0 && C > 0 && M <= INT64_MAX / 8 / C ? M * C : 0;
    const SpellsCall c = call_of(src_is_f32, C, T, C, op, table_host != nullptr, C, group != nullptr, G, M, min_length, stats, nstat, C, stride,
                                 nullptr, nullptr, nullptr);  // (before the upload)
    const SpellsPlan pl = spells_plan(c, group, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_in(table_host, table_host ? sizeof(double) * (size_t)c.G * C : 0),
                               sd_out(out_host, sizeof(double) * (size_t)nstat * M * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_spells_dev(ctx, d[0], src_is_f32, C, T, C, op, threshold, (const double*)d[1], C, group, G, offsets, M, min_length, stats, nstat,
                             (double*)d[2], C, stride);
    });
}

}  // extern "C"
