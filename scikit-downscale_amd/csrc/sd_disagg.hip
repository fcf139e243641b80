// Temporal disaggregation of a monthly [M, C] field into a daily [Tout, C] field (GridArray.disaggregate; the last step of BCSD, Wood
// et al. 2004): output row t of bin m borrows row src_row[t] of the daily observations, and the borrowed month is shifted
// (SD_DISAGG_SHIFT) or scaled (SD_DISAGG_SCALE_MEAN / _SUM) so that its monthly statistic equals target[m].  Every cell borrows the
// same rows, so the row map is wave-uniform.  pandas makes the tables on the host (skdownscale_amd/disagg.py: time_map); the launch
// plan and the refusals are in sd_disagg_plan.h.
//
// disagg_kernel<S, V, OP>: the geometry, the batched loads and the statistic of a bin are those of sd_bins.h.  src_row and offsets
// are indexed by wave-uniform values only, so they are read through scalar loads.
//   pass 1: the statistic of the borrowed rows in time order (bin_statistic, as in resample_kernel).
//   pass 2: the same rows again (the 64 * V * sizeof(S) bytes a wave has just read of each; which level of the memory hierarchy serves
//           them is discussed with the measurement in DESIGN.md 4.13), one add or one multiply per sample, one coalesced store of V
//           doubles per lane and row (16 bytes per access where the plan allows).
// A row past the end of the bin reads the bin's last row again and is neither counted nor stored; an empty bin runs no batch.  Every
// operation is a single add, subtract, multiply or divide (-ffp-contract=off): the result is that of tests/_disagg_oracle.py bit
// for bit, whatever the launch geometry and however a caller cuts the output into blocks of whole bins.  No LDS, no atomics.
// Algorithmic bytes: sizeof(S) * Tout * C read + 8 * M * C read + 8 * Tout * C written.
//
// shift:      out = x + (tgt - acc / cnt)
// scale_mean: out = x * (tgt / (acc / cnt)); a dry month (mean == 0) gives tgt on every non-NaN day
// scale_sum:  out = x * (tgt / acc);         a dry month (acc == 0) gives tgt / cnt on every non-NaN day
// with a climatology tgt = climo[group[m]] + target[m] (shift) or climo[group[m]] * target[m] (scale).  A NaN sample stays NaN, a bin
// without a sample and a bin with a NaN target are NaN, inf follows IEEE arithmetic.
#include <vector>

#include "sd_bins.h"
#include "sd_disagg_plan.h"
#include "sd_internal.h"
#include "sd_state.h"

namespace {
using namespace sdbn;

template <typename S, int V, int OP>
__global__ void __launch_bounds__(kLanes* kWaves)
    disagg_kernel(const double* __restrict__ target, int64_t ld_t, const S* __restrict__ obs, int64_t ld_obs, int64_t C,
                  const int64_t* __restrict__ src_row, const int64_t* __restrict__ offsets, int64_t M, int64_t ctiles,
                  const double* __restrict__ climo, int64_t ld_c, const int32_t* __restrict__ group, double* __restrict__ out, int64_t ld_out) {
    int64_t c0, m0;
    if (!lane_place<V>(ctiles, C, c0, m0)) return;
    const S* const col = obs + c0;
    const auto borrowed = [&](int64_t r) { return src_row[r]; };
    for (int b = 0; b < kBinsPerWave; ++b) {
        const int64_t m = m0 + b;
        if (m >= M) break;  // wave-uniform
        const int64_t r0 = offsets[m], r1 = offsets[m + 1];
        if (r0 >= r1) continue;  // an empty bin has no row to write
        double tgt[V];
        load_doubles<V>(target + m * ld_t + c0, tgt);
        if (climo != nullptr) {  // the target is an anomaly
            double base[V];
            load_doubles<V>(climo + (int64_t)group[m] * ld_c + c0, base);
#pragma unroll
            for (int v = 0; v < V; ++v) tgt[v] = OP == SD_DISAGG_SHIFT ? base[v] + tgt[v] : base[v] * tgt[v];
        }
        // pass 1: the statistic of the borrowed month, in time order
        double acc[V];
        int cnt[V];
        bin_statistic<S, V>(col, ld_obs, r0, r1, borrowed, acc, cnt);
        // what pass 2 applies: an addend (shift), or a factor and what a dry month gets instead (scale)
        double by[V], fill[V];
        bool dry[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double n = (double)cnt[v];
            if constexpr (OP == SD_DISAGG_SHIFT) {
                by[v] = tgt[v] - acc[v] / n, fill[v] = 0.0, dry[v] = false;
            } else {
                const double s = OP == SD_DISAGG_SCALE_MEAN ? acc[v] / n : acc[v];
                dry[v] = s == 0.0;
                by[v] = tgt[v] / s;
                fill[v] = OP == SD_DISAGG_SCALE_MEAN ? tgt[v] : tgt[v] / n;
            }
        }
        // pass 2: the rows
        double* const o = out + c0;
        for (int64_t r = r0; r < r1; r += kBatch) {
            Cells<S, V> q[kBatch];
            load_batch(q, col, ld_obs, r, r1, borrowed);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (r + u >= r1) break;  // wave-uniform
                double res[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double x = (double)q[u].v[v];
                    if constexpr (OP == SD_DISAGG_SHIFT)
                        res[v] = x + by[v];
                    else
                        res[v] = dry[v] ? (x == x ? fill[v] : x) : x * by[v];
                }
                store_doubles<V>(o + (r + u) * ld_out, res);
            }
        }
    }
}

struct DisaggTables {
    const int64_t *src_row, *offsets;
    const int32_t* group;
};

int launch(sd_ctx* ctx, const DisaggCall& c, const DisaggPlan& pl, const double* target, const void* obs, const DisaggTables& t,
           const double* climo, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    return with_cells(c.obs_is_f32, pl.cols, obs, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
#define SD_DISAGG_LAUNCH(OP)                                                                                                            \
    SD_LAUNCH(ctx, "disagg_kernel", (disagg_kernel<S, V, OP>), grid, block, 0, target, c.ld_t, s, c.ld_obs, c.C, t.src_row, t.offsets, c.M, \
              pl.ctiles, climo, c.ld_c, t.group, out, c.ld_out)
        if (c.op == SD_DISAGG_SHIFT)
            SD_DISAGG_LAUNCH(SD_DISAGG_SHIFT);
        else if (c.op == SD_DISAGG_SCALE_MEAN)
            SD_DISAGG_LAUNCH(SD_DISAGG_SCALE_MEAN);
        else
            SD_DISAGG_LAUNCH(SD_DISAGG_SCALE_SUM);
#undef SD_DISAGG_LAUNCH
        return (int)SD_OK;
    });
}

struct Field {
    const void* p;  // for its alignment
    int64_t ld;
};

DisaggCall call_of(int op, int obs_is_f32, int64_t To, int64_t C, int64_t Tout, int64_t M, int64_t G, bool has_climo, bool has_group, Field target,
                   Field obs, Field out, Field climo) {
    const auto aligned16 = [](Field f) { return ((uintptr_t)f.p & 15) == 0; };
    DisaggCall c;
    c.op = op, c.obs_is_f32 = obs_is_f32 != 0;
    c.To = To, c.C = C, c.Tout = Tout, c.M = M;
    c.ld_t = target.ld, c.ld_obs = obs.ld, c.ld_out = out.ld, c.ld_c = climo.ld;
    c.has_climo = has_climo, c.has_group = has_group, c.G = G;
    c.target_aligned16 = aligned16(target), c.obs_aligned16 = aligned16(obs), c.out_aligned16 = aligned16(out);
    c.climo_aligned16 = aligned16(climo);
    return c;
}

}  // namespace

extern "C" {

int sd_disagg_dev(sd_ctx* ctx, int op, const double* target_dev, int64_t ld_t, const void* obs_dev, int obs_is_f32, int64_t ld_obs, int64_t To,
                  int64_t C, const int64_t* src_row, int64_t Tout, const int64_t* offsets, int64_t M, const double* climo_dev, int64_t ld_c,
                  int64_t G, const int32_t* group, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && target_dev && obs_dev && src_row && offsets && out_dev, "sd_disagg: NULL argument");
    const DisaggCall c = call_of(op, obs_is_f32, To, C, Tout, M, G, climo_dev != nullptr, group != nullptr, {target_dev, ld_t}, {obs_dev, ld_obs},
                                 {out_dev, ld_out}, {climo_dev, ld_c});
    const DisaggPlan pl = disagg_check_tables(disagg_plan(c), c, src_row, offsets, group);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch rows, bins, groups;
    SD_TRY(upload(ctx, rows, std::vector<int64_t>(src_row, src_row + Tout)));
    SD_TRY(upload(ctx, bins, std::vector<int64_t>(offsets, offsets + M + 1)));
    if (group) SD_TRY(upload(ctx, groups, std::vector<int32_t>(group, group + M)));
    const DisaggTables t = {rows.as<int64_t>(), bins.as<int64_t>(), group ? groups.as<int32_t>() : nullptr};
    SD_TRY(launch(ctx, c, pl, target_dev, obs_dev, t, climo_dev, out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_disagg(sd_ctx* ctx, int op, const double* target_host, const void* obs_host, int obs_is_f32, int64_t To, int64_t C, const int64_t* src_row,
              int64_t Tout, const int64_t* offsets, int64_t M, const double* climo_host, int64_t G, const int32_t* group, double* out_host) {
    SD_CHECK_ARG(ctx && target_host && obs_host && src_row && offsets && out_host, "sd_disagg: NULL argument");
    const Field tight = {nullptr, C};  // (before the upload: tight rows, aligned scratch)
    const DisaggCall c = call_of(op, obs_is_f32, To, C, Tout, M, G, climo_host != nullptr, group != nullptr, tight, tight, tight, tight);
    const DisaggPlan pl = disagg_check_tables(disagg_plan(c), c, src_row, offsets, group);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t cells = (size_t)C, obs_bytes = (obs_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)To * cells;
    const sd_host_field f[] = {sd_in(target_host, sizeof(double) * (size_t)M * cells), sd_in(obs_host, obs_bytes),
                               sd_in(climo_host, climo_host ? sizeof(double) * (size_t)G * cells : 0),
                               sd_out(out_host, sizeof(double) * (size_t)Tout * cells)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_disagg_dev(ctx, op, (const double*)d[0], C, d[1], obs_is_f32, C, To, C, src_row, Tout, offsets, M, (const double*)d[2], C, G, group,
                             (double*)d[3], C);
    });
}

}  // extern "C"
