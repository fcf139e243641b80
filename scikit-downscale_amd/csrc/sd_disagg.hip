// Temporal disaggregation of a monthly [M, C] field into a daily [Tout, C] field (GridArray.disaggregate; the last step of BCSD, Wood
// et al. 2004): output row t of bin m borrows row src_row[t] of the daily observations, and the borrowed month is shifted
// (SD_DISAGG_SHIFT) or scaled (SD_DISAGG_SCALE_MEAN / _SUM) so that its monthly statistic equals target[m].  Every cell borrows the
// same rows, so the row map is wave-uniform.  pandas makes the tables on the host (skdownscale_amd/disagg.py: time_map); the launch
// plan and the refusals are in sd_disagg_plan.h.
//
// disagg_kernel<S, V, OP>: a workgroup of four waves owns one tile of 64 * V adjacent cells and a run of kBinsPerGroup consecutive bins;
// each wave takes kBinsPerWave whole bins, one after the other.  A lane owns its V cells for the whole bin.  src_row and offsets are
// indexed by wave-uniform values only, so they are read through scalar loads.
//   pass 1: the borrowed rows in time order, the loads of a batch of kBatch rows issued before any of their arithmetic; NaN samples are
//           skipped by a select, acc is the plain running sum and cnt the number of the others -- the statistic of resample_kernel.
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

#include "sd_disagg_plan.h"
#include "sd_internal.h"
#include "sd_state.h"

namespace {
using namespace sddg;

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

template <typename S, int V, int OP>
__global__ void __launch_bounds__(kLanes* kWaves)
    disagg_kernel(const double* __restrict__ target, int64_t ld_t, const S* __restrict__ obs, int64_t ld_obs, int64_t C,
                  const int64_t* __restrict__ src_row, const int64_t* __restrict__ offsets, int64_t M, int64_t ctiles,
                  const double* __restrict__ climo, int64_t ld_c, const int32_t* __restrict__ group, double* __restrict__ out, int64_t ld_out) {
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t ctile = blockIdx.x % ctiles, bins = blockIdx.x / ctiles;
    const int64_t c0 = (ctile * kLanes + lane) * V;  // (V divides C: the V cells are inside or outside together)
    if (c0 >= C) return;
    const int64_t m0 = bins * kBinsPerGroup + (int64_t)wave * kBinsPerWave;
    const S* const col = obs + c0;
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
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0, cnt[v] = 0;
        for (int64_t r = r0; r < r1; r += kBatch) {
            Cells<S, V> q[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) q[u] = *reinterpret_cast<const Cells<S, V>*>(col + src_row[min(r + u, r1 - 1)] * ld_obs);
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
#pragma unroll
            for (int u = 0; u < kBatch; ++u) q[u] = *reinterpret_cast<const Cells<S, V>*>(col + src_row[min(r + u, r1 - 1)] * ld_obs);
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

template <typename S, int V>
int launch_op(sd_ctx* ctx, const DisaggCall& c, const DisaggPlan& pl, const double* target, const S* obs, const DisaggTables& t,
              const double* climo, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
#define SD_DISAGG_LAUNCH(OP)                                                                                                                \
    SD_LAUNCH(ctx, "disagg_kernel", (disagg_kernel<S, V, OP>), grid, block, 0, target, c.ld_t, obs, c.ld_obs, c.C, t.src_row, t.offsets, c.M, \
              pl.ctiles, climo, c.ld_c, t.group, out, c.ld_out)
    if (c.op == SD_DISAGG_SHIFT)
        SD_DISAGG_LAUNCH(SD_DISAGG_SHIFT);
    else if (c.op == SD_DISAGG_SCALE_MEAN)
        SD_DISAGG_LAUNCH(SD_DISAGG_SCALE_MEAN);
    else
        SD_DISAGG_LAUNCH(SD_DISAGG_SCALE_SUM);
#undef SD_DISAGG_LAUNCH
    return SD_OK;
}

int launch(sd_ctx* ctx, const DisaggCall& c, const DisaggPlan& pl, const double* target, const void* obs, const DisaggTables& t,
           const double* climo, double* out) {
    if (c.obs_is_f32) {
        const float* s = (const float*)obs;
        return pl.cols == 4 ? launch_op<float, 4>(ctx, c, pl, target, s, t, climo, out)
               : pl.cols == 2 ? launch_op<float, 2>(ctx, c, pl, target, s, t, climo, out)
                              : launch_op<float, 1>(ctx, c, pl, target, s, t, climo, out);
    }
    const double* s = (const double*)obs;
    return pl.cols == 2 ? launch_op<double, 2>(ctx, c, pl, target, s, t, climo, out) : launch_op<double, 1>(ctx, c, pl, target, s, t, climo, out);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int sd_disagg_dev(sd_ctx* ctx, int op, const double* target_dev, int64_t ld_t, const void* obs_dev, int obs_is_f32, int64_t ld_obs, int64_t To,
                  int64_t C, const int64_t* src_row, int64_t Tout, const int64_t* offsets, int64_t M, const double* climo_dev, int64_t ld_c,
                  int64_t G, const int32_t* group, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && target_dev && obs_dev && src_row && offsets && out_dev, "sd_disagg: NULL argument");
    DisaggCall c;
    c.op = op, c.obs_is_f32 = obs_is_f32 != 0;
    c.To = To, c.C = C, c.Tout = Tout, c.M = M;
    c.ld_t = ld_t, c.ld_obs = ld_obs, c.ld_out = ld_out;
    c.has_climo = climo_dev != nullptr, c.has_group = group != nullptr;
    c.G = G, c.ld_c = ld_c;
    c.target_aligned16 = aligned16(target_dev), c.obs_aligned16 = aligned16(obs_dev), c.out_aligned16 = aligned16(out_dev);
    c.climo_aligned16 = aligned16(climo_dev);
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
    DisaggCall c;  // (before the upload: tight rows, aligned scratch)
    c.op = op, c.obs_is_f32 = obs_is_f32 != 0;
    c.To = To, c.C = C, c.Tout = Tout, c.M = M;
    c.ld_t = c.ld_obs = c.ld_out = c.ld_c = C;
    c.has_climo = climo_host != nullptr, c.has_group = group != nullptr, c.G = G;
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
