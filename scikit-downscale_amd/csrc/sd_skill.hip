// Paired skill statistics per period of two [T, C] fields walked in lock-step (GridArray.compare(other).resample(time=rule).count() /
// .bias() / .ratio() / .mae() / .rmse() / .corr() / .std_ratio()): bin m is the run of rows offsets[m] .. offsets[m + 1] - 1, made by
// pandas on the host.  The rule is stated in include/sd_downscale.h; the launch plan and the refusals are in sd_skill_plan.h.
//
// skill_kernel<SA, SB, V>: the geometry and the batched loads are those of sd_bins.h (lane_place, load_batch): a lane owns V adjacent
// cells for a whole bin, a wave takes kBinsPerWave whole bins, the loads of a batch of kBatch rows of both sources are issued before any
// of their arithmetic.  load_batch reads the bin's last row again for rows past its end: such a row is no valid pair (`inside` gates
// it, so it adds +0.0 to every sum).  Pass 1 keeps n and the five sums (sa, sb, sd, sabs, sq) of each cell in registers and serves
// count .. rmse by itself.  Pass 2 -- the centred sums qaa, qbb, qab around the means sa / n and sb / n -- runs over the same rows of
// the bin only when a wave-uniform flag, made from the packed statistic codes, says corr or std_ratio was asked for.  A bin ends with
// nstat stores of V doubles per lane, selected by wave-uniform codes: several statistics cost one read of both fields per pass.  No
// LDS, no atomics.  Every sum adds one term per row in time order, one IEEE operation per step (the library is built with
// -ffp-contract=off): the bits do not depend on V, the leading dimensions or the grid.
//
// Algorithmic bytes: (sizeof(SA) + sizeof(SB)) * T * C read per pass (one pass for count .. rmse, two with corr or std_ratio)
// + 8 * nstat * M * C written.
//
// skill_groups_kernel<SA, SB, V, BPW> (GridArray.compare(other).groupby("time.month").bias() ...) is skill_kernel with a row map, the way
// groupby_reduce_kernel is resample_kernel with one: row i of group g is row rows[offsets[g] + i] of both fields, rows / offsets being
// the counting sort of the group ids (sd_groupby_plan.h: groupby_tables).  Both kernels call skill_bin, the two passes and the finishing
// switch written once on a row map: a group is evaluated exactly as a bin of its rows.  A wave takes BPW whole groups: one where the
// plan found few groups (G <= kFewGroups), else kBinsPerWave.  Its bytes are those of skill_kernel plus 8 * T bytes of row table per
// pass and tile of cells (scalar loads); the compiler's figures of its eighteen instantiations are in profiles/skill_groups/README.md.
//
// A bin is never split across lanes: one very long bin over few cells has little parallelism.  That is the price of the fixed
// summation order (a split bin would add its partial sums in another order and change the last bits).
//
// Registers: the state of a cell is n and five doubles (11 registers) in pass 1 and five more doubles in pass 2, so at most 4 x 11
// for V = 4 beside the 2 x kBatch rows in flight, against __launch_bounds__(256).  The compiler's figures for every instantiation
// are in profiles/skill/README.md; none needs scratch.
#include <vector>

#include "sd_bins.h"
#include "sd_internal.h"
#include "sd_skill_plan.h"
#include "sd_state.h"

namespace {
using namespace sdbn;
using sdsk::kMaxStats;

// one bin of one lane: both passes over the rows row_of(r0) .. row_of(r1 - 1) of the lane's cells at acol / bcol, then the nstat stores
// at o.  Everything but the lane's columns is wave-uniform.  skill_kernel calls it with the identity, skill_groups_kernel with the row
// table of its group: one body, one sequence of IEEE operations per value.
template <typename SA, typename SB, int V, class Row>
__device__ __forceinline__ void skill_bin(const SA* acol, int64_t ld_a, const SB* bcol, int64_t ld_b, int64_t r0, int64_t r1, Row row_of, int centred,
                                          int stats, int nstat, double* o, int64_t stride_out) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int n[V];
    double sa[V], sb[V], sd[V], sabs[V], sq[V];
#pragma unroll
    for (int v = 0; v < V; ++v) n[v] = 0, sa[v] = sb[v] = sd[v] = sabs[v] = sq[v] = 0.0;
    for (int64_t r = r0; r < r1; r += kBatch) {
        Cells<SA, V> qa[kBatch];
        Cells<SB, V> qb[kBatch];
        load_batch(qa, acol, ld_a, r, r1, row_of);
        load_batch(qb, bcol, ld_b, r, r1, row_of);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const bool inside = r + u < r1;  // wave-uniform: a row past the bin's end is the clamped last row, not a step
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double x = (double)qa[u].v[v], y = (double)qb[u].v[v];
                const bool ok = inside && x == x && y == y;
                const double d = x - y;
                n[v] += ok ? 1 : 0;
                sa[v] += ok ? x : 0.0;
                sb[v] += ok ? y : 0.0;
                sd[v] += ok ? d : 0.0;
                sabs[v] += ok ? fabs(d) : 0.0;
                sq[v] += ok ? d * d : 0.0;
            }
        }
    }
    double qaa[V], qbb[V], qab[V];
#pragma unroll
    for (int v = 0; v < V; ++v) qaa[v] = qbb[v] = qab[v] = 0.0;
    if (centred) {  // wave-uniform
        double ma[V], mb[V];
#pragma unroll
        for (int v = 0; v < V; ++v) ma[v] = sa[v] / (double)n[v], mb[v] = sb[v] / (double)n[v];  // (NaN for n == 0: nothing is added then)
        for (int64_t r = r0; r < r1; r += kBatch) {
            Cells<SA, V> qa[kBatch];
            Cells<SB, V> qb[kBatch];
            load_batch(qa, acol, ld_a, r, r1, row_of);
            load_batch(qb, bcol, ld_b, r, r1, row_of);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool inside = r + u < r1;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double x = (double)qa[u].v[v], y = (double)qb[u].v[v];
                    const bool ok = inside && x == x && y == y;
                    const double da = x - ma[v], db = y - mb[v];
                    qaa[v] += ok ? da * da : 0.0;
                    qbb[v] += ok ? db * db : 0.0;
                    qab[v] += ok ? da * db : 0.0;
                }
            }
        }
    }
#pragma unroll 1
    for (int s = 0; s < nstat; ++s) {
        const int code = (stats >> (4 * s)) & 15;  // wave-uniform: the switch is a scalar branch
        double res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double dn = (double)n[v];
            double r;
            switch (code) {
                case SD_SKILL_COUNT: r = dn; break;
                case SD_SKILL_BIAS: r = sd[v] / dn; break;
                case SD_SKILL_RATIO: r = sa[v] / sb[v]; break;
                case SD_SKILL_MAE: r = sabs[v] / dn; break;
                case SD_SKILL_RMSE: r = sqrt(sq[v] / dn); break;
                case SD_SKILL_CORR: {
                    r = qab[v] / (sqrt(qaa[v]) * sqrt(qbb[v]));
                    r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;  // (NaN stays NaN)
                    if (n[v] < 2 || qaa[v] == 0.0 || qbb[v] == 0.0) r = nan;
                    break;
                }
                default: r = n[v] < 2 ? nan : sqrt(qaa[v] / qbb[v]); break;  // SD_SKILL_STD_RATIO
            }
            res[v] = (n[v] == 0 && code != SD_SKILL_COUNT) ? nan : r;
        }
        store_doubles<V>(o + s * stride_out, res);
    }
}

// wave-uniform: a statistic of the second pass is among the packed codes
__device__ __forceinline__ int skill_centred(int stats, int nstat) {
    int centred = 0;
    for (int s = 0; s < nstat; ++s) {
        const int code = (stats >> (4 * s)) & 15;
        centred |= (int)(code == SD_SKILL_CORR) | (int)(code == SD_SKILL_STD_RATIO);
    }
    return centred;
}

template <typename SA, typename SB, int V>
__global__ void __launch_bounds__(kLanes* kWaves)
    skill_kernel(const SA* __restrict__ a, int64_t ld_a, const SB* __restrict__ b, int64_t ld_b, int64_t C, const int64_t* __restrict__ offsets,
                 int64_t M, int64_t ctiles, int stats, int nstat, double* __restrict__ out, int64_t ld_out, int64_t stride_out) {
    int64_t c0, m0;
    if (!lane_place<V>(ctiles, C, c0, m0)) return;
    const int centred = skill_centred(stats, nstat);
    for (int k = 0; k < kBinsPerWave; ++k) {
        const int64_t m = m0 + k;
        if (m >= M) break;  // wave-uniform
        skill_bin<SA, SB, V>(a + c0, ld_a, b + c0, ld_b, offsets[m], offsets[m + 1], [](int64_t i) { return i; }, centred, stats, nstat,
                             out + m * ld_out + c0, stride_out);
    }
}

// skill_kernel with a row map, the way groupby_reduce_kernel is resample_kernel with one: row i of group g is row rows[offsets[g] + i]
// of both fields.  rows and offsets are indexed by wave-uniform values only (scalar loads) and are never written.  A wave takes BPW whole
// groups (1 where the plan found few groups, else kBinsPerWave).
template <typename SA, typename SB, int V, int BPW>
__global__ void __launch_bounds__(kLanes* kWaves)
    skill_groups_kernel(const SA* __restrict__ a, int64_t ld_a, const SB* __restrict__ b, int64_t ld_b, int64_t C, const int64_t* __restrict__ rows,
                        const int64_t* __restrict__ offsets, int64_t G, int64_t ctiles, int stats, int nstat, double* __restrict__ out,
                        int64_t ld_out, int64_t stride_out) {
    int64_t c0, g0;
    if (!lane_place<V, BPW>(ctiles, C, c0, g0)) return;
    const int centred = skill_centred(stats, nstat);
    for (int k = 0; k < BPW; ++k) {
        const int64_t g = g0 + k;
        if (g >= G) break;  // wave-uniform
        skill_bin<SA, SB, V>(a + c0, ld_a, b + c0, ld_b, offsets[g], offsets[g + 1], [&](int64_t i) { return rows[i]; }, centred, stats, nstat,
                             out + g * ld_out + c0, stride_out);
    }
}

template <typename SA, typename SB, int V>
int launch_as(sd_ctx* ctx, const SkillCall& c, const SkillPlan& pl, const void* a, const void* b, const int64_t* offsets, int stats, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    SD_LAUNCH(ctx, "skill_kernel", (skill_kernel<SA, SB, V>), grid, block, 0, (const SA*)a, c.ld_a, (const SB*)b, c.ld_b, c.C, offsets, c.M, pl.ctiles,
              stats, c.nstat, out, c.ld_out, c.stride_out);
    return SD_OK;
}

// the four dtype pairs by the cells per lane the plan can choose for them: four only where both sources are float32
int launch(sd_ctx* ctx, const SkillCall& c, const SkillPlan& pl, const void* a, const void* b, const int64_t* offsets, double* out) {
    int stats = 0;  // the codes, four bits each
    for (int s = 0; s < c.nstat; ++s) stats |= c.stats[s] << (4 * s);
    const int V = pl.cols;
#define SD_SKILL_PAIR(SA, SB) (V == 2 ? launch_as<SA, SB, 2>(ctx, c, pl, a, b, offsets, stats, out) : launch_as<SA, SB, 1>(ctx, c, pl, a, b, offsets, stats, out))
    if (c.a_is_f32 && c.b_is_f32) return V == 4 ? launch_as<float, float, 4>(ctx, c, pl, a, b, offsets, stats, out) : SD_SKILL_PAIR(float, float);
    if (c.a_is_f32) return SD_SKILL_PAIR(float, double);
    if (c.b_is_f32) return SD_SKILL_PAIR(double, float);
    return SD_SKILL_PAIR(double, double);
#undef SD_SKILL_PAIR
}

template <typename SA, typename SB, int V>
int launch_groups_as(sd_ctx* ctx, const SkillCall& c, const SkillGroupsPlan& pl, const void* a, const void* b, const int64_t* rows,
                     const int64_t* offsets, int stats, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    if (pl.bins_per_wave == 1)
        SD_LAUNCH(ctx, "skill_groups_kernel", (skill_groups_kernel<SA, SB, V, 1>), grid, block, 0, (const SA*)a, c.ld_a, (const SB*)b, c.ld_b, c.C, rows,
                  offsets, c.M, pl.ctiles, stats, c.nstat, out, c.ld_out, c.stride_out);
    else
        SD_LAUNCH(ctx, "skill_groups_kernel", (skill_groups_kernel<SA, SB, V, kBinsPerWave>), grid, block, 0, (const SA*)a, c.ld_a, (const SB*)b, c.ld_b,
                  c.C, rows, offsets, c.M, pl.ctiles, stats, c.nstat, out, c.ld_out, c.stride_out);
    return SD_OK;
}

// the same table of dtype pairs and cells per lane as launch
int launch_groups(sd_ctx* ctx, const SkillCall& c, const SkillGroupsPlan& pl, const void* a, const void* b, const int64_t* rows, const int64_t* offsets,
                  double* out) {
    int stats = 0;
    for (int s = 0; s < c.nstat; ++s) stats |= c.stats[s] << (4 * s);
    const int V = pl.cols;
#define SD_SKILL_PAIR(SA, SB) \
    (V == 2 ? launch_groups_as<SA, SB, 2>(ctx, c, pl, a, b, rows, offsets, stats, out) : launch_groups_as<SA, SB, 1>(ctx, c, pl, a, b, rows, offsets, stats, out))
    if (c.a_is_f32 && c.b_is_f32)
        return V == 4 ? launch_groups_as<float, float, 4>(ctx, c, pl, a, b, rows, offsets, stats, out) : SD_SKILL_PAIR(float, float);
    if (c.a_is_f32) return SD_SKILL_PAIR(float, double);
    if (c.b_is_f32) return SD_SKILL_PAIR(double, float);
    return SD_SKILL_PAIR(double, double);
#undef SD_SKILL_PAIR
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

SkillCall call_of(int a_is_f32, int64_t ld_a, int b_is_f32, int64_t ld_b, int64_t T, int64_t C, int64_t M, const int* stats, int nstat,
                  int64_t ld_out, int64_t stride_out, const void* a, const void* b, const void* out) {
    SkillCall c;
    c.a_is_f32 = a_is_f32 != 0, c.b_is_f32 = b_is_f32 != 0;
    c.T = T, c.C = C, c.ld_a = ld_a, c.ld_b = ld_b, c.M = M;
    c.nstat = nstat;
    for (int s = 0; s < nstat && s < kMaxStats; ++s) c.stats[s] = stats[s];
    c.ld_out = ld_out, c.stride_out = stride_out;
    c.a_aligned16 = aligned16(a), c.b_aligned16 = aligned16(b), c.out_aligned16 = aligned16(out);
    return c;
}

}  // namespace

extern "C" {

int sd_skill_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T, int64_t C,
                 const int64_t* offsets, int64_t M, const int* stats, int nstat, double* out_dev, int64_t ld_out, int64_t stride_out) {
    SD_CHECK_ARG(ctx && a_dev && b_dev && offsets && stats && out_dev, "sd_skill: NULL argument");
    const SkillCall c = call_of(a_is_f32, ld_a, b_is_f32, ld_b, T, C, M, stats, nstat, ld_out, stride_out, a_dev, b_dev, out_dev);
    const SkillPlan pl = skill_plan(c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch bins;
    SD_TRY(upload(ctx, bins, std::vector<int64_t>(offsets, offsets + M + 1)));
    SD_TRY(launch(ctx, c, pl, a_dev, b_dev, bins.as<int64_t>(), out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_skill(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C, const int64_t* offsets,
             int64_t M, const int* stats, int nstat, double* out_host) {
    SD_CHECK_ARG(ctx && a_host && b_host && offsets && stats && out_host, "sd_skill: NULL argument");
    const int64_t stride = M > 0 && C > 0 && M <= INT64_MAX / 8 / C ? M * C : 0;
    const SkillCall c = call_of(a_is_f32, C, b_is_f32, C, T, C, M, stats, nstat, C, stride, nullptr, nullptr, nullptr);  // (before the upload)
    const SkillPlan pl = skill_plan(c, offsets);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t a_bytes = (a_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const size_t b_bytes = (b_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(a_host, a_bytes), sd_in(b_host, b_bytes), sd_out(out_host, sizeof(double) * (size_t)nstat * M * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_skill_dev(ctx, d[0], a_is_f32, C, d[1], b_is_f32, C, T, C, offsets, M, stats, nstat, (double*)d[2], C, stride);
    });
}

int sd_skill_groups_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T, int64_t C,
                        const int32_t* group, int64_t G, const int* stats, int nstat, double* out_dev, int64_t ld_out, int64_t stride_out) {
    SD_CHECK_ARG(ctx && a_dev && b_dev && group && stats && out_dev, "sd_skill_groups: NULL argument");
    const SkillCall c = call_of(a_is_f32, ld_a, b_is_f32, ld_b, T, C, G, stats, nstat, ld_out, stride_out, a_dev, b_dev, out_dev);
    const SkillGroupsPlan pl = skill_groups_plan(c, group);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> rows((size_t)T), offsets((size_t)G + 1);
    groupby_tables(group, T, G, rows.data(), offsets.data());
    sd_scratch drows, doffsets;
    SD_TRY(upload(ctx, drows, rows));
    SD_TRY(upload(ctx, doffsets, offsets));
    SD_TRY(launch_groups(ctx, c, pl, a_dev, b_dev, drows.as<int64_t>(), doffsets.as<int64_t>(), out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_skill_groups(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C, const int32_t* group,
                    int64_t G, const int* stats, int nstat, double* out_host) {
    SD_CHECK_ARG(ctx && a_host && b_host && group && stats && out_host, "sd_skill_groups: NULL argument");
    const int64_t stride = G > 0 && C > 0 && G <= INT64_MAX / 8 / C ? G * C : 0;
    const SkillCall c = call_of(a_is_f32, C, b_is_f32, C, T, C, G, stats, nstat, C, stride, nullptr, nullptr, nullptr);  // (before the upload)
    const SkillGroupsPlan pl = skill_groups_plan(c, group);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t a_bytes = (a_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const size_t b_bytes = (b_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(a_host, a_bytes), sd_in(b_host, b_bytes), sd_out(out_host, sizeof(double) * (size_t)nstat * G * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_skill_groups_dev(ctx, d[0], a_is_f32, C, d[1], b_is_f32, C, T, C, group, G, stats, nstat, (double*)d[2], C, stride);
    });
}

}  // extern "C"
