// Grouping of the time axis of a [T, C] field (GridArray.groupby("time.month").mean() / .sum(), gb - clim, gb / clim; pandas'
// DataFrame.groupby(key).mean() / .sum() per cell and the reference's _remove_climatology): row t carries the group id group[t],
// made by pandas / NumPy on the host.  The launch plans, the refusals and the counting sort of the ids are in sd_groupby_plan.h.
//
// groupby_reduce_kernel<S, V, BPW>: a group is a bin of sd_bins.h whose rows are not consecutive: row i of bin g is row
// rows[offsets[g] + i] of the field, rows / offsets being the counting sort of the ids (indexed by wave-uniform values only, so they
// are read through scalar loads).  The geometry, the batched loads and the statistic are those of sd_bins.h; a wave takes BPW whole
// groups (1 where the plan found few groups, else kBinsPerWave) and a lane owns its V cells of a group for the whole call.  The
// statistic is the seeded one (bin_accumulate): acc / cnt start from sum / count with carry, from zero without; they are written back,
// and the result is finished into out in the same kernel when out is given.  A lane adds the samples of its cells in row order, so a
// result depends neither on the launch geometry nor on how a caller cuts the time axis into calls.  No LDS, no atomics.  Algorithmic
// bytes: sizeof(S) * T * C read + 12 * G * C accumulator traffic per call (twice with carry) + 8 * G * C written.
//
// groupby_apply_kernel<S, V, OP>: streams tiles of 64 * V cells by runs of kApplyRun rows (the bins of its plan; a wave takes
// kBinsPerWave runs).  group[t] is wave-uniform and read through a scalar load; the loads of a batch of kBatch rows -- the source row
// and its row of the table -- are issued before their arithmetic; one coalesced 16-byte store of V doubles per lane and row (the plan
// gives V <= 2 for float32 sources too: four cells per lane measured slower, profiles/groupby/).  One IEEE operation per element
// (-ffp-contract=off).  Algorithmic bytes: sizeof(S) * T * C + 8 * G * C read, 8 * T * C written.
//
// A group is never split across lanes: few long groups over few cells have little parallelism.  That is the price of the fixed order.
#include <vector>

#include "sd_bins.h"
#include "sd_groupby_plan.h"
#include "sd_internal.h"
#include "sd_state.h"

namespace {
using namespace sdbn;
using sdgb::kApplyRun;

template <typename S, int V, int BPW>
__global__ void __launch_bounds__(kLanes* kWaves)
    groupby_reduce_kernel(const S* __restrict__ src, int64_t ld, int64_t C, const int64_t* __restrict__ rows, const int64_t* __restrict__ offsets,
                          int64_t G, int64_t ctiles, double* __restrict__ sum, int32_t* __restrict__ count, int64_t ld_acc, int carry, int op,
                          double* __restrict__ out, int64_t ld_out) {
    int64_t c0, g0;
    if (!lane_place<V, BPW>(ctiles, C, c0, g0)) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int b = 0; b < BPW; ++b) {
        const int64_t g = g0 + b;
        if (g >= G) break;  // wave-uniform
        double acc[V];
        int cnt[V];
        double* const s = sum + g * ld_acc + c0;
        Cells<int32_t, V>* const n = reinterpret_cast<Cells<int32_t, V>*>(count + g * ld_acc + c0);
        if (carry) {
            load_doubles<V>(s, acc);
            const Cells<int32_t, V> q = *n;
#pragma unroll
            for (int v = 0; v < V; ++v) cnt[v] = q.v[v];
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0, cnt[v] = 0;
        }
        bin_accumulate<S, V>(src + c0, ld, offsets[g], offsets[g + 1], [&](int64_t i) { return rows[i]; }, acc, cnt);
        store_doubles<V>(s, acc);
        Cells<int32_t, V> q;
#pragma unroll
        for (int v = 0; v < V; ++v) q.v[v] = cnt[v];
        *n = q;
        if (out != nullptr) {
            double res[V];
#pragma unroll
            for (int v = 0; v < V; ++v) res[v] = op == SD_GROUPBY_MEAN ? (cnt[v] > 0 ? acc[v] / (double)cnt[v] : nan) : acc[v];
            store_doubles<V>(out + g * ld_out + c0, res);
        }
    }
}

template <typename S, int V, int OP>
__global__ void __launch_bounds__(kLanes* kWaves)
    groupby_apply_kernel(const S* __restrict__ src, int64_t ld, int64_t T, int64_t C, const int32_t* __restrict__ group, int64_t ctiles,
                         const double* __restrict__ table, int64_t ld_t, double* __restrict__ out, int64_t ld_out) {
    int64_t c0, m0;
    if (!lane_place<V>(ctiles, C, c0, m0)) return;
    const int64_t r0 = m0 * kApplyRun, r1 = min(T, r0 + (int64_t)kBinsPerWave * kApplyRun);  // wave-uniform
    const S* const col = src + c0;
    const double* const tab = table + c0;
    double* const o = out + c0;
    for (int64_t r = r0; r < r1; r += kBatch) {
        Cells<S, V> q[kBatch];
        double t[kBatch][V];
        load_batch(q, col, ld, r, r1, [](int64_t i) { return i; });
#pragma unroll
        for (int u = 0; u < kBatch; ++u) load_doubles<V>(tab + (int64_t)group[min(r + u, r1 - 1)] * ld_t, t[u]);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (r + u >= r1) break;  // wave-uniform
            double res[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double x = (double)q[u].v[v];
                res[v] = OP == SD_GROUPBY_SUB ? x - t[u][v] : OP == SD_GROUPBY_ADD ? x + t[u][v] : OP == SD_GROUPBY_MUL ? x * t[u][v] : x / t[u][v];
            }
            store_doubles<V>(o + (r + u) * ld_out, res);
        }
    }
}

int launch_reduce(sd_ctx* ctx, const GroupbyReduceCall& c, const GroupbyPlan& pl, const void* src, const int64_t* rows, const int64_t* offsets,
                  double* sum, int32_t* count, int carry, double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    return with_cells(c.src_is_f32, pl.cols, src, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
        if (pl.bins_per_wave == 1)
            SD_LAUNCH(ctx, "groupby_reduce_kernel", (groupby_reduce_kernel<S, V, 1>), grid, block, 0, s, c.ld, c.C, rows, offsets, c.G, pl.ctiles, sum,
                      count, c.ld_acc, carry, c.op, out, c.ld_out);
        else
            SD_LAUNCH(ctx, "groupby_reduce_kernel", (groupby_reduce_kernel<S, V, kBinsPerWave>), grid, block, 0, s, c.ld, c.C, rows, offsets, c.G,
                      pl.ctiles, sum, count, c.ld_acc, carry, c.op, out, c.ld_out);
        return (int)SD_OK;
    });
}

int launch_apply(sd_ctx* ctx, const GroupbyApplyCall& c, const GroupbyPlan& pl, const void* src, const int32_t* group, const double* table,
                 double* out) {
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    return with_cells(c.src_is_f32, pl.cols, src, [&](auto* s, auto cols) {
        using S = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
        constexpr int V = decltype(cols)::value;
#define SD_GROUPBY_LAUNCH(OP) \
    SD_LAUNCH(ctx, "groupby_apply_kernel", (groupby_apply_kernel<S, V, OP>), grid, block, 0, s, c.ld, c.T, c.C, group, pl.ctiles, table, c.ld_t, out, c.ld_out)
        if (c.op == SD_GROUPBY_SUB)
            SD_GROUPBY_LAUNCH(SD_GROUPBY_SUB);
        else if (c.op == SD_GROUPBY_ADD)
            SD_GROUPBY_LAUNCH(SD_GROUPBY_ADD);
        else if (c.op == SD_GROUPBY_MUL)
            SD_GROUPBY_LAUNCH(SD_GROUPBY_MUL);
        else
            SD_GROUPBY_LAUNCH(SD_GROUPBY_DIV);
#undef SD_GROUPBY_LAUNCH
        return (int)SD_OK;
    });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

GroupbyReduceCall reduce_call(int op, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t G, int64_t ld_acc, bool has_out, int64_t ld_out,
                              const void* src, const void* sum, const void* count, const void* out) {
    GroupbyReduceCall c;
    c.op = op, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.G = G, c.ld_acc = ld_acc, c.has_out = has_out, c.ld_out = ld_out;
    c.src_aligned16 = aligned16(src), c.sum_aligned16 = aligned16(sum), c.count_aligned16 = aligned16(count), c.out_aligned16 = aligned16(out);
    return c;
}

GroupbyApplyCall apply_call(int op, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t G, int64_t ld_t, int64_t ld_out, const void* src,
                            const void* table, const void* out) {
    GroupbyApplyCall c;
    c.op = op, c.src_is_f32 = src_is_f32 != 0;
    c.T = T, c.C = C, c.ld = ld, c.G = G, c.ld_t = ld_t, c.ld_out = ld_out;
    c.src_aligned16 = aligned16(src), c.table_aligned16 = aligned16(table), c.out_aligned16 = aligned16(out);
    return c;
}

}  // namespace

extern "C" {

int sd_groupby_reduce_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int32_t* group,
                          int64_t G, double* sum_dev, int32_t* count_dev, int64_t ld_acc, int carry, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && src_dev && group && sum_dev && count_dev, "sd_groupby_reduce: NULL argument");
    const GroupbyReduceCall c = reduce_call(op, src_is_f32, ld, T, C, G, ld_acc, out_dev != nullptr, ld_out, src_dev, sum_dev, count_dev, out_dev);
    const GroupbyPlan pl = groupby_check_groups(groupby_reduce_plan(c), "sd_groupby_reduce", group, T, G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> rows((size_t)T), offsets((size_t)G + 1);
    groupby_tables(group, T, G, rows.data(), offsets.data());
    sd_scratch drows, doffsets;
    SD_TRY(upload(ctx, drows, rows));
    SD_TRY(upload(ctx, doffsets, offsets));
    SD_TRY(launch_reduce(ctx, c, pl, src_dev, drows.as<int64_t>(), doffsets.as<int64_t>(), sum_dev, count_dev, carry, out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_groupby_reduce(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group, int64_t G,
                      double* out_host) {
    SD_CHECK_ARG(ctx && src_host && group && out_host, "sd_groupby_reduce: NULL argument");
    const GroupbyReduceCall c = reduce_call(op, src_is_f32, C, T, C, G, C, true, C, nullptr, nullptr, nullptr, nullptr);  // (before the upload)
    const GroupbyPlan pl = groupby_check_groups(groupby_reduce_plan(c), "sd_groupby_reduce", group, T, G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C, cells = (size_t)G * C;
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch sum, count;  // (carry == 0: they need no initialisation)
    SD_HIP(sum.alloc(ctx, sizeof(double) * cells));
    SD_HIP(count.alloc(ctx, sizeof(int32_t) * cells));
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_out(out_host, sizeof(double) * cells)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_groupby_reduce_dev(ctx, op, d[0], src_is_f32, C, T, C, group, G, sum.as<double>(), count.as<int32_t>(), C, 0, (double*)d[1], C);
    });
}

int sd_groupby_apply_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int32_t* group,
                         int64_t G, const double* table_dev, int64_t ld_t, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && src_dev && group && table_dev && out_dev, "sd_groupby_apply: NULL argument");
    const GroupbyApplyCall c = apply_call(op, src_is_f32, ld, T, C, G, ld_t, ld_out, src_dev, table_dev, out_dev);
    const GroupbyPlan pl = groupby_check_groups(groupby_apply_plan(c), "sd_groupby_apply", group, T, G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch groups;
    SD_TRY(upload(ctx, groups, std::vector<int32_t>(group, group + T)));
    SD_TRY(launch_apply(ctx, c, pl, src_dev, groups.as<int32_t>(), table_dev, out_dev));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int sd_groupby_apply(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group, int64_t G,
                     const double* table_host, double* out_host) {
    SD_CHECK_ARG(ctx && src_host && group && table_host && out_host, "sd_groupby_apply: NULL argument");
    const GroupbyApplyCall c = apply_call(op, src_is_f32, C, T, C, G, C, C, nullptr, nullptr, nullptr);  // (before the upload)
    const GroupbyPlan pl = groupby_check_groups(groupby_apply_plan(c), "sd_groupby_apply", group, T, G);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    const size_t in_bytes = (src_is_f32 ? sizeof(float) : sizeof(double)) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(src_host, in_bytes), sd_in(table_host, sizeof(double) * (size_t)G * C), sd_out(out_host, sizeof(double) * (size_t)T * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_groupby_apply_dev(ctx, op, d[0], src_is_f32, C, T, C, group, G, (const double*)d[1], C, (double*)d[2], C);
    });
}

}  // extern "C"
