// GARD analog models (PureAnalog / AnalogRegression), batched over the cell axis.
//
// Reference (file:line under skdownscale/pointwise_models/gard.py): AnalogBase.fit 58-87 (KDTree),
// PureAnalog.predict 273-364, AnalogRegression.predict/_predict_one_step 152-224 (thresh=None).
// KDTree.query is restated as: k training rows with the smallest reduced distance
// rdist = sum_f (q_f - x_f)^2 (accumulated f = 0..F-1, no FMA), ascending by (rdist, index).
//
// Which kernels a call runs is decided before its first launch by analog_plan() (sd_analog_plan.h, a pure host function checked by
// tests/test_analog_plan.py); every entry point below reads: validate -> build the call -> plan -> allocate -> run.
// fit   : mask / finite check, cell-major copies Xc[C][F][T], yc[C][T] (tiled LDS transpose); for F == 1
//         additionally the sorted view of a cell: xs[C][T] (values by (x, index)), xi[C][T] (their training
//         indices), yx[C][T] (y in that order) and pq[C][T+1][2] (prefix sums of the centred yx and its
//         squares) -- analog_sort2_kernel: workgroup merge sort (sd_sortnet.h); rx[C][T+1], the cross term of
//         the one-feature regression, is added by analog_rx_kernel on the first AnalogRegression call.  For
//         F > 1 a copy of the training points sorted by feature 0 (ps, indices xi).
// predict, F == 1 (one persistent workgroup per cell, queries and outputs through cell-major staging):
//   analog_f1_mean3_kernel  mean_analogs without a threshold: window search over xs in LDS, then the two prefix-sum
//                           components staged through the same LDS array (three generations per cell);
//   analog_f1_mean_kernel   a single analog, AnalogRegression, weighted / thresholded kinds: window search over xs
//                           in LDS, prefix sums or the window of yx read from memory (single pass);
//   analog_f1_window_kernel the other PureAnalog kinds: k-NN window over xs, statistics from yx, both
//                           LDS-resident per value range;
//   analog_f1_predict_kernel / f1_walk_query  exact (rdist, index)-ordered two-pointer walk: 'sample_analogs',
//                           neighbour outputs, and any query whose window has a tie on its boundary.
// predict, F > 1: analog_slab_topk_kernel (sd_analog_topk.h; k <= 30, F <= 6: one wave per 64 queries sorted by feature 0, only the
//   reachable slab of the feature-0 sorted copy is scanned, the 64 x 64 mask of a chunk from the matrix cores, candidate lists pruned
//   by a register sorting network); analog_slab_predict_kernel (the same scan with scalar-loaded points and a top-k heap in LDS:
//   larger k / F and the batches the first hands back);
//   analog_bf2_predict_kernel (same scanner over the whole set in index order); analog_bf_predict_kernel
//   (LDS-staged tiles, lists in global scratch) for k > 208.
// fit + predict in one call (sd_analog_fit_predict*): analog_f1_fused_kernel -- the workgroup that merged a cell's sorted runs
//   answers its queries (the mean3 phases) without a fitted state in memory; cells it hands back and every other configuration
//   take fit -> predict internally.
// Epilogues: PureAnalog statistics (gard.py:303-346), per-query least squares (gard.py:194-224).
// Layout of the sources: the launch plan and the sizing constants in sd_analog_plan.h; kernels and their launchers in
// sd_analog_fit.h (fit), sd_analog_runs.h (value-ordered query staging), sd_analog_epilogue.h, sd_analog_f1.h (F == 1 predict,
// fused kernel), sd_analog_fn.h, sd_analog_topk.h (F > 1 predict), included below; host code and the C entry points here.
#include <algorithm>
#include <cstdlib>

#include "sd_internal.h"
#include "sd_analog_plan.h"
#include "sd_lsq.h"
#include "sd_sortnet.h"
#include "sd_state.h"
#include "sd_wave.h"
#include "sd_wsort.h"

namespace {

using namespace sdan;  // sizing constants and functions of sd_analog_plan.h
static_assert(kMaxF == sdlsq::kMaxF, "sd_analog_plan.h restates the feature limit of sd_lsq.h");

__device__ __forceinline__ bool sd_finite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

// XCD-aware persistent mapping: workgroup b runs on XCD b % 8; give each XCD a contiguous range of
// cells and let its workgroups take adjacent cells at the same time, so 8-byte column reads of
// neighbouring cells merge into full lines in that XCD's L2.
__device__ __forceinline__ int64_t first_cell(int64_t C, int64_t* step, int64_t* end) {
    const int nb = gridDim.x, b = blockIdx.x;
    if (nb % 8 != 0) {
        *step = nb;
        *end = C;
        return b;
    }
    const int64_t cx = (C + 7) / 8;
    const int x = b % 8, j = b / 8;
    *step = nb / 8;
    *end = (x + 1) * cx < C ? (x + 1) * cx : C;
    return x * cx + j;
}

#include "sd_analog_fit.h"
#include "sd_analog_runs.h"
#include "sd_analog_epilogue.h"
#include "sd_analog_f1.h"
#include "sd_analog_fn.h"
#include "sd_analog_topk.h"

__global__ void __launch_bounds__(256) analog_status_public_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                                   int64_t C, int32_t* __restrict__ outp) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const int32_t bits = a[c] | (b ? b[c] : 0);
        outp[c] = (bits & SDI_MASKED) ? SD_CELL_MASKED : (bits & SDI_NONFINITE) ? SD_CELL_NONFINITE : (bits & SDI_ONE_CLASS) ? SD_CELL_ONE_CLASS : SD_CELL_OK;
    }
}

dim3 grid_of(const AnalogLaunch& L) { return dim3((unsigned)L.gx, (unsigned)L.gy, (unsigned)L.gz); }

// The device buffers of a state, each under its name.  Every state has kX, kY and kStatus; which of the others a fit or a first
// predict allocates is the plan's decision (sd_analog_fit_dev, build_prefix_sums), and sd_state_destroy skips the ones that never
// were.  A new buffer gets a name before kAnalogBufs and a line here; one without a line is caught below.
enum AnalogBuf { kX, kY, kStatus, kXs, kXi, kYx, kYbar, kPq, kRx, kXbar, kPs, kAnalogBufs };
std::vector<sd_buf> analog_bufs(const sd_analog_state* st) {
    const size_t T = (size_t)st->T, C = (size_t)st->C, F = (size_t)st->F;
    std::vector<sd_buf> b(kAnalogBufs, sd_buf{nullptr, 0, false});
    b[kX] = sd_buf_of(st->X, T * F * C);
    b[kY] = sd_buf_of(st->y, T * C);
    b[kStatus] = sd_buf_of(st->status, C, true);
    b[kXs] = sd_buf_of(st->xs, T * C);
    b[kXi] = sd_buf_of(st->xi, T * C);
    b[kYx] = sd_buf_of(st->yx, T * C);
    b[kYbar] = sd_buf_of(st->ybar, C);
    b[kPq] = sd_buf_of(st->pq, 2 * (T + 1) * C);
    b[kRx] = sd_buf_of(st->rx, (T + 1) * C);
    b[kXbar] = sd_buf_of(st->xbar, C);
    b[kPs] = sd_buf_of(st->ps, T * F * C);
    for (const sd_buf& x : b)
        if (!x.slot) abort();  // (a name without a line above)
    return b;
}
// Allocates the named buffers.  The state may be const (build_prefix_sums gets it from a predict call): sd_buf_of keeps the address
// of the pointer field as a plain void**, which is the const_cast of a late allocation; every state is created non-const by fit.
int analog_alloc(sd_ctx* ctx, const sd_analog_state* st, std::initializer_list<AnalogBuf> which) {
    const std::vector<sd_buf> all = analog_bufs(st);
    std::vector<sd_buf> some;
    for (AnalogBuf name : which) some.push_back(all[name]);
    return sd_state_alloc(ctx, some);
}

// exclusive prefix sums of the centred analog values (analog_prefix_kernel) and the cross term of the one-feature regression
// (analog_rx_kernel), built when a kernel that reads them from memory first runs on a state (calls on a context are serialised)
int build_prefix_sums(sd_ctx* ctx, const sd_analog_state* st, const AnalogPlan& pl) {
    const int64_t T = st->T, C = st->C;
    if (pl.need_pq) {
        const AnalogLaunch L = analog_launches::prefix_sums(T, C, ctx->cu_count, ctx->lds_max);
        SD_TRY(analog_alloc(ctx, st, {kPq}));
        if (L.lds != 0) {
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_prefix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
            SD_LAUNCH(ctx, "analog_prefix_kernel", analog_prefix_kernel, grid_of(L), dim3(L.block), L.lds, (const double*)st->yx, T, C, st->pq, st->ybar, 1);
        } else {
            SD_LAUNCH(ctx, "analog_prefix_kernel", analog_prefix_direct_kernel, grid_of(L), dim3(L.block), 0, (const double*)st->yx, T, C, st->pq, st->ybar, 1);
        }
    }
    if (pl.need_rx) {
        const AnalogLaunch L = analog_launches::rx(T, C, ctx->cu_count);
        SD_TRY(analog_alloc(ctx, st, {kRx, kXbar}));
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_rx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
        SD_LAUNCH(ctx, "analog_rx_kernel", analog_rx_kernel, grid_of(L), dim3(L.block), L.lds, (const double*)st->xs, (const double*)st->yx,
                  (const double*)st->ybar, T, C, st->rx, st->xbar);
    }
    return SD_OK;
}

// Query staging of the per-cell kernels, one chunk of cells at a time (the staging arrays start at cell 0 of the chunk): queries
// in (cell-major; plain transpose, or value-ordered runs with their time offsets in qtags), results out.  Used by the predict and
// the fused path alike.
struct QueryStaging {
    sd_scratch qc, oc, qtags;
    int alloc(sd_ctx* ctx, const AnalogPlan& pl, int64_t Tq, int64_t C) {
        const int64_t cc_max = C < pl.chunk ? C : pl.chunk;
        SD_HIP(qc.alloc(ctx, sizeof(double) * (size_t)Tq * cc_max));
        SD_HIP(oc.alloc(ctx, sizeof(double) * (size_t)Tq * 3 * cc_max));
        if (pl.runs_q) SD_HIP(qtags.alloc(ctx, sizeof(unsigned short) * (size_t)Tq * cc_max));
        return SD_OK;
    }
    int in(sd_ctx* ctx, const AnalogPlan& pl, const double* Xq, int64_t ld, int64_t Tq, int64_t cc, int32_t* status) {
        const AnalogLaunch L = analog_launches::stage_in(pl, Tq, cc);
        if (pl.runs_q) {
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_query_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
            SD_LAUNCH(ctx, "analog_query_runs_kernel", analog_query_runs_kernel, grid_of(L), dim3(L.block), L.lds, Xq, ld, Tq, cc,
                      (int)((Tq + kRun - 1) / kRun), qc.as<double>(), qtags.as<unsigned short>(), status);
        } else {
            SD_LAUNCH(ctx, "analog_transpose_kernel", analog_transpose_kernel, grid_of(L), dim3(L.block), 0, Xq, ld, Tq, 1, 0, cc, qc.as<double>(), status, 0);
        }
        return SD_OK;
    }
    int out(sd_ctx* ctx, const AnalogPlan& pl, int64_t Tq, int64_t cc, double* out, int64_t ld_out) {
        const AnalogLaunch L = analog_launches::stage_out(pl, Tq, cc);
        if (pl.runs_q) {
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_untranspose_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
            SD_LAUNCH(ctx, "analog_untranspose_runs_kernel", analog_untranspose_runs_kernel, grid_of(L), dim3(L.block), L.lds, (const double*)oc.p,
                      (const unsigned short*)qtags.p, Tq, cc, (int)((Tq + kRun - 1) / kRun), out, ld_out, pl.skip_prob);
        } else {
            SD_LAUNCH(ctx, "analog_untranspose_kernel", analog_untranspose_kernel, grid_of(L), dim3(L.block), 0, (const double*)oc.p, Tq, cc, out, ld_out,
                      pl.skip_prob);
        }
        return SD_OK;
    }
};

// the arguments every predict kernel takes; staged(): results go to the chunk's cell-major staging array
PredictArgs predict_args(const AnalogPlan& pl, int k, int has_thresh, double thresh, const int32_t* sample, int64_t ld_s, double* out,
                         int64_t ld_out, int64_t* inds, double* dist, int32_t* one_class) {
    PredictArgs pa;
    pa.k = k;
    pa.kind = pl.kind;
    pa.has_thresh = has_thresh;
    pa.thresh = thresh;
    pa.sample = sample;
    pa.ld_s = ld_s;
    pa.out = out;
    pa.ld_out = ld_out;
    pa.inds = inds;
    pa.dist = dist;
    pa.oc_Tq = 0;
    pa.one_class = one_class;
    return pa;
}
PredictArgs staged(PredictArgs pa, double* oc, int64_t Tq, int skip_prob) {
    pa.out = oc;
    pa.oc_Tq = Tq;
    pa.skip_prob = skip_prob;
    return pa;
}

int publish_status(sd_ctx* ctx, const int32_t* fit_status, const int32_t* predict_status, int64_t C, sd_scratch* buf, int32_t* cell_status) {
    const AnalogLaunch L = analog_launches::status_public(C);
    SD_HIP(buf->alloc(ctx, sizeof(int32_t) * C));
    SD_LAUNCH(ctx, "analog_status_public_kernel", analog_status_public_kernel, grid_of(L), dim3(L.block), 0, fit_status, predict_status, C, buf->as<int32_t>());
    SD_HIP(hipMemcpyAsync(cell_status, buf->p, sizeof(int32_t) * C, hipMemcpyDeviceToHost, ctx->stream));
    return SD_OK;
}

// the chunk loop of the staged F == 1 paths (Mean3 / Mean / Window)
int predict_staged(sd_ctx* ctx, int mode, const sd_analog_state* st, const AnalogPlan& pl, const AnalogDevSwitches& dev, const double* Xq, int64_t ld,
                   int64_t Tq, const PredictArgs& pa, int32_t* status_p, double* sc_d, int32_t* sc_i) {
    const int64_t C = st->C, T = st->T;
    QueryStaging qs;
    SD_TRY(qs.alloc(ctx, pl, Tq, C));
    SD_TRY(build_prefix_sums(ctx, st, pl));
    const void* kernel = pl.path == AnalogPath::Window ? reinterpret_cast<const void*>(&analog_f1_window_kernel)
                         : pl.path == AnalogPath::Mean ? reinterpret_cast<const void*>(&analog_f1_mean_kernel)
                         : pl.per == 8             ? reinterpret_cast<const void*>(&analog_f1_mean3_kernel<8>)
                         : pl.per == 16            ? reinterpret_cast<const void*>(&analog_f1_mean3_kernel<16>)
                                                   : reinterpret_cast<const void*>(&analog_f1_mean3_kernel<20>);
    SD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    for (int64_t cb = 0; cb < C; cb += pl.chunk) {
        const int64_t cc = C - cb < pl.chunk ? C - cb : pl.chunk;
        SD_TRY(qs.in(ctx, pl, Xq + cb, ld, Tq, cc, status_p + cb));
        const PredictArgs pw = staged(pa, qs.oc.as<double>(), Tq, pl.skip_prob);
        const AnalogLaunch L = analog_launches::per_cell(pl, cc);
        const double* qc = qs.qc.as<double>();
        const double *xs = (const double*)st->xs + cb * T, *yx = (const double*)st->yx + cb * T, *Xc = (const double*)st->X + cb * T,
                     *yc = (const double*)st->y + cb * T;
        const int32_t *xi = (const int32_t*)st->xi + cb * T, *st_fit = (const int32_t*)st->status + cb;
        if (pl.path == AnalogPath::Mean3) {
            long long* trace_dev = nullptr;
            sd_scratch trace_buf;
            if (dev.m3_trace) {  // development library: phase clocks of the first cells of block 0
                SD_HIP(trace_buf.alloc(ctx, sizeof(long long) * 128));
                SD_HIP(hipMemsetAsync(trace_buf.p, 0, sizeof(long long) * 128, ctx->stream));
                trace_dev = trace_buf.as<long long>();
            }
#define SD_MEAN3(PER)                                                                                                                            \
    SD_LAUNCH(ctx, "analog_f1_mean3_kernel", analog_f1_mean3_kernel<PER>, grid_of(L), dim3(L.block), L.lds, qc, Tq, T, cc, xs, xi,                 \
              (const double*)st->ybar + cb, yx, Xc, yc, st_fit, status_p + cb, sc_d, sc_i, pw, pl.skip_prob, trace_dev)
            if (pl.per == 8) SD_MEAN3(8);
            else if (pl.per == 16) SD_MEAN3(16);
            else SD_MEAN3(20);
#undef SD_MEAN3
            if (trace_dev != nullptr) {
                long long h[128];
                SD_HIP(hipMemcpyAsync(h, trace_dev, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
                SD_HIP(hipStreamSynchronize(ctx->stream));
                for (int r = 0; r < 8; ++r) {
                    fprintf(stderr, "mean3 trace cell %d:", r);
                    for (int j = 1; j <= 9; ++j) fprintf(stderr, " %lld", h[r * 16 + j] - h[r * 16 + j - 1]);
                    fprintf(stderr, "\n");
                }
            }
        } else if (pl.path == AnalogPath::Mean) {
            SD_LAUNCH(ctx, "analog_f1_mean_kernel", analog_f1_mean_kernel, grid_of(L), dim3(L.block), L.lds, mode, qc, Tq, T, cc, xs, xi,
                      (const double*)st->pq + 2 * cb * (T + 1), (const double*)st->ybar + cb, (const double*)st->rx + cb * (T + 1),
                      (const double*)st->xbar + cb, yx, Xc, yc, st_fit, status_p + cb, sc_d, sc_i, pw,
                      analog_launches::qsplit(pl, (int)L.gx, cc, Tq), pl.reg_direct ? 1 : 0);
        } else {
            SD_LAUNCH(ctx, "analog_f1_window_kernel", analog_f1_window_kernel, grid_of(L), dim3(L.block), L.lds, mode, qc, Tq, Tq, T, cc, pl.npass, xs,
                      xi, yx, Xc, yc, st_fit, status_p + cb, sc_d, sc_i, pw);
        }
        SD_TRY(qs.out(ctx, pl, Tq, cc, pa.out + cb, pa.ld_out));
    }
    SD_HIP(hipStreamSynchronize(ctx->stream));  // the staging arrays go back to the block cache at scope exit
    return SD_OK;
}

AnalogCall predict_call(int mode, const sd_ctx* ctx, const sd_analog_state* st, int64_t ld, int64_t Tq, int k, int kind, int has_thresh, bool sample,
                        int64_t ld_out, bool neighbors) {
    AnalogCall c;
    c.op = mode == 1 ? AnalogOp::RegPredict : AnalogOp::Predict;
    c.T = st->T; c.F = st->F; c.C = st->C; c.Tq = Tq; c.k = k; c.kind = kind;
    c.has_thresh = has_thresh != 0; c.neighbors = neighbors; c.has_sample = sample;
    c.ld_q = ld; c.ld_out = ld_out; c.lds_max = ctx->lds_max; c.cu_count = ctx->cu_count;
    c.has_xs = st->xs != nullptr; c.has_yx = st->yx != nullptr; c.has_ybar = st->ybar != nullptr; c.has_ps = st->ps != nullptr;
    c.has_pq = st->pq != nullptr; c.has_rx = st->rx != nullptr;
    return c;
}

int predict_common(int mode, sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t ld, int64_t Tq, int k,
                   int kind, int has_thresh, double thresh, const int32_t* sample_dev, int64_t ld_s, double* out,
                   int64_t ld_out, int64_t* inds, double* dist, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq && out, "sd_analog_predict: NULL argument");
    const AnalogDevSwitches dev = sd_analog_dev_switches();
    const AnalogCall call = predict_call(mode, ctx, st, ld, Tq, k, kind, has_thresh, sample_dev != nullptr, ld_out, inds || dist);
    const AnalogPlan pl = analog_plan(call, dev);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    const int64_t C = st->C, T = st->T;
    const int F = st->F;
    sd_scratch status_p, sc_d, sc_i, status_pub;
    SD_TRY(sd_status_scratch(ctx, status_p, C));
    SD_HIP(sc_d.alloc(ctx, sizeof(double) * (size_t)pl.nb * k * pl.nthr));
    SD_HIP(sc_i.alloc(ctx, sizeof(int32_t) * (size_t)pl.nb * k * pl.nthr));
    int32_t* sp = status_p.as<int32_t>();
    const PredictArgs pa = predict_args(pl, k, has_thresh, thresh, sample_dev, ld_s, out, ld_out, inds, dist, sp);
    switch (pl.path) {
        case AnalogPath::Mean3:
        case AnalogPath::Mean:
        case AnalogPath::Window: SD_TRY(predict_staged(ctx, mode, st, pl, dev, Xq, ld, Tq, pa, sp, sc_d.as<double>(), sc_i.as<int32_t>())); break;
        case AnalogPath::Walk: {
            const AnalogLaunch L = analog_launches::per_cell(pl, C);
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_f1_predict_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
            SD_LAUNCH(ctx, "analog_f1_predict_kernel", analog_f1_predict_kernel, grid_of(L), dim3(L.block), L.lds, mode, Xq, ld, Tq, T, C,
                      (const double*)st->xs, (const int32_t*)st->xi, (const double*)st->X, (const double*)st->y, (const int32_t*)st->status, sp,
                      sc_d.as<double>(), sc_i.as<int32_t>(), pa);
            break;
        }
        case AnalogPath::Slab: SD_TRY(predict_slab(ctx, mode, st, call, pl, Xq, ld, sp, pa, dev.count)); break;
        case AnalogPath::Bf2:
            switch (F) {
                case 1: SD_TRY(launch_bf2<1>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 2: SD_TRY(launch_bf2<2>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 3: SD_TRY(launch_bf2<3>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 4: SD_TRY(launch_bf2<4>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 5: SD_TRY(launch_bf2<5>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 6: SD_TRY(launch_bf2<6>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                case 7: SD_TRY(launch_bf2<7>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
                default: SD_TRY(launch_bf2<8>(ctx, mode, st, Xq, ld, Tq, sp, pa, pl)); break;
            }
            break;
        default: {  // AnalogPath::Bf
            const AnalogLaunch L = analog_launches::per_cell(pl, C);
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_bf_predict_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
            SD_LAUNCH(ctx, "analog_bf_predict_kernel", analog_bf_predict_kernel, grid_of(L), dim3(L.block), L.lds, mode, Xq, ld, Tq, T, F, C,
                      (const double*)st->X, (const double*)st->y, (const int32_t*)st->status, sp, sc_d.as<double>(), sc_i.as<int32_t>(), pa);
            break;
        }
    }
    if (cell_status) SD_TRY(publish_status(ctx, (const int32_t*)st->status, sp, C, &status_pub, cell_status));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

int predict_host(int mode, sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t Tq, int k, int kind,
                 int has_thresh, double thresh, const int32_t* sample, double* out, int64_t* inds, double* dist,
                 int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq && out, "sd_analog_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0 && k >= 1, "sd_analog_predict: bad sizes");
    const int64_t C = st->C;
    const size_t cells = (size_t)Tq * C;
    const sd_host_field f[] = {sd_in(Xq, sizeof(double) * cells * st->F), sd_in(sample, sizeof(int32_t) * cells), sd_out(out, sizeof(double) * cells * 3),
                               sd_out(inds, sizeof(int64_t) * cells * k), sd_out(dist, sizeof(double) * cells * k)};  // (sample, inds, dist may be NULL)
    return with_device_copies(ctx, f, [&](void* const* d) {
        return predict_common(mode, ctx, st, (const double*)d[0], C, Tq, k, kind, has_thresh, thresh, (const int32_t*)d[1], C, (double*)d[2], C,
                              (int64_t*)d[3], (double*)d[4], cell_status);
    });
}

// columns `list[0 .. nw)` of a [R, ld] field <-> a packed [R, nw] field (cells the fused kernel handed back)
__global__ void __launch_bounds__(256) analog_gather_cells_kernel(const double* __restrict__ src, int64_t ld, int64_t R,
                                                                  const int32_t* __restrict__ list, int64_t nw,
                                                                  double* __restrict__ dst) {
    const int64_t total = R * nw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / nw, j = i - r * nw;
        dst[i] = src[r * ld + list[j]];
    }
}
__global__ void __launch_bounds__(256) analog_scatter_cells_kernel(const double* __restrict__ src, int64_t R,
                                                                   const int32_t* __restrict__ list, int64_t nw,
                                                                   double* __restrict__ dst, int64_t ld) {
    const int64_t total = R * nw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / nw, j = i - r * nw;
        dst[r * ld + list[j]] = src[i];
    }
}

template <int K>
int launch_fused_k(sd_ctx* ctx, const AnalogLaunch& L, const double* runs, int np, const int32_t* odd, const double* Xc, const double* yc,
                   const double* qc, int64_t Tq, int64_t T, int64_t cc, const int32_t* st_fit, int32_t* st_p, int32_t* worklist,
                   int32_t* work_count, int64_t cell0, const PredictArgs& pw, int skip_prob) {
    SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&analog_f1_fused_kernel<K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    SD_LAUNCH(ctx, "analog_f1_fused_kernel", analog_f1_fused_kernel<K>, grid_of(L), dim3(L.block), L.lds, runs, np, odd, Xc, yc, qc, Tq, T, cc, st_fit,
              st_p, worklist, work_count, cell0, pw, skip_prob);
    return SD_OK;
}

// the split path on device fields: fit -> predict -> drop the state
int fit_predict_split(sd_ctx* ctx, const double* X, const double* y, int64_t ld, int64_t T, int F, int64_t C, const double* Xq,
                      int64_t ld_q, int64_t Tq, int k, int kind, int has_thresh, double thresh, double* out, int64_t ld_out,
                      int32_t* cell_status) {
    sd_analog_state* st = nullptr;
    SD_TRY(sd_analog_fit_dev(ctx, X, y, ld, T, F, C, &st));
    const int rc = predict_common(0, ctx, st, Xq, ld_q, Tq, k, kind, has_thresh, thresh, nullptr, 0, out, ld_out, nullptr, nullptr, cell_status);
    sd_analog_state_destroy(st);
    return rc;
}

// cells the fused kernel handed back (ties among the training values or on a window boundary), fewer than half of the grid: the
// split path answers them on packed copies of their columns (the same numbers as in place), and what it finds for the cells it
// recomputes replaces what the fused pass reported for them
int fit_predict_handbacks(sd_ctx* ctx, const int32_t* worklist, int32_t nw, const double* X, const double* y, int64_t ld, int64_t T,
                          const double* Xq, int64_t ld_q, int64_t Tq, int k, int kind, int has_thresh, double thresh, double* out, int64_t ld_out,
                          int32_t* cell_status) {
    sd_scratch Xw, yw, Qw, Ow;
    SD_HIP(Xw.alloc(ctx, sizeof(double) * (size_t)T * nw));
    SD_HIP(yw.alloc(ctx, sizeof(double) * (size_t)T * nw));
    SD_HIP(Qw.alloc(ctx, sizeof(double) * (size_t)Tq * nw));
    SD_HIP(Ow.alloc(ctx, sizeof(double) * (size_t)Tq * 3 * nw));
    auto blocks = [&](int64_t total) { return dim3((unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->cu_count * 16)); };
    SD_LAUNCH(ctx, "analog_gather_cells_kernel", analog_gather_cells_kernel, blocks(T * nw), dim3(256), 0, X, ld, T, worklist, (int64_t)nw, Xw.as<double>());
    SD_LAUNCH(ctx, "analog_gather_cells_kernel", analog_gather_cells_kernel, blocks(T * nw), dim3(256), 0, y, ld, T, worklist, (int64_t)nw, yw.as<double>());
    SD_LAUNCH(ctx, "analog_gather_cells_kernel", analog_gather_cells_kernel, blocks(Tq * nw), dim3(256), 0, Xq, ld_q, Tq, worklist, (int64_t)nw, Qw.as<double>());
    std::vector<int32_t> st_w((size_t)nw), cells_w((size_t)nw);
    SD_TRY(fit_predict_split(ctx, Xw.as<double>(), yw.as<double>(), nw, T, 1, nw, Qw.as<double>(), nw, Tq, k, kind, has_thresh, thresh, Ow.as<double>(), nw,
                             cell_status ? st_w.data() : nullptr));
    SD_LAUNCH(ctx, "analog_scatter_cells_kernel", analog_scatter_cells_kernel, blocks(3 * Tq * nw), dim3(256), 0, (const double*)Ow.p, 3 * Tq, worklist,
              (int64_t)nw, out, ld_out);
    if (cell_status) SD_HIP(hipMemcpyAsync(cells_w.data(), worklist, sizeof(int32_t) * (size_t)nw, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    if (cell_status)  // the recomputed cells report what the split path found for them
        for (int32_t j = 0; j < nw; ++j) cell_status[cells_w[(size_t)j]] = st_w[(size_t)j];
    return SD_OK;
}

int fit_predict_dev(sd_ctx* ctx, const double* X, const double* y, int64_t ld, int64_t T, int F, int64_t C, const double* Xq,
                    int64_t ld_q, int64_t Tq, int k, int kind, int has_thresh, double thresh, double* out, int64_t ld_out,
                    int32_t* cell_status) {
    SD_CHECK_ARG(ctx && X && y && Xq && out, "sd_analog_fit_predict: NULL argument");
    const AnalogDevSwitches dev = sd_analog_dev_switches();
    AnalogCall call;
    call.op = AnalogOp::FitPredict;
    call.T = T; call.F = F; call.C = C; call.Tq = Tq; call.k = k; call.kind = kind; call.has_thresh = has_thresh != 0;
    call.ld = ld; call.ld_q = ld_q; call.ld_out = ld_out;
    call.lds_max = ctx->lds_max; call.cu_count = ctx->cu_count;
    const AnalogPlan pl = analog_plan(call, dev);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    kind = pl.kind;  // (k == 1 is 'best_analog', as in predict_common: gard.py:291-296)
    if (pl.path == AnalogPath::Split) return fit_predict_split(ctx, X, y, ld, T, F, C, Xq, ld_q, Tq, k, kind, has_thresh, thresh, out, ld_out, cell_status);

    const int np = pl.np_runs;
    sd_scratch Xc, yc, runs, st_fit, st_p, odd, list, status_pub;
    QueryStaging qs;
    SD_HIP(Xc.alloc(ctx, sizeof(double) * (size_t)T * C));
    SD_HIP(yc.alloc(ctx, sizeof(double) * (size_t)T * C));
    SD_HIP(runs.alloc(ctx, sizeof(double) * (size_t)np * C));
    SD_HIP(st_fit.alloc(ctx, sizeof(int32_t) * (size_t)C));
    SD_HIP(st_p.alloc(ctx, sizeof(int32_t) * (size_t)C));
    SD_HIP(odd.alloc(ctx, sizeof(int32_t) * (size_t)C));
    SD_HIP(list.alloc(ctx, sizeof(int32_t) * (size_t)(C + 1)));
    SD_TRY(qs.alloc(ctx, pl, Tq, C));
    const PredictArgs pa = predict_args(pl, k, has_thresh, thresh, nullptr, 0, out, ld_out, nullptr, nullptr, st_p.as<int32_t>());
    int32_t* work_count = list.as<int32_t>();
    int32_t* worklist = work_count + 1;
    SD_HIP(hipMemsetAsync(st_fit.p, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
    SD_HIP(hipMemsetAsync(st_p.p, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
    SD_HIP(hipMemsetAsync(odd.p, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
    SD_HIP(hipMemsetAsync(work_count, 0, sizeof(int32_t), ctx->stream));
    SD_TRY(launch_tile_sort(ctx, pl.K, X, y, ld, T, C, Xc.as<double>(), yc.as<double>(), runs.as<double>(), np, st_fit.as<int32_t>(), odd.as<int32_t>()));
    for (int64_t cb = 0; cb < C; cb += pl.chunk) {
        const int64_t cc = C - cb < pl.chunk ? C - cb : pl.chunk;
        SD_TRY(qs.in(ctx, pl, Xq + cb, ld_q, Tq, cc, st_p.as<int32_t>() + cb));
        const PredictArgs pw = staged(pa, qs.oc.as<double>(), Tq, 0);  // (the fused kernel takes skip_prob as an argument of its own)
        const AnalogLaunch L = analog_launches::per_cell(pl, cc);
        const double* r = runs.as<double>() + cb * (int64_t)np;
        const double* xc = Xc.as<double>() + cb * T;
        const double* yy = yc.as<double>() + cb * T;
        const int32_t* sf = st_fit.as<int32_t>() + cb;
        int32_t* sp = st_p.as<int32_t>() + cb;
        const int32_t* od = odd.as<int32_t>() + cb;
        const double* qc = qs.qc.as<double>();
        switch (pl.K) {
            case 13: SD_TRY(launch_fused_k<13>(ctx, L, r, np, od, xc, yy, qc, Tq, T, cc, sf, sp, worklist, work_count, cb, pw, pl.skip_prob)); break;
            case 15: SD_TRY(launch_fused_k<15>(ctx, L, r, np, od, xc, yy, qc, Tq, T, cc, sf, sp, worklist, work_count, cb, pw, pl.skip_prob)); break;
            default: SD_TRY(launch_fused_k<17>(ctx, L, r, np, od, xc, yy, qc, Tq, T, cc, sf, sp, worklist, work_count, cb, pw, pl.skip_prob)); break;
        }
        SD_TRY(qs.out(ctx, pl, Tq, cc, out + cb, ld_out));
    }
    int32_t nw = 0;
    SD_HIP(hipMemcpyAsync(&nw, work_count, sizeof(nw), hipMemcpyDeviceToHost, ctx->stream));
    if (cell_status) SD_TRY(publish_status(ctx, st_fit.as<int32_t>(), st_p.as<int32_t>(), C, &status_pub, cell_status));
    SD_HIP(hipStreamSynchronize(ctx->stream));
#ifdef SD_DEV
    if (dev.count) fprintf(stderr, "analog fit_predict: %d of %lld cells handed back to the split path\n", nw, (long long)C);
    if (dev.fused_trace) {  // phase clocks (100 MHz ticks of s_memtime) of the first cells of workgroup 0, last chunk
        long long h[128];
        SD_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(sd_fused_trace), sizeof(h)));
        for (int r = 0; r < 8; ++r) {
            fprintf(stderr, "fused trace cell %d: runs %lld merge %lld tags+xs %lld search %lld yx %lld prefix %lld outputs %lld (means %lld, prefix of squares %lld, barrier %lld, spreads + stores %lld)\n", r, h[r * 16 + 1] - h[r * 16],
                    h[r * 16 + 2] - h[r * 16 + 1], h[r * 16 + 3] - h[r * 16 + 2], h[r * 16 + 4] - h[r * 16 + 3], h[r * 16 + 5] - h[r * 16 + 4],
                    h[r * 16 + 6] - h[r * 16 + 5], h[r * 16 + 7] - h[r * 16 + 6], h[r * 16 + 8] - h[r * 16 + 6], h[r * 16 + 9] - h[r * 16 + 8],
                    h[r * 16 + 10] - h[r * 16 + 9], h[r * 16 + 7] - h[r * 16 + 10]);
        }
    }
#endif
    if (nw == 0) return SD_OK;
    // few cells handed back: on packed copies of their columns; many: the whole grid in place (the same numbers either way)
    if (analog_handback_whole_grid(nw, C)) return fit_predict_split(ctx, X, y, ld, T, F, C, Xq, ld_q, Tq, k, kind, has_thresh, thresh, out, ld_out, cell_status);
    return fit_predict_handbacks(ctx, worklist, nw, X, y, ld, T, Xq, ld_q, Tq, k, kind, has_thresh, thresh, out, ld_out, cell_status);
}

}  // namespace

extern "C" {

int sd_analog_state_destroy(sd_analog_state* st) { return sd_state_destroy(st, analog_bufs); }

int sd_analog_state_info(const sd_analog_state* st, int64_t* T, int* F, int64_t* C) {
    SD_CHECK_ARG(st, "state is NULL");
    if (T) *T = st->T;
    if (F) *F = st->F;
    if (C) *C = st->C;
    return SD_OK;
}

int sd_analog_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                      sd_analog_state** out) {
    SD_CHECK_ARG(ctx && X_dev && y_dev && out, "sd_analog_fit: NULL argument");
    const AnalogDevSwitches dev = sd_analog_dev_switches();
    AnalogCall call;
    call.op = AnalogOp::Fit;
    call.T = T; call.F = F; call.C = C; call.ld = ld; call.lds_max = ctx->lds_max; call.cu_count = ctx->cu_count;
    AnalogPlan pl = analog_plan(call, dev);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_analog_state* st = new sd_analog_state();
    st->ctx = ctx;
    st->T = T;
    st->F = F;
    st->C = C;
    return sd_state_build(st, sd_analog_state_destroy, out, [&]() -> int {
        SD_TRY(analog_alloc(ctx, st, {kX, kY, kStatus}));
        sd_scratch runs_buf, odd_buf;
        if (pl.tiled && runs_buf.alloc(ctx, sizeof(double) * (size_t)pl.np_runs * (size_t)C) != hipSuccess) {
            (void)hipGetLastError();  // no room for the presorted runs: the plan with the two transposes
            AnalogDevSwitches no_tile = dev;
            no_tile.no_tile = true;
            pl = analog_plan(call, no_tile);
        }
        if (pl.tiled) {
            // F == 1: one tile-shaped kernel makes the cell-major copies and the sorted runs of 64 * K keys (csrc: analog_tile_sort_kernel)
            SD_HIP(odd_buf.alloc(ctx, sizeof(int32_t) * (size_t)C));
            SD_HIP(hipMemsetAsync(odd_buf.p, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
            SD_TRY(launch_tile_sort(ctx, pl.K, X_dev, y_dev, ld, T, C, st->X, st->y, runs_buf.as<double>(), pl.np_runs, st->status,
                                    odd_buf.as<int32_t>()));
        } else {
            const AnalogLaunch L = analog_launches::transpose(C, T);
            for (int f = 0; f < F; ++f)
                SD_LAUNCH(ctx, "analog_transpose_kernel", analog_transpose_kernel, grid_of(L), dim3(L.block), 0, X_dev, ld, T, F, f, C,
                          st->X, st->status, 1);
            SD_LAUNCH(ctx, "analog_transpose_kernel", analog_transpose_kernel, grid_of(L), dim3(L.block), 0, y_dev, ld, T, 1, 0, C,
                      st->y, st->status, 0);
        }
        if (pl.sorted) {
            // sorted view for the 1-D fast path: values, original indices, and y in the same order
            // (no prefix sums yet: the BASELINE path -- analog_f1_mean3_kernel -- builds its own on chip; the kernels
            // that read them from memory get them from build_prefix_sums on their first call)
            SD_TRY(analog_alloc(ctx, st, {kXs, kXi, kYx, kYbar}));
            Sort2Args a{st->X, T, 0, st->y, T, C, st->xs, st->xi, st->yx, nullptr, st->ybar};
            if (pl.tiled) {
                a.runs = runs_buf.as<double>();
                a.np_runs = pl.np_runs;
                a.odd_flags = odd_buf.as<int32_t>();
            }
            a.tagged = pl.tagged;
            a.count = dev.count;
            SD_TRY(launch_sort2_width(ctx, pl.K, a));
            SD_HIP(hipStreamSynchronize(ctx->stream));
        }
        if (pl.Ks != 0) {
            // F > 1: training points in feature-0 order for the slab search (analog_slab_predict_kernel)
            const AnalogLaunch L = analog_launches::gather_sorted(C, ctx->cu_count);
            sd_scratch keys;
            SD_HIP(keys.alloc(ctx, sizeof(double) * (size_t)T * C));
            SD_TRY(analog_alloc(ctx, st, {kXi, kPs}));
            Sort2Args a{st->X, (int64_t)F * T, 1, nullptr, T, C, keys.as<double>(), st->xi, nullptr, nullptr, nullptr};
            a.tagged = pl.tagged;
            a.count = dev.count;
            SD_TRY(launch_sort2_width(ctx, pl.Ks, a));
            SD_LAUNCH(ctx, "analog_gather_sorted_kernel", analog_gather_sorted_kernel, grid_of(L), dim3(L.block), 0, (const double*)st->X,
                      (const int32_t*)st->xi, T, F, C, st->ps);
            SD_HIP(hipStreamSynchronize(ctx->stream));
        }
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_analog_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, sd_analog_state** out) {
    SD_CHECK_ARG(ctx && X && y && out, "sd_analog_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && F >= 1, "sd_analog_fit: bad sizes");
    const sd_host_field f[] = {sd_in(X, sizeof(double) * (size_t)T * F * C), sd_in(y, sizeof(double) * (size_t)T * C)};
    return with_device_copies(ctx, f, [&](void* const* d) { return sd_analog_fit_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, F, C, out); });
}

int sd_analog_predict_dev(sd_ctx* ctx, const sd_analog_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, int k,
                          int kind, int has_thresh, double thresh, const int32_t* sample_inds_dev, double* out_dev,
                          int64_t ld_out, int64_t* inds_dev, double* dist_dev, int32_t* cell_status) {
    return predict_common(0, ctx, st, Xq_dev, ld, Tq, k, kind, has_thresh, thresh, sample_inds_dev, ld, out_dev, ld_out,
                          inds_dev, dist_dev, cell_status);
}

int sd_analog_predict(sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t Tq, int k, int kind,
                      int has_thresh, double thresh, const int32_t* sample_inds, double* out, int64_t* inds,
                      double* dist, int32_t* cell_status) {
    return predict_host(0, ctx, st, Xq, Tq, k, kind, has_thresh, thresh, sample_inds, out, inds, dist, cell_status);
}

int sd_analog_fit_predict_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                              const double* Xq_dev, int64_t ld_q, int64_t Tq, int k, int kind, int has_thresh, double thresh,
                              double* out_dev, int64_t ld_out, int32_t* cell_status) {
    return fit_predict_dev(ctx, X_dev, y_dev, ld, T, F, C, Xq_dev, ld_q, Tq, k, kind, has_thresh, thresh, out_dev, ld_out, cell_status);
}

int sd_analog_fit_predict(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, const double* Xq, int64_t Tq, int k,
                          int kind, int has_thresh, double thresh, double* out, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && X && y && Xq && out, "sd_analog_fit_predict: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && Tq > 0 && F >= 1, "sd_analog_fit_predict: bad sizes");
    const sd_host_field f[] = {sd_in(X, sizeof(double) * (size_t)T * F * C), sd_in(y, sizeof(double) * (size_t)T * C),
                               sd_in(Xq, sizeof(double) * (size_t)Tq * F * C), sd_out(out, sizeof(double) * (size_t)Tq * 3 * C)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return fit_predict_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, F, C, (const double*)d[2], C, Tq, k, kind, has_thresh, thresh,
                               (double*)d[3], C, cell_status);
    });
}

int sd_analogreg_predict_dev(sd_ctx* ctx, const sd_analog_state* st, const double* Xq_dev, int64_t ld, int64_t Tq,
                             int k, int has_thresh, double thresh, double* out_dev, int64_t ld_out, int32_t* cell_status) {
    return predict_common(1, ctx, st, Xq_dev, ld, Tq, k, SD_ANALOG_MEAN, has_thresh ? 1 : 0, thresh, nullptr, ld, out_dev, ld_out, nullptr,
                          nullptr, cell_status);
}

int sd_analogreg_predict(sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t Tq, int k, int has_thresh, double thresh,
                         double* out, int32_t* cell_status) {
    return predict_host(1, ctx, st, Xq, Tq, k, SD_ANALOG_MEAN, has_thresh ? 1 : 0, thresh, nullptr, out, nullptr, nullptr, cell_status);
}

}  // extern "C"
