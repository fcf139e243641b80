// GroupedRegressor(LinearRegression, PaddedDOYGrouper, ...) of the reference (grouping.py:12-138), batched over the cell
// axis: per cell one least-squares model per group g of [0, n), fitted on the samples whose key lies in the circular window
// {g - window .. g + window} (mod n), and a prediction that picks the model of each sample's own key.  window = 0 is a plain
// disjoint grouped regression (one model per month, per season, ...).
//
// fit, two kernels; X and y are read once:
//   grouped_day_kernel     one wave per (64 adjacent cells, key): walks the key's time steps (host table ordered by key) and
//                          sums the data shifted by the cell's first sample: sum x_f, sum y, sum x_f x_g (g >= f), sum x_f y.
//                          Every load is a 512-byte row fragment.  Result: part [nstat][n][C].
//   grouped_window_kernel  a workgroup owns `cells` adjacent cells and a run of consecutive groups (sd_grouped_plan.h): the
//                          statistics of the run's keys are staged in LDS once, every group re-adds the keys of its window
//                          from there in window order (no sliding add / subtract: nothing accumulates), centres the sums and
//                          solves with sdlsq::minnorm_solve like linreg_fit_kernel does for a whole series.
// predict, one kernel: one wave per (64 cells, key) loads the key's model once and walks the key's time steps.
#include <algorithm>
#include <vector>

#include "sd_grouped_plan.h"
#include "sd_internal.h"
#include "sd_lsq.h"
#include "sd_state.h"

struct sd_grouped_state {
    sd_ctx* ctx = nullptr;
    int64_t C = 0;
    int n = 0, F = 0, window = 0;
    double* coef = nullptr;        // device [n][F][C]
    double* intercept = nullptr;   // device [n][C]
    int32_t* status = nullptr;     // device [C] internal bitmask
    std::vector<int32_t> fitted;   // host [n]: 1 = the group's window held a sample
};

namespace {

constexpr int kMaxF = sdlsq::kMaxF;
constexpr int kCells = 64;
constexpr int kKeysPerBlock = 4;  // waves of a day / predict workgroup, one key each
constexpr int kUnroll = 4;        // time steps of a thread whose loads are in flight together

__device__ __forceinline__ bool gr_finite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

template <int F>
struct Stat {  // positions in the statistics vector of one (cell, key)
    static constexpr int kSx = 0, kSy = F, kSxx = F + 1, kSxy = F + 1 + F * (F + 1) / 2, kN = kSxy + F;
};

template <int F>
__global__ void __launch_bounds__(kCells * kKeysPerBlock) grouped_day_kernel(const double* __restrict__ X, const double* __restrict__ y,
                                                                             int64_t ld, int64_t C, int n,
                                                                             const int32_t* __restrict__ order,
                                                                             const int64_t* __restrict__ off, double* __restrict__ part,
                                                                             int32_t* __restrict__ status) {
    using S = Stat<F>;
    const int cx = threadIdx.x % kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const int d = blockIdx.y * kKeysPerBlock + threadIdx.x / kCells;
    if (c >= C || d >= n) return;
    double x0[F], acc[S::kN];
#pragma unroll
    for (int f = 0; f < F; ++f) x0[f] = X[(int64_t)f * ld + c];
    const double y0 = y[c];
#pragma unroll
    for (int q = 0; q < S::kN; ++q) acc[q] = 0.0;
    bool bad = false;
    const int64_t i1 = off[d + 1];
    for (int64_t i = off[d]; i < i1; i += kUnroll) {
        double wv[kUnroll], xv[kUnroll][F];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool ok = i + u < i1;
            const int64_t t = ok ? order[i + u] : 0;
            wv[u] = ok ? y[t * ld + c] : y0;
#pragma unroll
            for (int f = 0; f < F; ++f) xv[u][f] = ok ? X[(t * F + f) * ld + c] : x0[f];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (i + u >= i1) break;
            double dx[F];
            const double e = wv[u] - y0;
            bad |= !gr_finite(wv[u]);
            acc[S::kSy] += e;
            int q = S::kSxx;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                bad |= !gr_finite(xv[u][f]);
                dx[f] = xv[u][f] - x0[f];
            }
#pragma unroll
            for (int f = 0; f < F; ++f) {
                acc[S::kSx + f] += dx[f];
                acc[S::kSxy + f] += dx[f] * e;
#pragma unroll
                for (int g = f; g < F; ++g) acc[q++] += dx[f] * dx[g];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < S::kN; ++q) part[((int64_t)q * n + d) * C + c] = acc[q];
    if (d == 0 && x0[0] != x0[0]) atomicOr(&status[c], SDI_MASKED);  // core.py:35-37: the cell's first sample is NaN
    if (bad) atomicOr(&status[c], SDI_NONFINITE);                    // base.py:18-20
}

template <int F>
__global__ void __launch_bounds__(kGroupedThreads) grouped_window_kernel(const double* __restrict__ part, const double* __restrict__ cnt,
                                                                         const double* __restrict__ X, const double* __restrict__ y,
                                                                         int64_t ld, int64_t C, int n, int window, int cells, int run,
                                                                         int slots, const int32_t* __restrict__ status,
                                                                         double* __restrict__ coef_out, double* __restrict__ icpt_out) {
    using S = Stat<F>;
    extern __shared__ double staged[];  // [slots][kN][cells]: slot s holds key (g0 - window + s) mod n
    const int cx = threadIdx.x % cells, gs = threadIdx.x / cells, slices = kGroupedThreads / cells;
    const int64_t c = (int64_t)blockIdx.x * cells + cx;
    const int g0 = blockIdx.y * run, g1 = min(g0 + run, n);
    const bool live = c < C;
    for (int r = gs; r < slots * S::kN; r += slices) {
        const int slot = r / S::kN, q = r - slot * S::kN;
        int d = (g0 - window + slot) % n;
        if (d < 0) d += n;
        staged[(int64_t)r * cells + cx] = live ? part[((int64_t)q * n + d) * C + c] : 0.0;
    }
    __syncthreads();
    if (!live) return;
    const bool ok = status[c] == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double x0[F];
#pragma unroll
    for (int f = 0; f < F; ++f) x0[f] = X[(int64_t)f * ld + c];
    const double y0 = y[c];
    const int W = min(2 * window + 1, n);
    for (int g = g0 + gs; g < g1; g += slices) {
        double acc[S::kN], cn = 0.0;
#pragma unroll
        for (int q = 0; q < S::kN; ++q) acc[q] = 0.0;
        for (int j = 0; j < W; ++j) {
            int d = g - window + j, slot = g - g0 + j;
            d += d < 0 ? n : 0;
            d -= d >= n ? n : 0;
            slot -= slot >= n ? n : 0;  // (only a run that holds every key wraps)
            cn += cnt[d];
            const double* sp = staged + (int64_t)slot * S::kN * cells + cx;
#pragma unroll
            for (int q = 0; q < S::kN; ++q) acc[q] += sp[q * cells];
        }
        double coef[kMaxF], icpt = nan;
        const bool fit = ok && cn > 0.0;
        if (fit) {
            double dm[F], raw[F], A[kMaxF][kMaxF + 1];
            const double em = acc[S::kSy] / cn;
#pragma unroll
            for (int f = 0; f < F; ++f) dm[f] = acc[S::kSx + f] / cn;
            int q = S::kSxx;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                A[f][F] = acc[S::kSxy + f] - cn * dm[f] * em;  // centred: sum d e - n mean(d) mean(e)
#pragma unroll
                for (int h = f; h < F; ++h) {
                    if (h == f) raw[f] = acc[q];
                    const double v = acc[q++] - cn * dm[f] * dm[h];
                    A[f][h] = v;
                    A[h][f] = v;
                }
            }
            sdlsq::clear_unresolved(F, A, raw, cn);  // a feature that is constant over the window's samples
            sdlsq::minnorm_solve(F, A, coef);
            icpt = y0 + em;
#pragma unroll
            for (int f = 0; f < F; ++f) icpt -= (x0[f] + dm[f]) * coef[f];
        }
#pragma unroll
        for (int f = 0; f < F; ++f) coef_out[((int64_t)g * F + f) * C + c] = fit ? coef[f] : nan;
        icpt_out[(int64_t)g * C + c] = icpt;
    }
}

template <int F>
__global__ void __launch_bounds__(kCells * kKeysPerBlock) grouped_predict_kernel(const double* __restrict__ Xq, int64_t ld, int64_t C, int n,
                                                                                 const int32_t* __restrict__ order,
                                                                                 const int64_t* __restrict__ off,
                                                                                 const double* __restrict__ coef,
                                                                                 const double* __restrict__ icpt_all,
                                                                                 const int32_t* __restrict__ fit_status,
                                                                                 int32_t* __restrict__ status, double* __restrict__ out,
                                                                                 int64_t ld_out) {
    const int cx = threadIdx.x % kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const int k = blockIdx.y * kKeysPerBlock + threadIdx.x / kCells;
    if (c >= C || k >= n) return;
    const int64_t i0 = off[k], i1 = off[k + 1];
    if (i0 == i1) return;
    const bool active = fit_status[c] == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double cf[F];
#pragma unroll
    for (int f = 0; f < F; ++f) cf[f] = coef[((int64_t)k * F + f) * C + c];
    const double icpt = icpt_all[(int64_t)k * C + c];
    bool bad = false;
    for (int64_t i = i0; i < i1; i += kUnroll) {
        double xv[kUnroll][F];
        int64_t tv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool ok = i + u < i1;
            tv[u] = ok ? order[i + u] : 0;
#pragma unroll
            for (int f = 0; f < F; ++f) xv[u][f] = ok ? Xq[(tv[u] * F + f) * ld + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (i + u >= i1) break;
            double p = icpt;
            bool fin = true;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                fin = fin && gr_finite(xv[u][f]);
                p += xv[u][f] * cf[f];
            }
            bad |= !fin;
            out[tv[u] * ld_out + c] = active && fin ? p : nan;
        }
    }
    if (active && bad) atomicOr(&status[c], SDI_NONFINITE);
}

template <int F>
int launch_fit(sd_ctx* ctx, const double* X, const double* y, int64_t ld, sd_grouped_state* st, const GroupedWindowTile& tile,
               const int32_t* order, const int64_t* off, const double* cnt, double* part) {
    const int n = st->n;
    const dim3 dgrid((unsigned)((st->C + kCells - 1) / kCells), (unsigned)((n + kKeysPerBlock - 1) / kKeysPerBlock));
    SD_LAUNCH(ctx, "grouped_day_kernel", grouped_day_kernel<F>, dgrid, dim3(kCells * kKeysPerBlock), 0, X, y, ld, st->C, n, order, off, part,
              st->status);
    if (tile.lds > ((size_t)64 << 10))
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&grouped_window_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)tile.lds));
    const dim3 wgrid((unsigned)((st->C + tile.cells - 1) / tile.cells), (unsigned)((n + tile.run - 1) / tile.run));
    SD_LAUNCH(ctx, "grouped_window_kernel", grouped_window_kernel<F>, wgrid, dim3(kGroupedThreads), tile.lds, (const double*)part, cnt, X, y,
              ld, st->C, n, st->window, tile.cells, tile.run, tile.slots, (const int32_t*)st->status, st->coef, st->intercept);
    return SD_OK;
}

template <int F>
int launch_predict(sd_ctx* ctx, const sd_grouped_state* st, const double* Xq, int64_t ld, const int32_t* order, const int64_t* off,
                   int32_t* status_p, double* out, int64_t ld_out) {
    const dim3 grid((unsigned)((st->C + kCells - 1) / kCells), (unsigned)((st->n + kKeysPerBlock - 1) / kKeysPerBlock));
    SD_LAUNCH(ctx, "grouped_predict_kernel", grouped_predict_kernel<F>, grid, dim3(kCells * kKeysPerBlock), 0, Xq, ld, st->C, st->n, order,
              off, (const double*)st->coef, (const double*)st->intercept, (const int32_t*)st->status, status_p, out, ld_out);
    return SD_OK;
}

std::vector<sd_buf> grouped_bufs(const sd_grouped_state* st) {
    const size_t plane = (size_t)st->n * st->C;
    return {sd_buf_of(st->coef, plane * st->F), sd_buf_of(st->intercept, plane), sd_buf_of(st->status, (size_t)st->C, true)};
}

sd_grouped_state* new_grouped(sd_ctx* ctx, int n, int F, int64_t C, int window) {
    sd_grouped_state* st = new sd_grouped_state();
    st->ctx = ctx; st->n = n; st->F = F; st->C = C; st->window = window;
    return st;
}

// the time steps of a predict call ordered by key; refuses a key without a fitted model, the smallest one first
int predict_table(const sd_grouped_state* st, const int32_t* key, int64_t Tq, GroupedKeyTable* tab) {
    SD_CHECK_ARG(Tq < ((int64_t)1 << 31), "sd_grouped_predict: Tq = %lld samples exceed the int32 sample index", (long long)Tq);
    int32_t missing = 0;
    bool have = false;
    for (int64_t t = 0; t < Tq; ++t) {
        const int32_t k = key[t];
        if (k >= 0 && k < st->n && st->fitted[(size_t)k]) continue;
        missing = have ? std::min(missing, k) : k;
        have = true;
    }
    if (have) return sd_set_error(SD_ERR_INVALID, "sd_grouped_predict: no fitted model for key %d", (int)missing);
    *tab = grouped_key_table(key, Tq, st->n);
    return SD_OK;
}

}  // namespace

extern "C" {

int sd_grouped_state_destroy(sd_grouped_state* st) { return sd_state_destroy(st, grouped_bufs); }

int sd_grouped_state_info(const sd_grouped_state* st, int* n, int* F, int64_t* C, int* window) {
    SD_CHECK_ARG(st, "state is NULL");
    if (n) *n = st->n;
    if (F) *F = st->F;
    if (C) *C = st->C;
    if (window) *window = st->window;
    return SD_OK;
}

int sd_grouped_state_export(const sd_grouped_state* st, double* coef, double* intercept, int32_t* fitted, int32_t* cell_status) {
    SD_CHECK_ARG(st, "state is NULL");
    sd_ctx* ctx = st->ctx;
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(sd_state_copy(ctx, grouped_bufs(st), {coef, intercept}, hipMemcpyDeviceToHost));
    if (fitted) std::copy(st->fitted.begin(), st->fitted.end(), fitted);
    return sd_status_fold(ctx, st->status, nullptr, st->C, cell_status);
}

// fitted numbers -> device state (pickling, checkpoint / resume)
int sd_grouped_state_import(sd_ctx* ctx, int n, int F, int64_t C, int window, const double* coef, const double* intercept,
                            const int32_t* fitted, const int32_t* cell_status, sd_grouped_state** out) {
    SD_CHECK_ARG(ctx && coef && intercept && fitted && out, "sd_grouped_state_import: NULL argument");
    SD_CHECK_ARG(n > 0 && C > 0 && F >= 1 && F <= kMaxF && window >= 0, "sd_grouped_state_import: bad sizes");
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_grouped_state* st = new_grouped(ctx, n, F, C, window);
    st->fitted.assign(fitted, fitted + n);
    const std::vector<int32_t> bits = sd_status_bits(cell_status, C);
    return sd_state_build(st, sd_grouped_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, grouped_bufs(st)));
        SD_TRY(sd_state_copy(ctx, grouped_bufs(st), {coef, intercept, bits.data()}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_grouped_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                       const int32_t* key, int n, int window, sd_grouped_state** out) {
    SD_CHECK_ARG(ctx && X_dev && y_dev && key && out, "sd_grouped_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && ld >= C && n > 0, "sd_grouped_fit: bad sizes");
    SD_CHECK_ARG(T < ((int64_t)1 << 31), "sd_grouped_fit: T = %lld samples exceed the int32 sample index", (long long)T);
    SD_CHECK_ARG(F >= 1 && F <= kMaxF, "sd_grouped_fit: F=%d outside [1,%d]", F, kMaxF);
    SD_CHECK_ARG(window >= 0 && window < n, "sd_grouped_fit: window=%d outside [0,%d): the circular window wraps once only", window, n);
    *out = nullptr;
    const GroupedKeyTable tab = grouped_key_table(key, T, n);
    if (tab.err != SD_OK) return sd_set_error(tab.err, "sd_grouped_fit: %s", tab.msg.c_str());
    const GroupedWindowTile tile = grouped_window_tile(F, n, window, ctx->lds_max);
    SD_CHECK_ARG(tile.cells > 0, "sd_grouped_fit: the statistics of a window=%d, F=%d group do not fit in LDS", window, F);
    SD_HIP(hipSetDevice(ctx->device));
    sd_grouped_state* st = new_grouped(ctx, n, F, C, window);
    st->fitted = grouped_fitted(tab.cnt, window);
    return sd_state_build(st, sd_grouped_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, grouped_bufs(st)));
        sd_scratch d_order, d_off, d_cnt, d_part;
        SD_TRY(upload(ctx, d_order, tab.order));
        SD_TRY(upload(ctx, d_off, tab.off));
        SD_TRY(upload(ctx, d_cnt, tab.cnt));
        SD_HIP(d_part.alloc(ctx, sizeof(double) * (size_t)grouped_nstat(F) * n * C));
        SD_DISPATCH_F(F, launch_fit, ctx, X_dev, y_dev, ld, st, tile, d_order.as<const int32_t>(), d_off.as<const int64_t>(),
                      d_cnt.as<const double>(), d_part.as<double>());
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch tables go back to the cache on return)
        return SD_OK;
    });
}

int sd_grouped_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, const int32_t* key, int n, int window,
                   sd_grouped_state** out) {
    SD_CHECK_ARG(ctx && X && y && out, "sd_grouped_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && F >= 1, "sd_grouped_fit: bad sizes");
    const size_t bytes = sizeof(double) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(X, bytes * F), sd_in(y, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_grouped_fit_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, F, C, key, n, window, out);
    });
}

int sd_grouped_predict_dev(sd_ctx* ctx, const sd_grouped_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, const int32_t* key,
                           double* out_dev, int64_t ld_out, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq_dev && key && out_dev, "sd_grouped_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0 && ld >= st->C && ld_out >= st->C, "sd_grouped_predict: bad sizes");
    GroupedKeyTable tab;
    SD_TRY(predict_table(st, key, Tq, &tab));
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch status_p, d_order, d_off;
    SD_TRY(sd_status_scratch(ctx, status_p, st->C));
    SD_TRY(upload(ctx, d_order, tab.order));
    SD_TRY(upload(ctx, d_off, tab.off));
    SD_DISPATCH_F(st->F, launch_predict, ctx, st, Xq_dev, ld, d_order.as<const int32_t>(), d_off.as<const int64_t>(),
                  status_p.as<int32_t>(), out_dev, ld_out);
    return sd_status_fold(ctx, st->status, status_p.as<int32_t>(), st->C, cell_status);
}

int sd_grouped_predict(sd_ctx* ctx, const sd_grouped_state* st, const double* Xq, int64_t Tq, const int32_t* key, double* out,
                       int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq && key && out, "sd_grouped_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0, "sd_grouped_predict: bad sizes");
    GroupedKeyTable tab;
    SD_TRY(predict_table(st, key, Tq, &tab));  // (before the upload: a missing key costs no transfer)
    const size_t bytes = sizeof(double) * (size_t)Tq * st->C;
    const sd_host_field f[] = {sd_in(Xq, bytes * st->F), sd_out(out, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_grouped_predict_dev(ctx, st, (const double*)d[0], st->C, Tq, key, (double*)d[1], st->C, cell_status);
    });
}

}  // extern "C"
