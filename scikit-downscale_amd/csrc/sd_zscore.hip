// ZScoreRegressor (zscore.py of the reference), batched over the cell axis.
//
// fit (zscore.py:32-69, 123-238): per cell the mean and population std of X and of y over every kept day window of the
// day-of-year grid (sd_zscore_plan.h), then shift = y_mean - X_mean and scale = y_std / X_std.  Two kernels:
//   zscore_day_kernel     one workgroup per (64 adjacent cells, day): its four waves split the years of the day and reduce
//                         through LDS, so every row fragment (512 B) is read once.  The samples are shifted by the day's
//                         first-year sample; the day's (mean, M2) are written to a [4][D][C] scratch.
//   zscore_window_kernel  one thread per (cell, run of kept windows): merges the w day partials of a window with the
//                         pairwise (Chan) update.  An all-identical window stays exactly (value, 0).
// predict (zscore.py:71-112, 241-319): pandas' centred rolling mean / std (ddof = 1, min_periods = w) of the series, the
// z score, and the fitted parameters expanded by position (entry t % min(Tp, 364)).
//   zscore_predict_kernel 64 adjacent cells x 4 time chunks per workgroup; a thread slides shifted window sums over its chunk
//                         (plus the w - 1 halo), re-based from the window's values every kRebase steps, and tracks the run
//                         of identical consecutive values: a window that is one run gets pandas' exact (value, 0).  A window
//                         whose spread is tiny against the shifted sums (kIllCond) is recomputed in two passes.
#include <algorithm>
#include <vector>

#include "sd_internal.h"
#include "sd_state.h"
#include "sd_zscore_plan.h"

struct sd_zscore_state {
    sd_ctx* ctx = nullptr;
    int64_t K = 0, C = 0;
    int w = 0;
    double* stats = nullptr;    // device [6][K][C]: X mean, X std, y mean, y std, shift, scale
    int32_t* status = nullptr;  // device [C] internal bitmask
};

namespace {

constexpr int kCells = 64;
constexpr int kDaySlices = 4;   // waves of a day workgroup
constexpr int kWinRun = 16;     // kept windows of one window-kernel thread
constexpr int kPredSlices = 4;  // time chunks of a predict workgroup
constexpr int kChunk = 512;     // outputs of one predict thread: the w - 1 halo is 6 % of the reads at w = 31
constexpr int kRebase = 32;     // predict: window sums recomputed from the window's values every kRebase steps
constexpr double kIllCond = 1e-6;  // predict: a window whose centred square sum is below this fraction of its shifted one is
                                   // recomputed in two passes (the sliding sums carry ~1e-14 of the shifted sum in error)

enum { ZS_XM = 0, ZS_XS, ZS_YM, ZS_YS, ZS_SHIFT, ZS_SCALE, ZS_NSTATS };

__device__ __forceinline__ bool zs_finite(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__global__ void __launch_bounds__(kCells * kDaySlices) zscore_day_kernel(const double* __restrict__ X, const double* __restrict__ y,
                                                                        int64_t ld, int64_t C, int D, const int32_t* __restrict__ order,
                                                                        const int64_t* __restrict__ off, double* __restrict__ part,
                                                                        int32_t* __restrict__ status) {
    __shared__ double red[4][kDaySlices][kCells];
    const int cx = threadIdx.x % kCells, s = threadIdx.x / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const int d = blockIdx.y;
    const bool live = c < C;
    const int64_t i0 = off[d], i1 = off[d + 1];
    double kx = 0.0, ky = 0.0, sx = 0.0, sxx = 0.0, sy = 0.0, syy = 0.0;
    bool bad = false;
    if (live) {
        const int64_t tf = order[i0];  // the day's first-year sample: the shift
        kx = X[tf * ld + c];
        ky = y[tf * ld + c];
        for (int64_t i = i0 + s; i < i1; i += kDaySlices) {
            const int64_t t = order[i];
            const double vx = X[t * ld + c], vy = y[t * ld + c];
            bad |= !(zs_finite(vx) && zs_finite(vy));
            const double dx = vx - kx, dy = vy - ky;
            sx += dx;
            sxx += dx * dx;
            sy += dy;
            syy += dy * dy;
        }
    }
    red[0][s][cx] = sx;
    red[1][s][cx] = sxx;
    red[2][s][cx] = sy;
    red[3][s][cx] = syy;
    __syncthreads();
    if (!live) return;
    const bool masked = X[c] != X[c];  // core.py:35-37: the cell's first sample is NaN
    if (s == 0) {
        double S[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < kDaySlices; ++j) a += red[q][j][cx];
            S[q] = a;
        }
        const double n = (double)(i1 - i0);
        const int64_t DC = (int64_t)D * C, at = (int64_t)d * C + c;
        part[0 * DC + at] = kx + S[0] / n;
        part[1 * DC + at] = fmax(S[1] - S[0] * (S[0] / n), 0.0);
        part[2 * DC + at] = ky + S[2] / n;
        part[3 * DC + at] = fmax(S[3] - S[2] * (S[2] / n), 0.0);
        if (masked && d == 0) atomicOr(&status[c], SDI_MASKED);
    }
    if (bad && !masked) atomicOr(&status[c], SDI_NONFINITE);  // base.py:18-20
}

__device__ __forceinline__ void chan_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
    const double n = na + nb, delta = mb - ma;
    ma = ma + delta * (nb / n);
    qa = qa + qb + delta * delta * (na * nb / n);
    na = n;
}

__global__ void __launch_bounds__(kCells) zscore_window_kernel(const double* __restrict__ part, int64_t C, int D, int K, int w,
                                                               const int32_t* __restrict__ win, const double* __restrict__ cnt,
                                                               const int32_t* __restrict__ status, double* __restrict__ stats) {
    const int64_t c = (int64_t)blockIdx.x * kCells + threadIdx.x;
    if (c >= C) return;
    const int k0 = blockIdx.y * kWinRun, k1 = min(k0 + kWinRun, K);
    const bool ok = status[c] == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t DC = (int64_t)D * C, KC = (int64_t)K * C;
    for (int k = k0; k < k1; ++k) {
        const int32_t* wd = win + (int64_t)k * w;
        int d = wd[0];
        double nx = cnt[d], mx = part[0 * DC + (int64_t)d * C + c], qx = part[1 * DC + (int64_t)d * C + c];
        double my = part[2 * DC + (int64_t)d * C + c], qy = part[3 * DC + (int64_t)d * C + c];
        double ny = nx;
        for (int j = 1; j < w; ++j) {
            d = wd[j];
            const double nb = cnt[d];
            const int64_t at = (int64_t)d * C + c;
            chan_merge(nx, mx, qx, nb, part[0 * DC + at], part[1 * DC + at]);
            chan_merge(ny, my, qy, nb, part[2 * DC + at], part[3 * DC + at]);
        }
        const double sx = sqrt(qx / nx), sy = sqrt(qy / ny);  // population std (ddof = 0)
        const int64_t at = (int64_t)k * C + c;
        stats[ZS_XM * KC + at] = ok ? mx : nan;
        stats[ZS_XS * KC + at] = ok ? sx : nan;
        stats[ZS_YM * KC + at] = ok ? my : nan;
        stats[ZS_YS * KC + at] = ok ? sy : nan;
        stats[ZS_SHIFT * KC + at] = ok ? my - mx : nan;  // zscore.py:237-238
        stats[ZS_SCALE * KC + at] = ok ? sy / sx : nan;
    }
}

__global__ void __launch_bounds__(kCells * kPredSlices) zscore_predict_kernel(
    const double* __restrict__ X, int64_t ld, int64_t Tp, int64_t C, int w, int P, const double* __restrict__ shift,
    const double* __restrict__ scale, const int32_t* __restrict__ fit_status, int32_t* __restrict__ status, double* __restrict__ out,
    int64_t ld_out, double* __restrict__ meani, double* __restrict__ stdi, double* __restrict__ meanf, double* __restrict__ stdf) {
    const int cx = threadIdx.x % kCells, s = threadIdx.x / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const int64_t t0 = ((int64_t)blockIdx.y * kPredSlices + s) * kChunk;
    if (c >= C || t0 >= Tp) return;
    const int64_t t1 = min(t0 + kChunk, Tp);
    const bool live = fit_status[c] == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double* xc = X + c;
    const int h0 = w / 2, h1 = (w - 1) / 2;  // pandas' centred window of t: [t - w/2, t + (w-1)/2]
    const double wd = (double)w;
    double A = 0.0, s1 = 0.0, s2 = 0.0, prev = 0.0;
    int run = 0, since = kRebase;
    bool bad = false;
    for (int64_t t = t0; t < t1; ++t) {
        const double xt = xc[t * ld];
        bad |= !zs_finite(xt);
        double mean = nan, sd = nan;
        if (t >= h0 && t + h1 < Tp) {
            const int64_t a = t - h0, b = t + h1;
            if (since >= kRebase) {  // sums of the window shifted by its first value, from scratch
                A = xc[a * ld];
                s1 = s2 = 0.0;
                run = 0;
                for (int64_t j = a; j <= b; ++j) {
                    const double v = xc[j * ld], dv = v - A;
                    s1 += dv;
                    s2 += dv * dv;
                    run = (j > a && v == prev) ? run + 1 : 1;
                    prev = v;
                }
                since = 0;
            } else {  // slide by one
                const double vo = xc[(a - 1) * ld], vi = xc[b * ld];
                const double dout = vo - A, din = vi - A;
                s1 += din - dout;
                s2 += din * din - dout * dout;
                run = vi == prev ? run + 1 : 1;
                prev = vi;
            }
            ++since;
            if (run >= w) {  // every value of the window is the same: pandas returns the value and a std of exactly 0
                mean = prev;
                sd = w > 1 ? 0.0 : nan;  // one sample: ddof = 1 leaves no degree of freedom
            } else {
                mean = A + s1 / wd;
                double num = s2 - s1 * (s1 / wd);
                if (!(num > kIllCond * s2)) {  // a spread small against the shift: the exact two-pass sums of this window
                    double q1 = 0.0, q2 = 0.0;
                    for (int64_t j = a; j <= b; ++j) q1 += xc[j * ld] - A;
                    mean = A + q1 / wd;
                    for (int64_t j = a; j <= b; ++j) {
                        const double dv = xc[j * ld] - mean;
                        q2 += dv * dv;
                    }
                    num = q2;
                    since = kRebase;  // and the next window starts from fresh sums
                }
                sd = sqrt(num / (wd - 1.0));
            }
        }
        const int64_t k = (t % P) * C + c;  // zscore.py:300-313
        const double mf = mean + shift[k], sf = sd * scale[k];
        const double z = (xt - mean) / sd;
        const int64_t at = t * ld_out + c;
        out[at] = live ? z * sf + mf : nan;
        if (meani) meani[at] = live ? mean : nan;
        if (stdi) stdi[at] = live ? sd : nan;
        if (meanf) meanf[at] = live ? mf : nan;
        if (stdf) stdf[at] = live ? sf : nan;
    }
    if (live && bad) atomicOr(&status[c], SDI_NONFINITE);
}

std::vector<sd_buf> zscore_bufs(const sd_zscore_state* st) {
    return {sd_buf_of(st->stats, ZS_NSTATS * (size_t)st->K * st->C), sd_buf_of(st->status, (size_t)st->C, true)};
}

sd_zscore_state* new_zscore(sd_ctx* ctx, int64_t K, int64_t C, int window_width) {
    sd_zscore_state* st = new sd_zscore_state();
    st->ctx = ctx;
    st->K = K;
    st->C = C;
    st->w = window_width;
    return st;
}

}  // namespace

extern "C" {

int sd_zscore_state_destroy(sd_zscore_state* st) { return sd_state_destroy(st, zscore_bufs); }

int sd_zscore_state_info(const sd_zscore_state* st, int64_t* K, int64_t* C, int* window_width) {
    SD_CHECK_ARG(st, "state is NULL");
    if (K) *K = st->K;
    if (C) *C = st->C;
    if (window_width) *window_width = st->w;
    return SD_OK;
}

int sd_zscore_state_export(const sd_zscore_state* st, double* x_mean, double* x_std, double* y_mean, double* y_std, double* shift,
                           double* scale, int32_t* cell_status) {
    SD_CHECK_ARG(st, "state is NULL");
    sd_ctx* ctx = st->ctx;
    SD_HIP(hipSetDevice(ctx->device));
    const size_t plane = (size_t)st->K * st->C;
    double* dst[ZS_NSTATS] = {x_mean, x_std, y_mean, y_std, shift, scale};  // (the one buffer holds six planes)
    for (int q = 0; q < ZS_NSTATS; ++q)
        if (dst[q]) SD_HIP(hipMemcpyAsync(dst[q], st->stats + q * plane, sizeof(double) * plane, hipMemcpyDeviceToHost, ctx->stream));
    return sd_status_fold(ctx, st->status, nullptr, st->C, cell_status);
}

int sd_zscore_state_import(sd_ctx* ctx, int64_t K, int64_t C, int window_width, const double* x_mean, const double* x_std,
                           const double* y_mean, const double* y_std, const double* shift, const double* scale,
                           const int32_t* cell_status, sd_zscore_state** out) {
    SD_CHECK_ARG(ctx && x_mean && x_std && y_mean && y_std && shift && scale && out, "sd_zscore_state_import: NULL argument");
    SD_CHECK_ARG(K > 0 && C > 0 && window_width > 0, "sd_zscore_state_import: bad sizes");
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_zscore_state* st = new_zscore(ctx, K, C, window_width);
    const std::vector<int32_t> bits = sd_status_bits(cell_status, C);
    return sd_state_build(st, sd_zscore_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, zscore_bufs(st)));
        const size_t plane = (size_t)K * C;
        const double* src[ZS_NSTATS] = {x_mean, x_std, y_mean, y_std, shift, scale};
        for (int q = 0; q < ZS_NSTATS; ++q)
            SD_HIP(hipMemcpyAsync(st->stats + q * plane, src[q], sizeof(double) * plane, hipMemcpyHostToDevice, ctx->stream));
        SD_TRY(sd_state_copy(ctx, zscore_bufs(st), {nullptr, bits.data()}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_zscore_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int64_t C, int window_width,
                      const int32_t* day_idx, const int32_t* year, int D, sd_zscore_state** out) {
    SD_CHECK_ARG(ctx && X_dev && y_dev && day_idx && year && out, "sd_zscore_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && ld >= C && D > 0, "sd_zscore_fit: bad sizes");
    SD_CHECK_ARG(T < ((int64_t)1 << 31), "sd_zscore_fit: T = %lld samples exceed the int32 sample index", (long long)T);
    *out = nullptr;
    const ZscorePlan plan = zscore_plan(day_idx, year, T, D, window_width);
    if (plan.err != SD_OK) return sd_set_error(plan.err, "%s", plan.msg.c_str());
    SD_HIP(hipSetDevice(ctx->device));
    sd_zscore_state* st = new_zscore(ctx, plan.K, C, window_width);
    return sd_state_build(st, sd_zscore_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, zscore_bufs(st)));
        std::vector<double> cnt(plan.cnt.begin(), plan.cnt.end());
        sd_scratch d_order, d_off, d_win, d_cnt, d_part;
        SD_TRY(upload(ctx, d_order, plan.order));
        SD_TRY(upload(ctx, d_off, plan.off));
        SD_TRY(upload(ctx, d_win, plan.win));
        SD_TRY(upload(ctx, d_cnt, cnt));
        SD_HIP(d_part.alloc(ctx, sizeof(double) * 4 * (size_t)D * C));
        const unsigned gx = (unsigned)((C + kCells - 1) / kCells);
        SD_LAUNCH(ctx, "zscore_day_kernel", zscore_day_kernel, dim3(gx, (unsigned)D), dim3(kCells * kDaySlices), 0, X_dev, y_dev, ld, C, D,
                  d_order.as<const int32_t>(), d_off.as<const int64_t>(), d_part.as<double>(), st->status);
        SD_LAUNCH(ctx, "zscore_window_kernel", zscore_window_kernel, dim3(gx, (unsigned)((plan.K + kWinRun - 1) / kWinRun)), dim3(kCells), 0,
                  d_part.as<const double>(), C, D, plan.K, window_width, d_win.as<const int32_t>(), d_cnt.as<const double>(),
                  (const int32_t*)st->status, st->stats);
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch tables go back to the cache on return)
        return SD_OK;
    });
}

int sd_zscore_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int64_t C, int window_width, const int32_t* day_idx,
                  const int32_t* year, int D, sd_zscore_state** out) {
    SD_CHECK_ARG(ctx && X && y && out, "sd_zscore_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0, "sd_zscore_fit: bad sizes");
    const size_t bytes = sizeof(double) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(X, bytes), sd_in(y, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_zscore_fit_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, C, window_width, day_idx, year, D, out);
    });
}

int sd_zscore_predict_dev(sd_ctx* ctx, const sd_zscore_state* st, const double* Xp_dev, int64_t ld, int64_t Tp, double* out_dev,
                          int64_t ld_out, double* meani, double* stdi, double* meanf, double* stdf, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xp_dev && out_dev, "sd_zscore_predict: NULL argument");
    SD_CHECK_ARG(Tp > 0 && ld >= st->C && ld_out >= st->C, "sd_zscore_predict: bad sizes");
    if (!zscore_expand_ok(Tp, (int)st->K)) return sd_set_error(SD_ERR_INVALID, "positional indexers are out-of-bounds");
    SD_HIP(hipSetDevice(ctx->device));
    const int64_t C = st->C;
    sd_scratch status_p;
    SD_TRY(sd_status_scratch(ctx, status_p, C));
    const size_t plane = (size_t)st->K * C;
    const dim3 grid((unsigned)((C + kCells - 1) / kCells), (unsigned)((Tp + kPredSlices * kChunk - 1) / (kPredSlices * kChunk)));
    SD_LAUNCH(ctx, "zscore_predict_kernel", zscore_predict_kernel, grid, dim3(kCells * kPredSlices), 0, Xp_dev, ld, Tp, C, st->w,
              zscore_expand_period(Tp), (const double*)(st->stats + ZS_SHIFT * plane), (const double*)(st->stats + ZS_SCALE * plane),
              (const int32_t*)st->status, status_p.as<int32_t>(), out_dev, ld_out, meani, stdi, meanf, stdf);
    return sd_status_fold(ctx, st->status, status_p.as<int32_t>(), C, cell_status);
}

int sd_zscore_predict(sd_ctx* ctx, const sd_zscore_state* st, const double* Xp, int64_t Tp, double* out, double* meani, double* stdi,
                      double* meanf, double* stdf, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xp && out, "sd_zscore_predict: NULL argument");
    SD_CHECK_ARG(Tp > 0, "sd_zscore_predict: bad sizes");
    if (!zscore_expand_ok(Tp, (int)st->K)) return sd_set_error(SD_ERR_INVALID, "positional indexers are out-of-bounds");  // (before the upload)
    const size_t bytes = sizeof(double) * (size_t)Tp * st->C;
    const sd_host_field f[] = {sd_in(Xp, bytes), sd_out(out, bytes), sd_out(meani, bytes), sd_out(stdi, bytes), sd_out(meanf, bytes),
                               sd_out(stdf, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_zscore_predict_dev(ctx, st, (const double*)d[0], st->C, Tp, (double*)d[1], st->C, (double*)d[2], (double*)d[3],
                                     (double*)d[4], (double*)d[5], cell_status);
    });
}

}  // extern "C"
