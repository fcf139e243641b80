// PureRegression (gard.py:367-504), batched over the cell axis: one ordinary least-squares fit of y on the F features per
// cell (sklearn LinearRegression = centred lstsq, gard.py:439-442), fit_error_ = RMSE of that fit; predict returns
// [pred, exceedance_prob, fit_error_] per sample (gard.py:462-470).  With a threshold (gard.py:416-437): a logistic
// regression of (y > thresh) on the features gives the exceedance probability (exact minimiser of sklearn's default
// L2-penalised objective by damped Newton steps; sklearn's L-BFGS stops within ~1e-3 of it), and the linear model and its
// RMSE use the exceeding samples only.  A cell whose samples all exceed drops its threshold like the reference does
// (probability 1); a cell without any exceeding sample is flagged (the reference's LinearRegression gets 0 samples).
//
// Fields stay in their time-major layout: a workgroup owns 64 adjacent cells x 8 time slices, every load is a
// 512-byte row fragment, so fit is one streaming pass (shifted sums and cross products), a second one over the residuals
// for the cells whose fit error the sums do not carry (one more over the sums for a cell whose first sample lies far
// from its series, one more over the residuals for a cell whose coefficients needed a refinement step), and predict one.
#include <algorithm>
#include <vector>

#include "sd_internal.h"
#include "sd_lsq.h"
#include "sd_state.h"

struct sd_linreg_state {
    sd_ctx* ctx = nullptr;
    int64_t T = 0, C = 0;
    int F = 0;
    double* coef = nullptr;       // device [F][C]
    double* intercept = nullptr;  // device [C]
    double* rmse = nullptr;       // device [C]
    int32_t* status = nullptr;    // device [C] internal bitmask
    int has_thresh = 0;
    double thresh = 0.0;
    double* logit = nullptr;        // device [F+1][C]: logistic coefficients and intercept (has_thresh)
    int32_t* thresh_off = nullptr;  // device [C]: 1 = one class only, threshold dropped (gard.py:426-437)
};

namespace {

constexpr int kMaxF = sdlsq::kMaxF;
constexpr int kCells = 64, kSlices = 8;
constexpr int kFitUnroll = 4;  // time steps of a thread whose loads are in flight together in the fit pass
constexpr double kRecentre = 16.0;  // fit: a cell whose shifted square sum of a feature exceeds this multiple of the centred one sums again

__device__ __forceinline__ bool lr_finite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

// sum over the time slices of a workgroup: part[slice][cell] -> every thread gets the total of its cell
__device__ __forceinline__ double slice_sum(double v, double* part, int cx, int ty) {
    __syncthreads();
    part[ty * kCells + cx] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int s = 0; s < kSlices; ++s) t += part[s * kCells + cx];
    return t;
}

template <int F>
__global__ void __launch_bounds__(kCells * kSlices) linreg_fit_kernel(const double* __restrict__ X, const double* __restrict__ y,
                                                                      int64_t ld, int64_t T, int64_t C, int has_thresh, double thresh,
                                                                      double* __restrict__ coef_out, double* __restrict__ icpt_out,
                                                                      double* __restrict__ rmse_out, int32_t* __restrict__ status,
                                                                      int32_t* __restrict__ thresh_off) {
    __shared__ double part[kSlices * kCells];
    __shared__ double model[(F + 1) * kCells];  // coefficients and intercept of the tile's cells
    __shared__ double rss1[kCells];             // residual sum of squares from the sums of pass 1, or -1: the cell takes pass 2
    const int cx = threadIdx.x % kCells, ty = threadIdx.x / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const bool live = c < C;
    // pass 1: sums and cross products of the data shifted by the cell's first sample (one pass; the shift keeps the
    // centring subtraction below benign as long as that sample is an ordinary one, see kRecentre), plus the mask / finite
    // bookkeeping of core.py:35-37, base.py:18-20
    double x0[F], sx[F], S[F][F], b[F], sy = 0.0, syy = 0.0;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        x0[f] = live ? X[(int64_t)f * ld + c] : 0.0;
        sx[f] = 0.0;
        b[f] = 0.0;
#pragma unroll
        for (int g = 0; g < F; ++g) S[f][g] = 0.0;
    }
    double y0 = live ? y[c] : 0.0;
    double cnt = 0.0;  // samples entering the linear model: all, or those above the threshold (gard.py:439)
    if (live)
        for (int64_t t0 = ty; t0 < T; t0 += kSlices * kFitUnroll) {
            // (the loads of kFitUnroll time steps are requested together; the sums run in time order as before)
            double wv[kFitUnroll], xv[kFitUnroll][F];
#pragma unroll
            for (int u = 0; u < kFitUnroll; ++u) {
                const int64_t t = t0 + (int64_t)u * kSlices;
                const bool ok = t < T;
                wv[u] = ok ? y[t * ld + c] : y0;
#pragma unroll
                for (int f = 0; f < F; ++f) xv[u][f] = ok ? X[(t * F + f) * ld + c] : x0[f];
            }
#pragma unroll
            for (int u = 0; u < kFitUnroll; ++u) {
                if (t0 + (int64_t)u * kSlices >= T) break;
                double d[F];
                const double w = wv[u];
                bad |= !lr_finite(w);
                const bool in = !has_thresh || w > thresh;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const double v = xv[u][f];
                    bad |= !lr_finite(v);
                    d[f] = v - x0[f];
                }
                if (!in) continue;
                cnt += 1.0;
                const double e = w - y0;
                sy += e;
                syy += e * e;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    sx[f] += d[f];
                    b[f] += d[f] * e;
#pragma unroll
                    for (int g = f; g < F; ++g) S[f][g] += d[f] * d[g];
                }
            }
        }
    if (live && ty == 0 && x0[0] != x0[0]) atomicOr(&status[c], SDI_MASKED);
    if (live && bad) atomicOr(&status[c], SDI_NONFINITE);
    const double n = slice_sum(cnt, part, cx, ty);
    if (has_thresh && live && ty == 0) {
        thresh_off[c] = n == (double)T ? 1 : 0;                  // every sample exceeds: the reference drops the threshold
        if (n == 0.0) atomicOr(&status[c], SDI_ONE_CLASS);       // none does: LinearRegression would get 0 samples
    }
    double xm[F], dm[F], em, ym, see, Syy;
    double A[kMaxF][kMaxF + 1], raw[F];
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            dm[f] = slice_sum(sx[f], part, cx, ty) / n;  // mean of the shifted feature
            xm[f] = x0[f] + dm[f];
        }
        em = slice_sum(sy, part, cx, ty) / n;
        ym = y0 + em;
        see = slice_sum(syy, part, cx, ty);
        Syy = see - n * em * em;  // centred: sum e^2 - n mean(e)^2
#pragma unroll
        for (int f = 0; f < F; ++f) {
            A[f][F] = slice_sum(b[f], part, cx, ty) - n * dm[f] * em;  // centred: sum d e - n mean(d) mean(e)
#pragma unroll
            for (int g = f; g < F; ++g) {
                const double s = slice_sum(S[f][g], part, cx, ty);
                if (g == f) raw[f] = s;
                const double v = s - n * dm[f] * dm[g];
                A[f][g] = v;
                A[g][f] = v;
            }
        }
        if (round == 1) break;
        // The shifted sums carry a rounding of ~ T u raw_f where the centred S_ff = raw_f - n dm_f^2 is wanted: a first sample
        // far from the series (a bad value, a leverage point) costs raw_f / S_ff in accuracy, on every entry of the system.
        // By the worst-case bound 3 m u (raw_f / S_ff) kappa <= 1e-7, 14 600 samples of features correlated 0.9999 tolerate a
        // ratio of 16 (a first sample 3.9 standard deviations from the mean); beyond that (kRecentre) the cell sums once more,
        // shifted by the means of pass 1, which are good to ~ u |x0 - mean|.  Decided per cell from the cell's own totals; a
        // tile without such a cell skips the pass.  Gaussian fields never take it; skewed ones (precipitation) do in 1 to 2 %
        // of their cells, which costs their tiles the pass (profiles/fit_error/README.md).
        bool recentre = false;
#pragma unroll
        for (int f = 0; f < F; ++f) recentre |= kRecentre * A[f][f] < raw[f];
        if (!__syncthreads_or(recentre)) break;
        if (live && recentre) {
            y0 = ym;
            sy = 0.0;
            syy = 0.0;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                x0[f] = xm[f];
                sx[f] = 0.0;
                b[f] = 0.0;
#pragma unroll
                for (int g = 0; g < F; ++g) S[f][g] = 0.0;
            }
            for (int64_t t0 = ty; t0 < T; t0 += kSlices * kFitUnroll) {  // (loads batched like pass 1; the sums in time order)
                double wv[kFitUnroll], xv[kFitUnroll][F];
#pragma unroll
                for (int u = 0; u < kFitUnroll; ++u) {
                    const int64_t t = t0 + (int64_t)u * kSlices;
                    const bool ok = t < T;
                    wv[u] = ok ? y[t * ld + c] : y0;
#pragma unroll
                    for (int f = 0; f < F; ++f) xv[u][f] = ok ? X[(t * F + f) * ld + c] : x0[f];
                }
#pragma unroll
                for (int u = 0; u < kFitUnroll; ++u) {
                    if (t0 + (int64_t)u * kSlices >= T) break;
                    const double w = wv[u];
                    if (has_thresh && !(w > thresh)) continue;
                    double d[F];
                    const double e = w - y0;
                    sy += e;
                    syy += e * e;
#pragma unroll
                    for (int f = 0; f < F; ++f) d[f] = xv[u][f] - x0[f];
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        sx[f] += d[f];
                        b[f] += d[f] * e;
#pragma unroll
                        for (int g = f; g < F; ++g) S[f][g] += d[f] * d[g];
                    }
                }
            }
        }
    }
    if (ty == 0) {
        double coef[kMaxF], sxy[F], sd[F];
        sdlsq::clear_unresolved(F, A, raw, n);  // a feature that is constant over the samples of the linear model
#pragma unroll
        for (int f = 0; f < F; ++f) {  // (the solver works in place)
            sxy[f] = A[f][F];
            sd[f] = A[f][f];
        }
        sdlsq::minnorm_solve(F, A, coef);
        double icpt = ym;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            icpt -= xm[f] * coef[f];
            model[f * kCells + cx] = coef[f];
        }
        model[F * kCells + cx] = icpt;
        // Residual sum of squares of the least-squares solution from the sums of pass 1: rss = Syy - coef . Sxy (the normal
        // equations), taken only where the error it carries is bounded by 1e-7 rss -- a tenth of the parity contract, which
        // leaves the square root of the RMSE and the reference's own rounding inside 1e-6.  What it carries (u = 2^-53):
        //  * every sum is m = T / 8 + 11 roundings deep (the additions of one time slice, the 8 slices, the shift and the
        //    product of a term), so sum e^2 is off by <= m u sum e^2, and n mean(e)^2, formed from sum e, by twice that:
        //    |d Syy| <= 3 m u sum e^2 -- of the *uncentred* sum, which a far first y sample makes much larger than Syy;
        //    likewise |d Sxy_f| <= 3 m u sqrt(raw_f sum e^2) >= 3 m u (sum |d_f e| + n |dm_f em|) by Cauchy-Schwarz;
        //  * with the computed coefficients the identity holds up to coef . r, r = S coef - Sxy the residual of the in-place
        //    solve: cyclic Jacobi on the equilibrated system (norm <= F) applies at most 12 F^2 / 2 rotations of 6 roundings
        //    each, |coef . r| <= 36 F^3 u (sum_f |coef_f| sqrt(S_ff))^2.
        // Every cell beyond that bound, and every cell with a threshold (subset fit: kept as it was), sums its residuals in a
        // second pass.  The decision is per cell: a cell's result does not depend on the cells that share its tile.
        double rss = Syy, lin = 0.0, wsum = 0.0;
        const double se = sqrt(see);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            rss -= coef[f] * sxy[f];
            lin += fabs(coef[f]) * sqrt(raw[f]) * se;
            wsum += fabs(coef[f]) * sqrt(sd[f] > 0.0 ? sd[f] : 0.0);
        }
        const double m = (double)((T + kSlices - 1) / kSlices + kSlices + 3), u = 1.1102230246251565e-16;
        const double carried = u * (3.0 * m * (see + lin) + 36.0 * F * F * F * wsum * wsum);
        const bool second = has_thresh || !(carried <= 1e-7 * rss);
        rss1[cx] = second ? -1.0 : rss;
    }
    __syncthreads();
    // pass 2 (cells that need it): residuals of the fit (root_mean_squared_error, gard.py:441-442), and their cross products
    // with the centred features, g = Xc^T r -- zero for the exact least-squares coefficients
    double cf[F], g[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        cf[f] = model[f * kCells + cx];
        g[f] = 0.0;
    }
    double icpt = model[F * kCells + cx];
    const double rss_sums = rss1[cx];
    const bool second = rss_sums < 0.0;
    double ss = 0.0;
    if (live && second)
        for (int64_t t = ty; t < T; t += kSlices) {
            const double w = y[t * ld + c];
            if (has_thresh && !(w > thresh)) continue;
            double xv[F], yh = icpt;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                xv[f] = X[(t * F + f) * ld + c];
                yh += xv[f] * cf[f];
            }
            const double r = w - yh;
            ss += r * r;
#pragma unroll
            for (int f = 0; f < F; ++f) g[f] += (xv[f] - xm[f]) * r;
        }
    ss = slice_sum(ss, part, cx, ty);
#pragma unroll
    for (int f = 0; f < F; ++f) g[f] = slice_sum(g[f], part, cx, ty);
    // The residual sum splits into that of the exact solution and d . g, d = S^-1 g the error of the coefficients: the part that
    // the sums and the solve put into the residuals (~ eps sqrt(T kappa) of the prediction; all there is when the fit is exact and
    // the features are nearly collinear).  Where it exceeds 1e-7 of the sum -- a tenth of the contract again -- the cell takes the
    // step d (one step of iterative refinement: the residuals come from the data, so they carry the error of the coefficients
    // to the rounding of one evaluation) and sums the residuals of the refined model in a third pass.  The second slice of a cell
    // still holds the system that the first one solved in place.  Per cell; every other cell keeps its numbers bit for bit.
    bool refine = false;
    if (ty == 1 && live && second) {
        double dl[kMaxF], dg = 0.0;
        sdlsq::clear_unresolved(F, A, raw, n);
#pragma unroll
        for (int f = 0; f < F; ++f) A[f][F] = g[f];
        sdlsq::minnorm_solve(F, A, dl);
#pragma unroll
        for (int f = 0; f < F; ++f) dg += dl[f] * g[f];
        refine = dg > 1e-7 * ss;
        if (refine) {
            double ic = ym;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const double c1 = cf[f] + dl[f];
                ic -= xm[f] * c1;
                model[f * kCells + cx] = c1;
            }
            model[F * kCells + cx] = ic;
            rss1[cx] = -2.0;
        }
    }
    if (__syncthreads_or(refine)) {
        const bool third = rss1[cx] == -2.0;
#pragma unroll
        for (int f = 0; f < F; ++f) cf[f] = model[f * kCells + cx];
        icpt = model[F * kCells + cx];
        double s3 = 0.0;
        if (live && third)
            for (int64_t t = ty; t < T; t += kSlices) {
                const double w = y[t * ld + c];
                if (has_thresh && !(w > thresh)) continue;
                double yh = icpt;
#pragma unroll
                for (int f = 0; f < F; ++f) yh += X[(t * F + f) * ld + c] * cf[f];
                const double r = w - yh;
                s3 += r * r;
            }
        s3 = slice_sum(s3, part, cx, ty);
        if (third) ss = s3;
    }
    if (live && ty == 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) coef_out[(int64_t)f * C + c] = cf[f];
        icpt_out[c] = icpt;
        rmse_out[c] = sqrt((second ? ss : rss_sums) / n);
    }
}

// LogisticRegression() of sklearn (L2, C = 1, intercept not penalised) of (y > thresh) on the features over the whole
// series of a cell (gard.py:416-420): minimise  sum_t [log(1 + exp(z_t)) - l_t z_t] + |w|^2 / 2,  z_t = w . x_t + b,
// by damped Newton steps.  Same tiling as the linear fit; every step is one streaming pass for gradient and Hessian and
// one per trial step length for the objective.  Cells with one class only keep zero coefficients (not used).
template <int F>
__global__ void __launch_bounds__(kCells * kSlices) linreg_logistic_kernel(const double* __restrict__ X, const double* __restrict__ y,
                                                                           int64_t ld, int64_t T, int64_t C, double thresh,
                                                                           const int32_t* __restrict__ status,
                                                                           const int32_t* __restrict__ thresh_off,
                                                                           double* __restrict__ logit /* [F+1][C] */) {
    constexpr int N = F + 1;
    __shared__ double part[kSlices * kCells];
    __shared__ double th_s[N * kCells], d_s[N * kCells], f_s[kCells], step_s[kCells];
    __shared__ int done_s[kCells];
    const int cx = threadIdx.x % kCells, ty = threadIdx.x / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const bool live = c < C && status[c < C ? c : 0] == 0 && thresh_off[c < C ? c : 0] == 0;
    auto objective = [&](const double* t) {  // this thread's share
        double f = 0.0;
        if (live)
            for (int64_t tt = ty; tt < T; tt += kSlices) {
                double z = t[F];
#pragma unroll
                for (int a = 0; a < F; ++a) z += t[a] * X[(tt * F + a) * ld + c];
                f += sdlsq::softplus(z) - (y[tt * ld + c] > thresh ? z : 0.0);
            }
        return f;
    };
    if (ty == 0) {
#pragma unroll
        for (int a = 0; a < N; ++a) th_s[a * kCells + cx] = 0.0;
        done_s[cx] = live ? 0 : 1;
    }
    __syncthreads();
    double th[N];
#pragma unroll
    for (int a = 0; a < N; ++a) th[a] = 0.0;
    double fcur = slice_sum(objective(th), part, cx, ty);  // (penalty is 0 at the origin)
    for (int it = 0; it < 60; ++it) {
        if (__syncthreads_and(done_s[cx])) break;
        double g[N], H[N][N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            g[a] = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) H[a][b] = 0.0;
        }
        if (live && !done_s[cx])
            for (int64_t tt = ty; tt < T; tt += kSlices) {
                double xa[N];
                double z = th[F];
#pragma unroll
                for (int a = 0; a < F; ++a) {
                    xa[a] = X[(tt * F + a) * ld + c];
                    z += th[a] * xa[a];
                }
                xa[F] = 1.0;
                const double sg = sdlsq::sigmoid(z), r = sg - (y[tt * ld + c] > thresh ? 1.0 : 0.0), w = sg * (1.0 - sg);
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    g[a] += r * xa[a];
#pragma unroll
                    for (int b = 0; b <= a; ++b) H[a][b] += w * xa[a] * xa[b];
                }
            }
        double gt[N], Ht[kMaxF + 1][kMaxF + 1];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            gt[a] = slice_sum(g[a], part, cx, ty) + (a < F ? th[a] : 0.0);
#pragma unroll
            for (int b = 0; b <= a; ++b) Ht[a][b] = slice_sum(H[a][b], part, cx, ty) + ((a == b && a < F) ? 1.0 : 0.0);
        }
        if (ty == 0 && !done_s[cx]) {
            double gmax = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) gmax = fmax(gmax, fabs(gt[a]));
            double d[kMaxF + 1];
            bool stop = gmax <= 1e-12 * (double)T;
            if (!stop) {
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    Ht[a][a] += 1e-12;
                    gt[a] = -gt[a];
                }
                stop = !sdlsq::chol_solve(N, Ht, gt, d);
            }
            if (stop) {
                done_s[cx] = 1;
            } else {
#pragma unroll
                for (int a = 0; a < N; ++a) d_s[a * kCells + cx] = d[a];
                step_s[cx] = 1.0;
            }
        }
        __syncthreads();
        // line search: halve the step until the objective does not increase (at most 40 halvings)
        for (int ls = 0; ls < 40; ++ls) {
            const bool searching = !done_s[cx] && step_s[cx] > 0.0;  // (a negative step marks an accepted one)
            double trial[N];
            double pen = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                trial[a] = th[a] + (searching ? step_s[cx] * d_s[a * kCells + cx] : 0.0);
                if (a < F) pen += 0.5 * trial[a] * trial[a];
            }
            const double fn = slice_sum(searching ? objective(trial) : 0.0, part, cx, ty) + pen;
            __syncthreads();
            if (ty == 0 && searching) {
                if (fn <= fcur || step_s[cx] < 1e-10) {
                    f_s[cx] = fn;
#pragma unroll
                    for (int a = 0; a < N; ++a) th_s[a * kCells + cx] = trial[a];
                    step_s[cx] = -1.0;  // accepted
                } else {
                    step_s[cx] *= 0.5;
                }
            }
            __syncthreads();
            const bool pending = !done_s[cx] && step_s[cx] > 0.0;
            if (!__syncthreads_or(pending)) break;
        }
#pragma unroll
        for (int a = 0; a < N; ++a) th[a] = th_s[a * kCells + cx];
        if (!done_s[cx] && step_s[cx] < 0.0) fcur = f_s[cx];
        __syncthreads();
    }
    if (ty == 0 && c < C) {
#pragma unroll
        for (int a = 0; a < N; ++a) logit[(int64_t)a * C + c] = th[a];
    }
}

template <int F>
__global__ void __launch_bounds__(kCells * kSlices) linreg_predict_kernel(const double* __restrict__ Xq, int64_t ld, int64_t Tq, int64_t C,
                                                                          const double* __restrict__ coef, const double* __restrict__ icpt_all,
                                                                          const double* __restrict__ rmse_all,
                                                                          const double* __restrict__ logit /* [F+1][C] or null */,
                                                                          const int32_t* __restrict__ thresh_off,
                                                                          const int32_t* __restrict__ fit_status, int32_t* __restrict__ status,
                                                                          double* __restrict__ out, int64_t ld_out) {
    const int cx = threadIdx.x % kCells, ty = threadIdx.x / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    if (c >= C) return;
    const bool active = fit_status[c] == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double cf[F];
#pragma unroll
    for (int f = 0; f < F; ++f) cf[f] = coef[(int64_t)f * C + c];
    const double icpt = icpt_all[c], rmse = rmse_all[c];
    const bool with_prob = logit != nullptr && thresh_off[c] == 0;  // gard.py:455-459
    double lw[F + 1];
#pragma unroll
    for (int a = 0; a <= F; ++a) lw[a] = with_prob ? logit[(int64_t)a * C + c] : 0.0;
    bool bad = false;
    const int64_t t0 = (int64_t)blockIdx.y * kSlices * 16;
    for (int64_t t = t0 + ty; t < t0 + kSlices * 16 && t < Tq; t += kSlices) {
        double p = icpt, z = lw[F];
        bool fin = true;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const double v = Xq[(t * F + f) * ld + c];
            fin = fin && lr_finite(v);
            p += v * cf[f];
            z += v * lw[f];
        }
        bad |= !fin;
        const bool okq = active && fin;
        out[(t * 3 + 0) * ld_out + c] = okq ? p : nan;      // gard.py:465
        out[(t * 3 + 1) * ld_out + c] = okq ? (with_prob ? sdlsq::sigmoid(z) : 1.0) : nan;  // gard.py:455-459: predict_proba(X)[:, 1]
        out[(t * 3 + 2) * ld_out + c] = okq ? rmse : nan;   // gard.py:461-463
    }
    if (active && bad) atomicOr(&status[c], SDI_NONFINITE);
}

template <int F>
int launch_fit(sd_ctx* ctx, const double* X, const double* y, int64_t ld, sd_linreg_state* st) {
    const dim3 grid((unsigned)((st->C + kCells - 1) / kCells));
    SD_LAUNCH(ctx, "linreg_fit_kernel", linreg_fit_kernel<F>, grid, dim3(kCells * kSlices), 0, X, y, ld, st->T, st->C, st->has_thresh,
              st->thresh, st->coef, st->intercept, st->rmse, st->status, st->thresh_off);
    if (st->has_thresh)
        SD_LAUNCH(ctx, "linreg_logistic_kernel", linreg_logistic_kernel<F>, grid, dim3(kCells * kSlices), 0, X, y, ld, st->T, st->C,
                  st->thresh, (const int32_t*)st->status, (const int32_t*)st->thresh_off, st->logit);
    return SD_OK;
}

template <int F>
int launch_predict(sd_ctx* ctx, const sd_linreg_state* st, const double* Xq, int64_t ld, int64_t Tq, int32_t* status_p, double* out,
                   int64_t ld_out) {
    const dim3 grid((unsigned)((st->C + kCells - 1) / kCells), (unsigned)((Tq + kSlices * 16 - 1) / (kSlices * 16)));
    SD_LAUNCH(ctx, "linreg_predict_kernel", linreg_predict_kernel<F>, grid, dim3(kCells * kSlices), 0, Xq, ld, Tq, st->C,
              (const double*)st->coef, (const double*)st->intercept, (const double*)st->rmse, (const double*)st->logit,
              (const int32_t*)st->thresh_off, (const int32_t*)st->status, status_p, out, ld_out);
    return SD_OK;
}

// the device buffers of a state; logit and thresh_off exist with a threshold only
std::vector<sd_buf> linreg_bufs(const sd_linreg_state* st) {
    const size_t C = (size_t)st->C, F = (size_t)st->F;
    std::vector<sd_buf> b = {sd_buf_of(st->coef, F * C), sd_buf_of(st->intercept, C), sd_buf_of(st->rmse, C), sd_buf_of(st->status, C, true)};
    if (st->has_thresh) {
        b.push_back(sd_buf_of(st->logit, (F + 1) * C, true));
        b.push_back(sd_buf_of(st->thresh_off, C, true));
    }
    return b;
}

sd_linreg_state* new_linreg(sd_ctx* ctx, int64_t T, int F, int64_t C, int has_thresh, double thresh) {
    sd_linreg_state* st = new sd_linreg_state();
    st->ctx = ctx; st->T = T; st->F = F; st->C = C;
    st->has_thresh = has_thresh;
    st->thresh = thresh;
    return st;
}

}  // namespace

extern "C" {

int sd_linreg_state_destroy(sd_linreg_state* st) { return sd_state_destroy(st, linreg_bufs); }

int sd_linreg_state_info(const sd_linreg_state* st, int64_t* T, int* F, int64_t* C) {
    SD_CHECK_ARG(st, "state is NULL");
    if (T) *T = st->T;
    if (F) *F = st->F;
    if (C) *C = st->C;
    return SD_OK;
}

int sd_linreg_state_export(const sd_linreg_state* st, double* coef, double* intercept, double* fit_error, double* logistic,
                           int32_t* thresh_dropped, int32_t* cell_status) {
    SD_CHECK_ARG(st, "state is NULL");
    sd_ctx* ctx = st->ctx;
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(sd_state_copy(ctx, linreg_bufs(st), {coef, intercept, fit_error, nullptr, logistic, thresh_dropped}, hipMemcpyDeviceToHost));
    return sd_status_fold(ctx, st->status, nullptr, st->C, cell_status);
}

// fitted numbers -> device state (pickling, checkpoint / resume): logistic == NULL for a model without a threshold
int sd_linreg_state_import(sd_ctx* ctx, int64_t T, int F, int64_t C, const double* coef, const double* intercept, const double* fit_error,
                           const double* logistic, const int32_t* thresh_dropped, const int32_t* cell_status, sd_linreg_state** out) {
    SD_CHECK_ARG(ctx && coef && intercept && fit_error && out, "sd_linreg_state_import: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && F >= 1 && F <= kMaxF, "sd_linreg_state_import: bad sizes");
    SD_CHECK_ARG((logistic == nullptr) == (thresh_dropped == nullptr), "sd_linreg_state_import: logistic and thresh_dropped go together");
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_linreg_state* st = new_linreg(ctx, T, F, C, logistic != nullptr, 0.0);
    const std::vector<int32_t> bits = sd_status_bits(cell_status, C);
    return sd_state_build(st, sd_linreg_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, linreg_bufs(st)));
        SD_TRY(sd_state_copy(ctx, linreg_bufs(st), {coef, intercept, fit_error, bits.data(), logistic, thresh_dropped}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_linreg_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                      int has_thresh, double thresh, sd_linreg_state** out) {
    SD_CHECK_ARG(ctx && X_dev && y_dev && out, "sd_linreg_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && ld >= C, "sd_linreg_fit: bad sizes");
    SD_CHECK_ARG(F >= 1 && F <= kMaxF, "sd_linreg_fit: F=%d outside [1,%d]", F, kMaxF);
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_linreg_state* st = new_linreg(ctx, T, F, C, has_thresh ? 1 : 0, thresh);
    return sd_state_build(st, sd_linreg_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, linreg_bufs(st)));
        SD_DISPATCH_F(F, launch_fit, ctx, X_dev, y_dev, ld, st);
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_linreg_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, int has_thresh, double thresh,
                  sd_linreg_state** out) {
    SD_CHECK_ARG(ctx && X && y && out, "sd_linreg_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0 && F >= 1, "sd_linreg_fit: bad sizes");
    const size_t bytes = sizeof(double) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(X, bytes * F), sd_in(y, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_linreg_fit_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, F, C, has_thresh, thresh, out);
    });
}

int sd_linreg_predict_dev(sd_ctx* ctx, const sd_linreg_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, double* out_dev,
                          int64_t ld_out, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq_dev && out_dev, "sd_linreg_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0 && ld >= st->C && ld_out >= st->C, "sd_linreg_predict: bad sizes");
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch status_p;
    SD_TRY(sd_status_scratch(ctx, status_p, st->C));
    SD_DISPATCH_F(st->F, launch_predict, ctx, st, Xq_dev, ld, Tq, status_p.as<int32_t>(), out_dev, ld_out);
    return sd_status_fold(ctx, st->status, status_p.as<int32_t>(), st->C, cell_status);
}

int sd_linreg_predict(sd_ctx* ctx, const sd_linreg_state* st, const double* Xq, int64_t Tq, double* out, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq && out, "sd_linreg_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0, "sd_linreg_predict: bad sizes");
    const size_t bytes = sizeof(double) * (size_t)Tq * st->C;
    const sd_host_field f[] = {sd_in(Xq, bytes * st->F), sd_out(out, bytes * 3)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_linreg_predict_dev(ctx, st, (const double*)d[0], st->C, Tq, (double*)d[1], st->C, cell_status);
    });
}

}  // extern "C"
