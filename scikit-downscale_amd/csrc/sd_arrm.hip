// PiecewiseLinearRegression(fit_option='arrm') of the reference (arrm.py:19-105, 144-177), batched over the cell axis: the
// breakpoints of the Asynchronous Regional Regression Model (windows of the two independently sorted series whose correlation
// is lowest) and a continuous piecewise-linear least-squares fit on them (pwlf's fit_with_breaks, degree 1).
//
// fit:
//   sd_qm_fit_dev          np.sort of X and of y per cell (the quantile-mapping sorts) -> xs, ys [C][T] in HBM
//   arrm_select_kernel     one workgroup per cell.  The r2 series of the cell lives in LDS (8 T bytes); xs and ys are read from
//                          HBM / L2, each thread sums its first window directly around a pivot at the window's centre and slides
//                          to its next windows.  Of two windows that share a slot only the one the reference writes last stores.
//                          Then the reference's sequence as it stands: upper picks with their masks, the lower windows, lower picks.
//                          A cell whose lower range is empty (smallest upper pick 6), where the reference's argmin raises, gets
//                          SDI_EMPTY_RANGE and no model.
//   arrm_accum_kernel      one pass over the original (x, y) pairs, [T, C] with coalesced rows: the Gram sums of the hat-function
//                          basis on the cell's knots, five per segment, in LDS per thread; fixed-order reduction.
//   arrm_solve_kernel      one thread per cell: equilibrated tridiagonal Cholesky, conversion to pwlf's beta, minimum-norm
//                          correction for redundant columns (duplicate breaks, breaks at the ends of the data).
// predict: arrm_predict_kernel, one streaming pass: beta0 + beta1 (x - b0) + sum_j beta_{j+1} max(x - b_j, 0).
#include <algorithm>
#include <climits>
#include <vector>

#include "sd_arrm_plan.h"
#include "sd_internal.h"
#include "sd_state.h"

struct sd_arrm_state {
    sd_ctx* ctx = nullptr;
    int64_t C = 0, T = 0;
    int B = 0;
    double* breaks = nullptr;        // device [B][C]
    int32_t* break_index = nullptr;  // device [B][C]
    double* beta = nullptr;          // device [B][C]
    double* ssr = nullptr;           // device [C]
    int32_t* status = nullptr;       // device [C] internal bitmask
};

namespace {

using sdarrm::kCells;
using sdarrm::kMaxBreaks;
using sdarrm::kMinWidth;
using sdarrm::kWindowThreads;

__device__ __forceinline__ bool ar_finite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }
__device__ __forceinline__ double ar_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// np.argmin's order: NaN is the minimum, the lowest index wins among equals
__device__ __forceinline__ bool ar_better(double a, int ia, double b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (na || a == b) return ia < ib;
    return a < b;
}

__device__ int ar_block_argmin(const double* r2, int limit, double* red_v, int* red_i) {
    const int tid = threadIdx.x;
    double bv = 0.0;
    int bi = INT_MAX;  // INT_MAX: nothing seen
    for (int i = tid; i < limit; i += kWindowThreads) {
        const double v = r2[i];
        if (bi == INT_MAX || ar_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = kWindowThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int oi = red_i[tid + s];
            const double ov = red_v[tid + s];
            if (oi != INT_MAX && (red_i[tid] == INT_MAX || ar_better(ov, oi, red_v[tid], red_i[tid]))) {
                red_v[tid] = ov;
                red_i[tid] = oi;
            }
        }
        __syncthreads();
    }
    const int res = red_i[0];
    __syncthreads();
    return res == INT_MAX ? 0 : res;
}

// r2 of the windows [left, min(left + w, T)) for left in [lo, hi]: the thread takes a run of consecutive lefts, sums the first
// window directly as deviations from the samples at its centre and slides on with the same pivot (a run is at most
// T / kWindowThreads + 1 windows long, so the pivot stays inside or next to the window).  No barrier inside.
__device__ void ar_window_pass(const double* __restrict__ xs, const double* __restrict__ ys, int T, int w, int lo, int hi, bool upper,
                               double* r2, double* __restrict__ diag, int64_t C) {
    const int nwin = hi - lo + 1;
    if (nwin <= 0) return;
    const int L = (nwin + kWindowThreads - 1) / kWindowThreads;
    const int l0 = lo + (int)threadIdx.x * L, l1 = min(l0 + L - 1, hi);
    if (l0 > hi) return;
    const int piv = min(l0 + w / 2, T - 1);
    const double px = xs[piv], py = ys[piv];
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int j = l0, r = min(l0 + w, T); j < r; ++j) {
        const double dx = xs[j] - px, dy = ys[j] - py;
        sx += dx;
        sy += dy;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
    }
    for (int left = l0; left <= l1; ++left) {
        const int right = min(left + w, T), cnt = right - left;
        const double x_first = xs[left], y_first = ys[left];
        const bool fin = upper ? sdarrm::upper_final(left, w, T) : sdarrm::lower_final(left, w);
        if (fin) {
            const double n = (double)cnt, my = sy / n;
            const double cxx = sxx - sx * (sx / n), cyy = syy - sy * my, cxy = sxy - sx * my;
            double val = ar_nan();
            // a window of equal xs or equal ys (sorted: first == last) has no correlation: NaN, which argmin takes first
            if (x_first != xs[right - 1] && y_first != ys[right - 1] && cxx > 0.0 && cyy > 0.0) {
                double r = cxy / sqrt(cxx) / sqrt(cyy);
                r = fmin(fmax(r, -1.0), 1.0);  // np.corrcoef clips
                val = r * r;
            }
            const int mid = (int)sdarrm::mid_of(left, left + w);
            if (mid < T) {  // (always: the reference would fail with an IndexError otherwise)
                r2[mid] = val;
                if (diag) diag[(int64_t)mid * C] = val;
            }
        }
        if (left < l1) {
            double dx = x_first - px, dy = y_first - py;
            sx -= dx;
            sy -= dy;
            sxx -= dx * dx;
            syy -= dy * dy;
            sxy -= dx * dy;
            if (left + w < T) {
                dx = xs[left + w] - px;
                dy = ys[left + w] - py;
                sx += dx;
                sy += dy;
                sxx += dx * dx;
                syy += dy * dy;
                sxy += dx * dy;
            }
        }
    }
}

// r2[i - 10 : i + 11] = 1 with Python's slice rules on a series of T >= 50 samples: a negative start wraps to T + start, which
// lies behind the stop, so nothing is masked (and the same index is picked again)
__device__ __forceinline__ void ar_mask(double* r2, int i, int T) {
    int lo = i - kMinWidth;
    const int hi = min(i + kMinWidth + 1, T);
    if (lo < 0) lo += T;
    for (int j = lo + (int)threadIdx.x; j < hi; j += kWindowThreads) r2[j] = 1.0;
}

__global__ void __launch_bounds__(kWindowThreads) arrm_select_kernel(const double* __restrict__ xs_all, const double* __restrict__ ys_all, int T,
                                                                     int64_t C, int start, int w, int half,
                                                                     int32_t* status, double* __restrict__ breaks,
                                                                     int32_t* __restrict__ break_index, double* __restrict__ diag_all) {
    extern __shared__ double r2[];  // [T]
    __shared__ double red_v[kWindowThreads];
    __shared__ int red_i[kWindowThreads];
    __shared__ int picks[kMaxBreaks];
    const int tid = threadIdx.x, B = 2 * half;
    for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
        double* diag = diag_all ? diag_all + c : nullptr;
        if (status[c] != 0) {  // (uniform over the workgroup)
            if (tid < B) {
                breaks[(int64_t)tid * C + c] = ar_nan();
                break_index[(int64_t)tid * C + c] = -1;
            }
            if (diag)
                for (int t = tid; t < T; t += kWindowThreads) diag[(int64_t)t * C] = ar_nan();
            continue;
        }
        const double* xs = xs_all + c * T;
        const double* ys = ys_all + c * T;
        for (int t = tid; t < T; t += kWindowThreads) {
            r2[t] = 2.0;
            if (diag) diag[(int64_t)t * C] = 2.0;
        }
        __syncthreads();
        ar_window_pass(xs, ys, T, w, start - w, T - w, true, r2, diag, C);  // right = start .. T
        __syncthreads();
        for (int k = 0; k < half; ++k) {
            const int i = ar_block_argmin(r2, T, red_v, red_i);
            if (tid == 0) picks[k] = i;
            ar_mask(r2, i, T);
            __syncthreads();
        }
        int start2 = picks[0];
        for (int k = 1; k < half; ++k) start2 = min(start2, picks[k]);
        start2 -= kMinWidth / 2 + 1;
        if (start2 == 0) {  // (uniform) arrm.py:95: r2[:0] is empty and np.argmin raises: the cell gets no model, r2 keeps the upper windows
            if (tid < B) {
                breaks[(int64_t)tid * C + c] = ar_nan();
                break_index[(int64_t)tid * C + c] = -1;
            }
            if (tid == 0) status[c] = SDI_EMPTY_RANGE;  // (read again by this workgroup only at its next cell; the later kernels see it)
            continue;
        }
        if (start2 >= 0) ar_window_pass(xs, ys, T, w, 0, start2, false, r2, diag, C);  // left = start2 .. 0
        __syncthreads();
        const int limit = start2 >= 0 ? start2 : T + start2;  // r2[:start2]
        for (int k = 0; k < half; ++k) {
            const int i = ar_block_argmin(r2, limit, red_v, red_i);
            if (tid == 0) picks[half + k] = i;
            ar_mask(r2, i, T);
            __syncthreads();
        }
        if (tid == 0) {
            for (int a = 1; a < B; ++a) {
                const int v = picks[a];
                int b = a - 1;
                for (; b >= 0 && picks[b] > v; --b) picks[b + 1] = picks[b];
                picks[b + 1] = v;
            }
            for (int j = 0; j < B; ++j) {
                breaks[(int64_t)j * C + c] = xs[picks[j]];
                break_index[(int64_t)j * C + c] = picks[j];
            }
        }
        __syncthreads();
    }
}

// Knots of the hat-function basis of one cell: the smallest x, the distinct breaks b[1 .. B-2] strictly inside the data, the
// largest x.  b[0] is only pwlf's origin and b[B-1] does not enter the model.  kn has stride `stride`.
__device__ __forceinline__ int ar_knots(const double* __restrict__ breaks, int64_t C, int64_t c, int B, double xmin, double xmax, double* kn,
                                        int stride) {
    int nk = 1;
    double last = xmin;
    kn[0] = xmin;
    for (int j = 1; j <= B - 2; ++j) {
        const double b = breaks[(int64_t)j * C + c];
        if (b > last && b < xmax) {
            kn[nk * stride] = b;
            ++nk;
            last = b;
        }
    }
    if (xmax > xmin) {
        kn[nk * stride] = xmax;
        ++nk;
    }
    return nk;
}

// Per segment s of the cell's knots, with u = (x - k_s) / (k_{s+1} - k_s) and v = 1 - u: sum v^2, sum u v, sum u^2, sum v e,
// sum u e, where e = y - y[0]; and sum e^2.  part [slice][nacc][C].
__global__ void __launch_bounds__(256) arrm_accum_kernel(const double* __restrict__ X, const double* __restrict__ y, int64_t ld, int T, int64_t C,
                                                         int B, const double* __restrict__ xs_all, const double* __restrict__ breaks,
                                                         const int32_t* __restrict__ status, double* __restrict__ part, int nacc) {
    extern __shared__ double sm[];  // knots [kMaxBreaks][kCells], then the sums [nacc - 1][blockDim.x]
    __shared__ int nks[kCells];
    double* knots = sm;
    double* acc = sm + kMaxBreaks * kCells;
    const int tid = threadIdx.x, nthr = blockDim.x, cx = tid % kCells, sl = tid / kCells, nsl = nthr / kCells;
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    const bool live = c < C && status[c] == 0;
    if (sl == 0) nks[cx] = live ? ar_knots(breaks, C, c, B, xs_all[c * T], xs_all[c * T + T - 1], knots + cx, kCells) : 0;
    for (int q = 0; q < nacc - 1; ++q) acc[q * nthr + tid] = 0.0;
    __syncthreads();
    const int nk = nks[cx];
    const int S = gridDim.y * nsl, my = blockIdx.y * nsl + sl;
    const int t0 = (int)((int64_t)T * my / S), t1 = (int)((int64_t)T * (my + 1) / S);
    double see = 0.0;
    if (live) {
        const double y0 = y[c];
        for (int t = t0; t < t1; ++t) {
            const double x = X[(int64_t)t * ld + c], e = y[(int64_t)t * ld + c] - y0;
            int s = 0;
            for (int i = 1; i < nk - 1; ++i) s += x >= knots[i * kCells + cx] ? 1 : 0;
            double u = 0.0;
            if (nk >= 2) {
                const double k0 = knots[s * kCells + cx], k1 = knots[(s + 1) * kCells + cx];
                u = (x - k0) / (k1 - k0);
            }
            const double v = 1.0 - u;
            double* a = acc + (5 * s) * nthr + tid;
            a[0] += v * v;
            a[nthr] += u * v;
            a[2 * nthr] += u * u;
            a[3 * nthr] += v * e;
            a[4 * nthr] += u * e;
            see += e * e;
        }
    }
    __syncthreads();
    knots[tid] = see;  // (the knots are not needed any more: kMaxBreaks * kCells >= blockDim.x slots)
    __syncthreads();
    if (sl == 0 && c < C) {
        double* dst = part + (int64_t)blockIdx.y * nacc * C + c;
        for (int q = 0; q < nacc - 1; ++q) {
            double s = 0.0;
            for (int k = 0; k < nsl; ++k) s += acc[q * nthr + cx + kCells * k];
            dst[(int64_t)q * C] = s;
        }
        double s = 0.0;
        for (int k = 0; k < nsl; ++k) s += knots[cx + kCells * k];
        dst[(int64_t)(nacc - 1) * C] = s;
    }
}

// Least squares in the hat basis (tridiagonal Gram matrix, equilibrated, Cholesky), then pwlf's parameters:
// beta0 + beta1 (x - b0) + sum_{j=1}^{B-2} beta_{j+1} max(x - b_j, 0).  A hinge whose break repeats an earlier one, or sits at the
// smallest or largest x, makes the design matrix rank deficient; LAPACK's gelsd then returns the solution of minimum norm, which
// is the particular solution below minus its component in the null space spanned by the vectors built here.
__global__ void __launch_bounds__(256) arrm_solve_kernel(const double* __restrict__ part, int slices, int nacc, const double* __restrict__ y,
                                                         int T, int64_t C, int B, const double* __restrict__ xs_all,
                                                         const double* __restrict__ breaks, const int32_t* __restrict__ status,
                                                         double* __restrict__ beta_out, double* __restrict__ ssr_out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (status[c] != 0) {
        for (int j = 0; j < B; ++j) beta_out[(int64_t)j * C + c] = ar_nan();
        ssr_out[c] = ar_nan();
        return;
    }
    double kn[kMaxBreaks], b[kMaxBreaks];
    const double xmin = xs_all[c * T], xmax = xs_all[c * T + T - 1], y0 = y[c];
    for (int j = 0; j < B; ++j) b[j] = breaks[(int64_t)j * C + c];
    const int nk = ar_knots(breaks, C, c, B, xmin, xmax, kn, 1);
    const int nseg = nk >= 2 ? nk - 1 : 1;
    double D[kMaxBreaks], O[kMaxBreaks], g[kMaxBreaks], cf[kMaxBreaks];
    for (int i = 0; i < kMaxBreaks; ++i) D[i] = O[i] = g[i] = cf[i] = 0.0;
    for (int s = 0; s < nseg; ++s) {
        double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < slices; ++k)
            for (int r = 0; r < 5; ++r) q[r] += part[((int64_t)k * nacc + 5 * s + r) * C + c];
        D[s] += q[0];
        O[s] = q[1];
        D[s + 1] += q[2];
        g[s] += q[3];
        g[s + 1] += q[4];
    }
    double see = 0.0;
    for (int k = 0; k < slices; ++k) see += part[((int64_t)k * nacc + nacc - 1) * C + c];
    // equilibrated tridiagonal Cholesky: unit diagonal, off-diagonal O_i / sqrt(D_i D_{i+1})
    double sc[kMaxBreaks], l[kMaxBreaks], m[kMaxBreaks], z[kMaxBreaks];
    bool ok = true;
    for (int i = 0; i < nk; ++i) {
        ok = ok && D[i] > 0.0;
        sc[i] = 1.0 / sqrt(D[i]);
    }
    l[0] = 1.0;
    z[0] = g[0] * sc[0];
    for (int i = 0; i + 1 < nk; ++i) {
        m[i] = O[i] * sc[i] * sc[i + 1] / l[i];
        const double d = 1.0 - m[i] * m[i];
        ok = ok && d > 0.0;
        l[i + 1] = sqrt(d);
        z[i + 1] = (g[i + 1] * sc[i + 1] - m[i] * z[i]) / l[i + 1];
    }
    cf[nk - 1] = z[nk - 1] / l[nk - 1];
    for (int i = nk - 2; i >= 0; --i) cf[i] = (z[i] - m[i] * cf[i + 1]) / l[i];
    double fit = 0.0;
    for (int i = 0; i < nk; ++i) {
        cf[i] *= sc[i];  // the fitted value at knot i, relative to y0
        fit += cf[i] * g[i];
    }
    // particular solution: the slopes of the segments; redundant hinges get 0
    double slope[kMaxBreaks], beta[kMaxBreaks];
    for (int i = 0; i + 1 < nk; ++i) slope[i] = (cf[i + 1] - cf[i]) / (kn[i + 1] - kn[i]);
    for (int j = 0; j < B; ++j) beta[j] = 0.0;
    beta[1] = nk >= 2 ? slope[0] : 0.0;
    beta[0] = y0 + cf[0] - beta[1] * (xmin - b[0]);
    double N[kMaxBreaks][kMaxBreaks];
    int nn = 0;
    const auto null_vector = [&](int col, int col2, double w2, double w0) {  // e_col + w2 e_col2 + w0 e_0
        for (int f = 0; f < B; ++f) N[nn][f] = 0.0;
        N[nn][col] = 1.0;
        if (col2 >= 0) N[nn][col2] += w2;
        N[nn][0] += w0;
        ++nn;
    };
    if (nk == 1) null_vector(1, -1, 0.0, -(xmin - b[0]));  // x - b0 is constant on the data
    int ki = 0, rep = 0;  // interior knots seen; the hinge that owns the last of them
    for (int j = 1; j <= B - 2; ++j) {
        if (b[j] <= xmin) {
            null_vector(j + 1, 1, -1.0, -(b[0] - b[j]));  // the hinge is x - b_j on all of the data
        } else if (b[j] >= xmax) {
            null_vector(j + 1, -1, 0.0, 0.0);  // the hinge is 0 on all of the data
        } else if (ki > 0 && b[j] == kn[ki]) {
            null_vector(j + 1, rep + 1, -1.0, 0.0);  // the same hinge again
        } else {
            ++ki;
            rep = j;
            beta[j + 1] = slope[ki] - slope[ki - 1];
        }
    }
    // minimum norm: take out the components along the null space (modified Gram-Schmidt)
    int no = 0;
    for (int p = 0; p < nn; ++p) {
        for (int q = 0; q < no; ++q) {
            double dot = 0.0;
            for (int f = 0; f < B; ++f) dot += N[p][f] * N[q][f];
            for (int f = 0; f < B; ++f) N[p][f] -= dot * N[q][f];
        }
        double n2 = 0.0;
        for (int f = 0; f < B; ++f) n2 += N[p][f] * N[p][f];
        if (!(n2 > 1e-24)) continue;
        const double inv = 1.0 / sqrt(n2);
        for (int f = 0; f < B; ++f) N[no][f] = N[p][f] * inv;
        ++no;
    }
    for (int q = 0; q < no; ++q) {
        double dot = 0.0;
        for (int f = 0; f < B; ++f) dot += beta[f] * N[q][f];
        for (int f = 0; f < B; ++f) beta[f] -= dot * N[q][f];
    }
    for (int j = 0; j < B; ++j) beta_out[(int64_t)j * C + c] = ok ? beta[j] : ar_nan();
    ssr_out[c] = ok ? fmax(see - fit, 0.0) : ar_nan();
}

__global__ void __launch_bounds__(256) arrm_predict_kernel(const double* __restrict__ Xq, int64_t ld, int64_t Tq, int64_t C, int B,
                                                           const double* __restrict__ breaks, const double* __restrict__ beta,
                                                           const int32_t* __restrict__ fit_status, int32_t* __restrict__ status,
                                                           double* __restrict__ out, int64_t ld_out) {
    extern __shared__ double sm[];  // breaks [B][kCells], beta [B][kCells]
    double* bk = sm;
    double* bt = sm + B * kCells;
    const int tid = threadIdx.x, cx = tid % kCells, sl = tid / kCells, nsl = blockDim.x / kCells;
    for (int i = tid; i < B * kCells; i += blockDim.x) {
        const int64_t c2 = (int64_t)blockIdx.x * kCells + i % kCells;
        const int j = i / kCells;
        bk[i] = c2 < C ? breaks[(int64_t)j * C + c2] : 0.0;
        bt[i] = c2 < C ? beta[(int64_t)j * C + c2] : 0.0;
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * kCells + cx;
    if (c >= C) return;
    const bool active = fit_status[c] == 0;
    const double b0 = bk[cx], beta0 = bt[cx], beta1 = bt[kCells + cx];
    const int64_t t_begin = (int64_t)blockIdx.y * nsl * 64 + sl;
    bool bad = false;
#pragma unroll 4
    for (int i = 0; i < 64; ++i) {
        const int64_t t = t_begin + (int64_t)i * nsl;
        if (t >= Tq) break;
        const double x = Xq[t * ld + c];
        const bool fin = ar_finite(x);
        double p = beta0 + beta1 * (x - b0);
        for (int j = 1; j <= B - 2; ++j) p += bt[(j + 1) * kCells + cx] * fmax(x - bk[j * kCells + cx], 0.0);
        bad |= !fin;
        out[t * ld_out + c] = active && fin ? p : ar_nan();
    }
    if (active && bad) atomicOr(&status[c], SDI_NONFINITE);
}

dim3 grid_of(const ArrmLaunch& L) { return dim3((unsigned)L.gx, (unsigned)L.gy); }

template <class Kernel>
int allow_lds(Kernel kernel, const ArrmLaunch& L) {
    if (L.lds > ((size_t)64 << 10))
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    return SD_OK;
}

std::vector<sd_buf> arrm_bufs(const sd_arrm_state* st) {
    const size_t C = (size_t)st->C, n = (size_t)st->B * C;
    return {sd_buf_of(st->breaks, n), sd_buf_of(st->break_index, n), sd_buf_of(st->beta, n), sd_buf_of(st->ssr, C),
            sd_buf_of(st->status, C, true)};
}

sd_arrm_state* new_arrm(sd_ctx* ctx, int B, int64_t C, int64_t T) {
    sd_arrm_state* st = new sd_arrm_state();
    st->ctx = ctx; st->B = B; st->C = C; st->T = T;
    return st;
}

}  // namespace

extern "C" {

int sd_arrm_state_destroy(sd_arrm_state* st) { return sd_state_destroy(st, arrm_bufs); }

int sd_arrm_state_info(const sd_arrm_state* st, int* B, int64_t* C, int64_t* T) {
    SD_CHECK_ARG(st, "state is NULL");
    if (B) *B = st->B;
    if (C) *C = st->C;
    if (T) *T = st->T;
    return SD_OK;
}

int sd_arrm_state_export(const sd_arrm_state* st, double* breaks, int32_t* break_index, double* beta, double* ssr, int32_t* cell_status) {
    SD_CHECK_ARG(st, "state is NULL");
    sd_ctx* ctx = st->ctx;
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(sd_state_copy(ctx, arrm_bufs(st), {breaks, break_index, beta, ssr}, hipMemcpyDeviceToHost));
    return sd_status_fold(ctx, st->status, nullptr, st->C, cell_status);
}

// fitted numbers -> device state (pickling, checkpoint / resume)
int sd_arrm_state_import(sd_ctx* ctx, int B, int64_t C, int64_t T, const double* breaks, const int32_t* break_index, const double* beta,
                         const double* ssr, const int32_t* cell_status, sd_arrm_state** out) {
    SD_CHECK_ARG(ctx && breaks && break_index && beta && ssr && out, "sd_arrm_state_import: NULL argument");
    SD_CHECK_ARG(C > 0 && B >= 2 && B <= kMaxBreaks && B % 2 == 0 && T >= 0, "sd_arrm_state_import: bad sizes");
    *out = nullptr;
    SD_HIP(hipSetDevice(ctx->device));
    sd_arrm_state* st = new_arrm(ctx, B, C, T);
    const std::vector<int32_t> bits = sd_status_bits(cell_status, C);
    return sd_state_build(st, sd_arrm_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, arrm_bufs(st)));
        SD_TRY(sd_state_copy(ctx, arrm_bufs(st), {breaks, break_index, beta, ssr, bits.data()}, hipMemcpyHostToDevice));
        SD_HIP(hipStreamSynchronize(ctx->stream));
        return SD_OK;
    });
}

int sd_arrm_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int64_t C, int max_breakpoints,
                    double* r2_dev, sd_arrm_state** out) {
    SD_CHECK_ARG(ctx && X_dev && y_dev && out, "sd_arrm_fit: NULL argument");
    *out = nullptr;
    ArrmCall call;
    call.T = T, call.C = C, call.ld = ld;
    call.max_breakpoints = max_breakpoints;
    call.lds_max = ctx->lds_max;
    call.cu_count = ctx->cu_count;
    const ArrmPlan pl = arrm_plan(call);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    sd_qm_state* sorted = nullptr;
    SD_TRY(sd_qm_fit_dev(ctx, X_dev, y_dev, ld, T, C, &sorted));  // xs, ys [C][T]; the mask and non-finite bookkeeping
    sd_arrm_state* st = new_arrm(ctx, pl.B, C, T);
    const int rc = sd_state_build(st, sd_arrm_state_destroy, out, [&]() -> int {
        SD_TRY(sd_state_alloc(ctx, arrm_bufs(st)));
        SD_HIP(hipMemcpyAsync(st->status, sorted->status, sizeof(int32_t) * C, hipMemcpyDeviceToDevice, ctx->stream));
        SD_TRY(allow_lds(&arrm_select_kernel, pl.select));
        SD_LAUNCH(ctx, "arrm_select_kernel", arrm_select_kernel, grid_of(pl.select), dim3(pl.select.block), pl.select.lds,
                  (const double*)sorted->xs, (const double*)sorted->ys, (int)T, C, (int)pl.start, (int)pl.width, pl.half,
                  st->status, st->breaks, st->break_index, r2_dev);
        sd_scratch part;
        SD_HIP(part.alloc(ctx, sizeof(double) * (size_t)pl.slices * pl.nacc * C));
        SD_TRY(allow_lds(&arrm_accum_kernel, pl.accum));
        SD_LAUNCH(ctx, "arrm_accum_kernel", arrm_accum_kernel, grid_of(pl.accum), dim3(pl.accum.block), pl.accum.lds, X_dev, y_dev, ld, (int)T, C,
                  pl.B, (const double*)sorted->xs, (const double*)st->breaks, (const int32_t*)st->status, part.as<double>(), pl.nacc);
        SD_LAUNCH(ctx, "arrm_solve_kernel", arrm_solve_kernel, grid_of(pl.solve), dim3(pl.solve.block), pl.solve.lds,
                  (const double*)part.p, pl.slices, pl.nacc, y_dev, (int)T, C, pl.B, (const double*)sorted->xs, (const double*)st->breaks,
                  (const int32_t*)st->status, st->beta, st->ssr);
        SD_HIP(hipStreamSynchronize(ctx->stream));  // (the partial sums go back to the cache on return)
        return SD_OK;
    });
    sd_qm_state_destroy(sorted);
    return rc;
}

int sd_arrm_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int64_t C, int max_breakpoints, double* r2, sd_arrm_state** out) {
    SD_CHECK_ARG(ctx && X && y && out, "sd_arrm_fit: NULL argument");
    SD_CHECK_ARG(T > 0 && C > 0, "sd_arrm_fit: bad sizes");
    *out = nullptr;
    const size_t bytes = sizeof(double) * (size_t)T * C;
    const sd_host_field f[] = {sd_in(X, bytes), sd_in(y, bytes), sd_out(r2, bytes)};
    const int rc = with_device_copies(ctx, f, [&](void* const* d) {
        return sd_arrm_fit_dev(ctx, (const double*)d[0], (const double*)d[1], C, T, C, max_breakpoints, (double*)d[2], out);
    });
    if (rc != SD_OK && *out) {  // the fit succeeded, r2 did not come back: no state without it
        sd_arrm_state_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int sd_arrm_predict_dev(sd_ctx* ctx, const sd_arrm_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, double* out_dev, int64_t ld_out,
                        int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq_dev && out_dev, "sd_arrm_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0 && ld >= st->C && ld_out >= st->C, "sd_arrm_predict: bad sizes");
    const int64_t C = st->C;
    const ArrmLaunch L = arrm_predict_launch(Tq, C, st->B);
    SD_CHECK_ARG(L.gy < 65536, "sd_arrm_predict: Tq = %lld samples exceed the grid", (long long)Tq);
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch status_p;
    SD_TRY(sd_status_scratch(ctx, status_p, C));
    SD_LAUNCH(ctx, "arrm_predict_kernel", arrm_predict_kernel, grid_of(L), dim3(L.block), L.lds, Xq_dev, ld, Tq, C, st->B,
              (const double*)st->breaks, (const double*)st->beta, (const int32_t*)st->status, status_p.as<int32_t>(), out_dev, ld_out);
    return sd_status_fold(ctx, st->status, status_p.as<int32_t>(), C, cell_status);
}

int sd_arrm_predict(sd_ctx* ctx, const sd_arrm_state* st, const double* Xq, int64_t Tq, double* out, int32_t* cell_status) {
    SD_CHECK_ARG(ctx && st && Xq && out, "sd_arrm_predict: NULL argument");
    SD_CHECK_ARG(Tq > 0, "sd_arrm_predict: bad sizes");
    const size_t bytes = sizeof(double) * (size_t)Tq * st->C;
    const sd_host_field f[] = {sd_in(Xq, bytes), sd_out(out, bytes)};
    return with_device_copies(ctx, f, [&](void* const* d) {
        return sd_arrm_predict_dev(ctx, st, (const double*)d[0], st->C, Tq, (double*)d[1], st->C, cell_status);
    });
}

}  // extern "C"
