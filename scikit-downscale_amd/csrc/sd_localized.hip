// Localized analogs (LocalizedAnalogs; LOCA, Pierce et al. 2014): from the k regional analogs of a target day every coarse cell keeps
// the library day that matches the target best around that cell, and the fine field copies, cell by cell, the day chosen for its coarse
// cell, shifted or scaled to the coarse target.  The rule is stated in include/sd_downscale.h and restated by
// tests/_localized_oracle.py; the launch plans and the tile constants are in sd_localized_plan.h.  The regional stage is
// sd_ca_select_dev (sd_constructed.hip); the used columns come from the kernel both units share (sd_constructed_cols.h).
//
// ca_local_kernel: one workgroup of 512 threads per target.  Q[q] is staged once; then, analog by analog, the row of terms
// wc * (e * e) -- +0.0 at a column that is not used: every term is >= +0.0 or +inf, so adding +0.0 gives the bits of skipping it, and
// the e of such a column is never formed.  Thread tid owns the coarse cells tid, tid + 512, ...: it adds the terms of a cell's
// neighbourhood in the order of the rule (rows ascending, columns ascending within a row) and keeps the running minimum and its slot in
// registers.  The order is per cell, so no split over threads can change a bit; no separable or sliding sums, which would.
// Tq * k * Cc * (2 ry + 1)(2 rx + 1) LDS reads and additions: small beside ca_select_kernel.
//
// ca_local_apply_kernel<S>: the memory side, one gather per output value: Tq * Cf fine samples read for Tq * Cf doubles written.
// A workgroup of 4 waves owns 256 consecutive fine cells, one per thread, and 16 targets.  cell_of is read once per thread; per target
// a thread reads the day of its coarse cell from the local_idx row (neighbouring lanes share a coarse cell: a wave touches a few
// distinct words of a row of Cc ints that stays in cache), gathers its fine sample -- consecutive lanes of one coarse cell read
// consecutive samples of one library row -- and, for SHIFT / SCALE, Q[q, c] and L[t, c] the same way.  4 targets are in flight per
// thread before their arithmetic.  Floor: Tq * Cf * (itemsize + 8) bytes; profiles/localized_analogs/ has what is reached.
#include <algorithm>
#include <vector>

#include "sd_constructed_cols.h"
#include "sd_internal.h"
#include "sd_localized_plan.h"
#include "sd_state.h"

namespace {
using namespace sdlo;

__global__ void __launch_bounds__(kLocBlock) ca_local_kernel(const double* __restrict__ L, int64_t ld_l, int Tl, const double* __restrict__ Q,
                                                            int64_t ld_q, int ny, int nx, const double* __restrict__ wuse, int k, int ry, int rx,
                                                            const int32_t* __restrict__ idx, int32_t* __restrict__ lidx,
                                                            double* __restrict__ ldist) {
    extern __shared__ double lds[];
    const int Cc = ny * nx, tid = threadIdx.x;
    double* const Qs = lds;        // [Cc] the target
    double* const Ds = lds + Cc;   // [Cc] the terms of the analog at hand
    const int64_t q = blockIdx.x;
    const int32_t* const iq = idx + q * k;  // (uniform: scalar loads)
    bool ok = true;
    for (int a = 0; a < k; ++a) ok = ok && iq[a] >= 0 && iq[a] < Tl;
    if (!ok) {  // (uniform) no analogs: any status other than OK
        for (int c = tid; c < Cc; c += kLocBlock) lidx[q * Cc + c] = -1, ldist[q * Cc + c] = ca_nan();
        return;
    }
    for (int c = tid; c < Cc; c += kLocBlock) Qs[c] = Q[q * ld_q + c];
    double bd[kLocPerThread];
    int ba[kLocPerThread];
#pragma unroll
    for (int s = 0; s < kLocPerThread; ++s) bd[s] = 0.0, ba[s] = 0;
    for (int a = 0; a < k; ++a) {
        const double* const row = L + (int64_t)iq[a] * ld_l;
        __syncthreads();  // (Qs is written; the last analog's terms are consumed)
        for (int c = tid; c < Cc; c += kLocBlock) {
            const double w = wuse[c];  // wc of a used column, 0 of any other
            double term = 0.0;
            if (w > 0.0) {
                const double e = Qs[c] - row[c];
                term = w * (e * e);
            }
            Ds[c] = term;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kLocPerThread; ++s) {
            const int c = tid + s * kLocBlock;
            if (c < Cc) {
                const int i = c / nx, j = c - i * nx;
                const int i1 = min(ny - 1, i + ry), j0 = max(0, j - rx), j1 = min(nx - 1, j + rx);
                double dl = 0.0;
                for (int ii = max(0, i - ry); ii <= i1; ++ii)
                    for (int jj = j0; jj <= j1; ++jj) dl = dl + Ds[ii * nx + jj];
                if (a == 0 || dl < bd[s]) bd[s] = dl, ba[s] = a;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kLocPerThread; ++s) {
        const int c = tid + s * kLocBlock;
        if (c < Cc) lidx[q * Cc + c] = iq[ba[s]], ldist[q * Cc + c] = bd[s];
    }
}

template <typename S>
__global__ void __launch_bounds__(kLapBlock) ca_local_apply_kernel(const S* __restrict__ F, int64_t ld_f, int Tl, int64_t Cf,
                                                                  const int32_t* __restrict__ cell_of, const int32_t* __restrict__ lidx, int Cc,
                                                                  const double* __restrict__ L, int64_t ld_l, const double* __restrict__ Q,
                                                                  int64_t ld_q, int adjust, double max_scale, int64_t q0, int64_t q1,
                                                                  int64_t ctiles, double* __restrict__ out, int64_t ld_out) {
    const int64_t tile = blockIdx.x % ctiles, rg = blockIdx.x / ctiles;
    const int64_t f = tile * kLapCells + threadIdx.x;
    if (f >= Cf) return;  // (no barrier below)
    const int32_t cell = cell_of[f];
    const bool inside = cell >= 0 && cell < Cc;
    const int c = inside ? cell : 0;  // (a cell outside the coarse grid reads column 0 and stores NaN)
    const int64_t qa = q0 + rg * kLapRows, qb = min(qa + kLapRows, q1);
    for (int64_t qs = qa; qs < qb; qs += kLapBatch) {
        int32_t t[kLapBatch];
        bool has[kLapBatch];
        double v[kLapBatch], qv[kLapBatch], lv[kLapBatch];
#pragma unroll
        for (int u = 0; u < kLapBatch; ++u) {
            const int64_t q = min(qs + u, qb - 1);  // (a row past the end reads the last one again and stores nothing)
            const int32_t day = lidx[q * Cc + c];
            has[u] = inside && day >= 0 && day < Tl;
            t[u] = has[u] ? day : 0;
        }
#pragma unroll
        for (int u = 0; u < kLapBatch; ++u) v[u] = (double)F[(int64_t)t[u] * ld_f + f];
        if (adjust != SD_CA_ADJUST_NONE) {  // (uniform)
#pragma unroll
            for (int u = 0; u < kLapBatch; ++u) {
                const int64_t q = min(qs + u, qb - 1);
                qv[u] = Q[q * ld_q + c], lv[u] = L[(int64_t)t[u] * ld_l + c];
            }
        }
#pragma unroll
        for (int u = 0; u < kLapBatch; ++u) {
            double r = v[u];
            if (adjust == SD_CA_ADJUST_SHIFT) {
                r = v[u] + (qv[u] - lv[u]);
            } else if (adjust == SD_CA_ADJUST_SCALE) {
                double ratio = lv[u] > 0.0 ? qv[u] / lv[u] : 1.0;
                if (max_scale > 0.0 && ratio > max_scale) ratio = max_scale;
                r = v[u] * ratio;
            }
            if (qs + u < qb) out[(qs + u - q0) * ld_out + f] = has[u] ? r : ca_nan();
        }
    }
}

}  // namespace

extern "C" {

int sd_ca_local_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t ny,
                    int64_t nx, const double* wc, int k, int64_t ry, int64_t rx, const int32_t* idx_dev, int32_t* local_idx_dev,
                    double* local_dist_dev) {
    SD_CHECK_ARG(ctx && L_dev && Q_dev && wc && idx_dev && local_idx_dev && local_dist_dev, "sd_ca_local: NULL argument");
    CaLocalCall c;
    c.Tl = Tl, c.Tq = Tq, c.ny = ny, c.nx = nx, c.ld_l = ld_l, c.ld_q = ld_q, c.ry = ry, c.rx = rx, c.k = k, c.wc = wc;
    const CaLocalPlan pl = ca_local_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    const int64_t Cc = ny * nx;
    std::vector<int32_t> used;
    SD_TRY(ca_column_flags(ctx, "sd_ca_local", L_dev, ld_l, Tl, Cc, wc, used));
    std::vector<double> wuse((size_t)Cc);
    for (int64_t i = 0; i < Cc; ++i) wuse[(size_t)i] = used[(size_t)i] != 0 ? wc[i] : 0.0;
    sd_scratch wuse_dev;
    SD_TRY(upload(ctx, wuse_dev, wuse));
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    SD_LAUNCH(ctx, "ca_local_kernel", ca_local_kernel, grid, block, (size_t)pl.lds_bytes, L_dev, ld_l, (int)Tl, Q_dev, ld_q, (int)ny, (int)nx,
              (const double*)wuse_dev.p, k, pl.ry, pl.rx, idx_dev, local_idx_dev, local_dist_dev);
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the tables go away on return)
    return SD_OK;
}

int sd_ca_local_apply_dev(sd_ctx* ctx, const void* F_dev, int f_is_f32, int64_t ld_f, int64_t Tl, int64_t Cf, const int32_t* cell_of_dev,
                          const int32_t* local_idx_dev, int64_t Cc, const double* L_dev, int64_t ld_l, const double* Q_dev, int64_t ld_q,
                          int adjust, double max_scale, int64_t Tq, int64_t q0, int64_t q1, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && F_dev && cell_of_dev && local_idx_dev && out_dev, "sd_ca_local_apply: NULL argument");
    CaLocalApplyCall c;
    c.Tl = Tl, c.Cf = Cf, c.ld_f = ld_f, c.Cc = Cc, c.ld_l = ld_l, c.ld_q = ld_q, c.Tq = Tq, c.q0 = q0, c.q1 = q1, c.ld_out = ld_out;
    c.adjust = adjust, c.max_scale = max_scale, c.has_coarse = L_dev != nullptr && Q_dev != nullptr;
    const CaLocalPlan pl = ca_local_apply_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    if (f_is_f32 != 0)
        SD_LAUNCH(ctx, "ca_local_apply_kernel", ca_local_apply_kernel<float>, grid, block, 0, (const float*)F_dev, ld_f, (int)Tl, Cf, cell_of_dev,
                  local_idx_dev, (int)Cc, L_dev, ld_l, Q_dev, ld_q, adjust, max_scale, q0, q1, pl.ctiles, out_dev, ld_out);
    else
        SD_LAUNCH(ctx, "ca_local_apply_kernel", ca_local_apply_kernel<double>, grid, block, 0, (const double*)F_dev, ld_f, (int)Tl, Cf, cell_of_dev,
                  local_idx_dev, (int)Cc, L_dev, ld_l, Q_dev, ld_q, adjust, max_scale, q0, q1, pl.ctiles, out_dev, ld_out);
    return SD_OK;
}

}  // extern "C"
