// Constructed analogs (ConstructedAnalogs; Hidalgo et al. 2008, Maurer et al. 2010): for each target day the k library days whose coarse
// pattern is closest, the regression of the target pattern on those k patterns, and the k weights applied to the fine fields of the same
// days.  The rule is stated in include/sd_downscale.h and restated by tests/_constructed_oracle.py; the launch plans and the tile
// constants are in sd_constructed_plan.h.
//
// ca_columns_kernel (sd_constructed_cols.h, shared with sd_localized.hip): one thread per coarse column says whether the column is used.
// The flags come back to the host, which makes the ascending list of used columns (at most 2^16 ints; the only host round trip).
//
// ca_select_kernel: a workgroup of 256 threads owns kSelQ = 8 targets and sweeps the library in tiles of kSelL = 128 days.  The used
// columns of both are staged kSelCols = 32 at a time in LDS, column-major, so that a thread reads its 4 library days as two 16-byte LDS
// loads and its target as a broadcast.  Each thread holds a 1 x 4 register tile of accumulators; an accumulator adds its columns in
// ascending order, so the fixed order of the rule is free.  After a library tile the distances go to LDS and each wave merges them into
// the k-lists of its 2 targets: lane i of the wave holds entry i of the list, sorted by (d, t), the unused entries (+inf, INT32_MAX); a
// candidate that is not smaller than entry k - 1 is rejected by one comparison, a survivor is inserted by a ballot (its position) and a
// shift by one lane.  The list is the exact set of the k smallest (d, t) whatever the tiles: nothing depends on the geometry.  The
// [Tq, Tl] distance matrix never leaves the chip.  3 * Tq * Tl * nu float64 operations beside the (e * e) product.
//
// ca_weights_kernel: one workgroup per target.  The k analog rows are staged kWgtCols = 64 used columns at a time; the up to 528 entries
// of the lower triangle of G and the 32 of b are spread over the threads, each summed sequentially over the columns.  The Cholesky
// factor is made in LDS column by column by all threads -- every element still sees its products subtracted in ascending index order,
// so the bits are those of the row-by-row form of the rule -- and one thread runs the two substitutions.
//
// ca_apply_kernel<S>: the memory side, Tq * k * Cf fine samples read for Tq * Cf written.  A workgroup of 4 waves owns 64 consecutive
// cells and 32 targets, 8 per wave; idx and weights of a target are wave-uniform (scalar loads), the k row segments are read coalesced,
// 8 loads in flight before their arithmetic.  The workgroup ids of one XCD (every kXcds-th id) walk the row groups of one cell tile before
// the next tile: the workgroups in flight share few cell tiles, which keeps the slab of the library they gather from
// (Tl * cells in flight * itemsize) small.  Floor: Tl * Cf * itemsize + 8 * Tq * Cf bytes; profiles/constructed_analogs/ has what is reached.
#include <algorithm>
#include <vector>

#include "sd_constructed_cols.h"
#include "sd_constructed_plan.h"
#include "sd_internal.h"
#include "sd_state.h"

namespace {
using namespace sdca;

// (d, t) < (e, u) in lexicographic order
__device__ __forceinline__ bool ca_less(double d, int32_t t, double e, int32_t u) { return d < e || (d == e && t < u); }

__global__ void __launch_bounds__(kSelBlock) ca_select_kernel(const double* __restrict__ L, int64_t ld_l, int Tl, const double* __restrict__ Q,
                                                             int64_t ld_q, int64_t Tq, const int32_t* __restrict__ cols,
                                                             const double* __restrict__ wcu, int nu, int k, const int32_t* __restrict__ key_l,
                                                             const int32_t* __restrict__ key_q, int64_t period, int64_t window,
                                                             const int32_t* __restrict__ excl_l, const int32_t* __restrict__ excl_q,
                                                             int32_t* __restrict__ idx, double* __restrict__ dist, int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) double Ls[kSelCols][kSelL + kSelPad];
    __shared__ double Qs[kSelCols][kSelQ];
    __shared__ double Ws[kSelCols];
    __shared__ double Dt[kSelQ][kSelL];
    __shared__ int32_t bad[kSelQ];
    static_assert(sizeof(Ls) + sizeof(Qs) + sizeof(Ws) + sizeof(Dt) + sizeof(bad) == sel_lds_bytes(), "the plan's LDS bytes");
    constexpr int kWavesSel = kSelBlock / kLanes, kQPerWave = kSelQ / kWavesSel;
    const int tid = threadIdx.x, lane = tid % kLanes, wave = __builtin_amdgcn_readfirstlane(tid / kLanes);
    const int tt = tid % (kSelL / kSelLPerThread), tq = tid / (kSelL / kSelLPerThread);
    const int64_t q0 = (int64_t)blockIdx.x * kSelQ;

    // a used column of a target that is not finite
    if (tid < kSelQ) bad[tid] = 0;
    __syncthreads();
    for (int e = tid; e < kSelQ * nu; e += kSelBlock) {
        const int qi = e / nu, c = e % nu;
        if (!ca_finite(Q[min(q0 + qi, Tq - 1) * ld_q + cols[c]])) bad[qi] = 1;
    }
    // the k-lists of this wave's targets: lane i holds entry i
    double ld[kQPerWave];
    int32_t lt[kQPerWave];
#pragma unroll
    for (int u = 0; u < kQPerWave; ++u) ld[u] = ca_inf(), lt[u] = INT32_MAX;

    for (int t0 = 0; t0 < Tl; t0 += kSelL) {
        double acc[kSelQPerThread][kSelLPerThread];
#pragma unroll
        for (int a = 0; a < kSelQPerThread; ++a)
#pragma unroll
            for (int b = 0; b < kSelLPerThread; ++b) acc[a][b] = 0.0;
        for (int c0 = 0; c0 < nu; c0 += kSelCols) {
            const int kn = min(kSelCols, nu - c0);
            __syncthreads();  // (the last step's columns are consumed)
            for (int e = tid; e < kSelL * kSelCols; e += kSelBlock) {
                const int kc = e % kSelCols, t = e / kSelCols;  // (a day past the end reads the last one again and is no candidate)
                if (kc < kn) Ls[kc][t] = L[(int64_t)min(t0 + t, Tl - 1) * ld_l + cols[c0 + kc]];
            }
            for (int e = tid; e < kSelQ * kSelCols; e += kSelBlock) {
                const int kc = e % kSelCols, qi = e / kSelCols;
                if (kc < kn) Qs[kc][qi] = Q[min(q0 + qi, Tq - 1) * ld_q + cols[c0 + kc]];
            }
            if (tid < kn) Ws[tid] = wcu[c0 + tid];
            __syncthreads();
#pragma unroll 4
            for (int kc = 0; kc < kn; ++kc) {
                const double w = Ws[kc];
                double qv[kSelQPerThread], lv[kSelLPerThread];
#pragma unroll
                for (int a = 0; a < kSelQPerThread; ++a) qv[a] = Qs[kc][tq * kSelQPerThread + a];
#pragma unroll
                for (int b = 0; b < kSelLPerThread; b += 2) {
                    const double2 p = *reinterpret_cast<const double2*>(&Ls[kc][tt * kSelLPerThread + b]);
                    lv[b] = p.x, lv[b + 1] = p.y;
                }
#pragma unroll
                for (int a = 0; a < kSelQPerThread; ++a)
#pragma unroll
                    for (int b = 0; b < kSelLPerThread; ++b) {
                        const double e = qv[a] - lv[b];
                        acc[a][b] += w * (e * e);
                    }
            }
        }
#pragma unroll
        for (int a = 0; a < kSelQPerThread; ++a)
#pragma unroll
            for (int b = 0; b < kSelLPerThread; ++b) Dt[tq * kSelQPerThread + a][tt * kSelLPerThread + b] = acc[a][b];
        __syncthreads();
        // merge: the next tile writes Dt only behind the barriers of its column steps
#pragma unroll
        for (int u = 0; u < kQPerWave; ++u) {
            const int qi = wave * kQPerWave + u;
            const int64_t q = q0 + qi;
            if (q >= Tq || bad[qi] != 0) continue;  // (wave-uniform)
            const int64_t a = key_q[q];
            const int32_t xq = excl_q[q];
            for (int h = 0; h < kSelL; h += kLanes) {
                const int t = t0 + h + lane;
                bool cand = t < Tl;
                if (cand) {
                    const int64_t diff = a > key_l[t] ? a - key_l[t] : key_l[t] - a;
                    cand = (window < 0 || min(diff, period - diff) <= window) && (xq < 0 || excl_l[t] != xq);
                }
                const double d = Dt[qi][h + lane];
                // (the worst entry is read by every lane, not behind `cand &&`: a lane that skips the shuffle cannot be read from)
                const double kd = __shfl(ld[u], k - 1);
                const int32_t kt = __shfl(lt[u], k - 1);
                const bool survives = cand && ca_less(d, t, kd, kt);
                unsigned long long todo = __ballot(survives);
                while (todo != 0) {  // in ascending t
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const double xd = __shfl(d, src);
                    const int32_t xt = __shfl(t, src);
                    const int pos = __popcll(__ballot(lane < k && ca_less(ld[u], lt[u], xd, xt)));
                    const double pd = __shfl_up(ld[u], 1);
                    const int32_t pt = __shfl_up(lt[u], 1);
                    if (lane < k) {
                        if (lane == pos) ld[u] = xd, lt[u] = xt;
                        else if (lane > pos) ld[u] = pd, lt[u] = pt;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kQPerWave; ++u) {
        const int qi = wave * kQPerWave + u;
        const int64_t q = q0 + qi;
        if (q >= Tq) continue;
        const int n = __popcll(__ballot(lane < k && lt[u] != INT32_MAX));
        const int32_t st = bad[qi] != 0 ? SD_CA_QUERY_NONFINITE : n < k ? SD_CA_FEW_CANDIDATES : SD_CA_OK;
        if (lane < k) {
            idx[q * k + lane] = st == SD_CA_OK ? lt[u] : -1;
            dist[q * k + lane] = st == SD_CA_OK ? ld[u] : ca_nan();
        }
        if (lane == 0) status[q] = st;
    }
}

__global__ void __launch_bounds__(kWgtBlock) ca_weights_kernel(const double* __restrict__ L, int64_t ld_l, int Tl, const double* __restrict__ Q,
                                                              int64_t ld_q, const int32_t* __restrict__ cols, const double* __restrict__ wcu,
                                                              int nu, int k, int kind, double ridge, int32_t* __restrict__ idx,
                                                              double* __restrict__ dist, double* __restrict__ weights,
                                                              int32_t* __restrict__ status) {
    __shared__ double A[kMaxK][kWgtCols + 1];
    __shared__ double Qc[kWgtCols], Wc[kWgtCols];
    __shared__ double G[kMaxK][kMaxK + 1];  // the lower triangle: G, then the Cholesky factor in place
    __shared__ double bv[kMaxK], yv[kMaxK], wv[kMaxK];
    __shared__ int32_t rows[kMaxK];
    __shared__ int32_t flag;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const auto give_up = [&](int32_t st) {  // (uniform)
        if (tid < k) weights[q * k + tid] = ca_nan(), idx[q * k + tid] = -1, dist[q * k + tid] = ca_nan();
        if (tid == 0) status[q] = st;
    };
    const int32_t st = status[q];
    if (st != SD_CA_OK) return give_up(st);
    if (tid == 0) flag = 0;
    __syncthreads();
    if (tid < k) {
        rows[tid] = idx[q * k + tid];
        if (rows[tid] < 0 || rows[tid] >= Tl) flag = 1;  // (not a table of sd_ca_select_dev: no such day)
    }
    __syncthreads();
    if (flag != 0) return give_up(SD_CA_FEW_CANDIDATES);
    if (kind == SD_CA_MEAN) {
        if (tid < k) weights[q * k + tid] = 1.0 / (double)k;
        return;
    }
    // the sums of this thread: entry e of the lower triangle row by row, then b
    const int ntri = k * (k + 1) / 2, nent = ntri + k;
    int ei[kWgtPerThread], ej[kWgtPerThread];
    double acc[kWgtPerThread];
#pragma unroll
    for (int s = 0; s < kWgtPerThread; ++s) {
        const int e = tid + s * kWgtBlock;
        acc[s] = 0.0, ei[s] = -1, ej[s] = -1;
        if (e < ntri) {
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= e) ++i;
            ei[s] = i, ej[s] = e - i * (i + 1) / 2;
        } else if (e < nent) {
            ei[s] = e - ntri;
        }
    }
    for (int c0 = 0; c0 < nu; c0 += kWgtCols) {
        const int kn = min(kWgtCols, nu - c0);
        __syncthreads();
        for (int e = tid; e < k * kWgtCols; e += kWgtBlock) {
            const int kc = e % kWgtCols, i = e / kWgtCols;
            if (kc < kn) A[i][kc] = L[(int64_t)rows[i] * ld_l + cols[c0 + kc]];
        }
        if (tid < kn) Qc[tid] = Q[q * ld_q + cols[c0 + tid]], Wc[tid] = wcu[c0 + tid];
        __syncthreads();
        for (int kc = 0; kc < kn; ++kc) {
            const double w = Wc[kc];
#pragma unroll
            for (int s = 0; s < kWgtPerThread; ++s)
                if (ei[s] >= 0) acc[s] += w * (A[ei[s]][kc] * (ej[s] >= 0 ? A[ej[s]][kc] : Qc[kc]));
        }
    }
#pragma unroll
    for (int s = 0; s < kWgtPerThread; ++s)
        if (ei[s] >= 0) {
            if (ej[s] >= 0) G[ei[s]][ej[s]] = acc[s];
            else bv[ei[s]] = acc[s];
        }
    __syncthreads();
    if (tid == 0) {
        double trace = G[0][0];
        for (int i = 1; i < k; ++i) trace += G[i][i];
        const double lambda = ridge * (trace / (double)k);
        for (int i = 0; i < k; ++i) G[i][i] += lambda;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kWgtPerThread; ++s)
        if (ej[s] >= 0) acc[s] = G[ei[s]][ej[s]];
    // the factor column by column: element (i, j) has had C[i][p] * C[j][p] subtracted for p = 0 .. j - 1 in ascending order when
    // column j is finished
    for (int p = 0; p < k; ++p) {
#pragma unroll
        for (int s = 0; s < kWgtPerThread; ++s)
            if (ej[s] == p && ei[s] == p) {
                if (acc[s] > 0.0) G[p][p] = sqrt(acc[s]);
                else flag = 1;
            }
        __syncthreads();
        if (flag != 0) break;  // (uniform)
#pragma unroll
        for (int s = 0; s < kWgtPerThread; ++s)
            if (ej[s] == p && ei[s] > p) G[ei[s]][p] = acc[s] / G[p][p];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kWgtPerThread; ++s)
            if (ej[s] > p) acc[s] -= G[ei[s]][p] * G[ej[s]][p];
    }
    if (flag != 0) return give_up(SD_CA_SINGULAR);
    if (tid == 0) {
        for (int i = 0; i < k; ++i) {
            double s = bv[i];
            for (int p = 0; p < i; ++p) s -= G[i][p] * yv[p];
            yv[i] = s / G[i][i];
        }
        for (int i = k - 1; i >= 0; --i) {
            double s = yv[i];
            for (int p = i + 1; p < k; ++p) s -= G[p][i] * wv[p];
            wv[i] = s / G[i][i];
        }
    }
    __syncthreads();
    if (tid < k) weights[q * k + tid] = wv[tid];
}

template <typename S>
__global__ void __launch_bounds__(kAppBlock) ca_apply_kernel(const S* __restrict__ F, int64_t ld_f, int Tl, int64_t Cf,
                                                            const int32_t* __restrict__ idx, const double* __restrict__ weights, int k,
                                                            int64_t q0, int64_t q1, int64_t row_groups, double* __restrict__ out,
                                                            int64_t ld_out) {
    constexpr int kRowsPerWave = kAppRows / kAppWaves;
    const int lane = threadIdx.x % kLanes, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const int64_t slot = blockIdx.x / kXcds;  // (the ids of one XCD: the row groups of one cell tile, then the next tile's)
    const int64_t rg = slot % row_groups, tile = slot / row_groups * kXcds + blockIdx.x % kXcds;
    if (tile * kAppCells >= Cf) return;  // (the padding of the last round of tiles)
    const int64_t f = tile * kAppCells + lane;
    const bool active = f < Cf;
    const S* const col = F + (active ? f : Cf - 1);  // (a lane past the end reads the last cell again and stores nothing)
    const int64_t qa = q0 + rg * kAppRows + (int64_t)wave * kRowsPerWave;
    for (int64_t q = qa; q < min(qa + kRowsPerWave, q1); ++q) {
        const int32_t* const iq = idx + q * k;  // (wave-uniform: scalar loads)
        const double* const wq = weights + q * k;
        bool inside = true;
        for (int i = 0; i < k; ++i) inside = inside && iq[i] >= 0 && iq[i] < Tl;
        double acc = 0.0;
        if (!inside) {
            acc = ca_nan();
        } else {
            for (int i0 = 0; i0 < k; i0 += kAppBatch) {
                double v[kAppBatch];
#pragma unroll
                for (int u = 0; u < kAppBatch; ++u) v[u] = (double)col[(int64_t)iq[min(i0 + u, k - 1)] * ld_f];
#pragma unroll
                for (int u = 0; u < kAppBatch; ++u)
                    if (i0 + u < k) acc += wq[i0 + u] * v[u];
            }
        }
        if (active) out[(q - q0) * ld_out + f] = acc;
    }
}

// the used columns of a call: ascending indices and their weights on the device
struct CaColumns {
    sd_scratch cols, wcu;
    int nu = 0;
};

int ca_used_columns(sd_ctx* ctx, const char* who, const double* L_dev, int64_t ld_l, int64_t Tl, int64_t Cc, const double* wc, CaColumns& u) {
    std::vector<int32_t> used;
    SD_TRY(ca_column_flags(ctx, who, L_dev, ld_l, Tl, Cc, wc, used));
    std::vector<int32_t> cols;
    std::vector<double> wcu;
    for (int64_t c = 0; c < Cc; ++c)
        if (used[(size_t)c] != 0) cols.push_back((int32_t)c), wcu.push_back(wc[c]);
    u.nu = (int)cols.size();
    SD_TRY(upload(ctx, u.cols, cols));
    SD_TRY(upload(ctx, u.wcu, wcu));
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the host tables go away on return)
    return SD_OK;
}

CaCoarse coarse_of(int64_t ld_l, int64_t Tl, int64_t ld_q, int64_t Tq, int64_t Cc, const double* wc, int k) {
    CaCoarse c;
    c.Tl = Tl, c.Tq = Tq, c.Cc = Cc, c.ld_l = ld_l, c.ld_q = ld_q, c.k = k, c.wc = wc;
    return c;
}

}  // namespace

extern "C" {

int sd_ca_select_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t Cc,
                     const double* wc, int k, const int32_t* key_l, const int32_t* key_q, int64_t period, int64_t window,
                     const int32_t* excl_l, const int32_t* excl_q, int32_t* idx_dev, double* dist_dev, int32_t* status_dev) {
    SD_CHECK_ARG(ctx && L_dev && Q_dev && wc && key_l && key_q && excl_l && excl_q && idx_dev && dist_dev && status_dev,
                 "sd_ca_select: NULL argument");
    const CaPlan pl = ca_select_plan(coarse_of(ld_l, Tl, ld_q, Tq, Cc, wc, k), period, window);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    CaColumns u;
    SD_TRY(ca_used_columns(ctx, "sd_ca_select", L_dev, ld_l, Tl, Cc, wc, u));
    sd_scratch kl, kq, xl, xq;
    SD_TRY(upload(ctx, kl, std::vector<int32_t>(key_l, key_l + Tl)));
    SD_TRY(upload(ctx, kq, std::vector<int32_t>(key_q, key_q + Tq)));
    SD_TRY(upload(ctx, xl, std::vector<int32_t>(excl_l, excl_l + Tl)));
    SD_TRY(upload(ctx, xq, std::vector<int32_t>(excl_q, excl_q + Tq)));
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the temporaries above are gone after this statement's full expression)
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    SD_LAUNCH(ctx, "ca_select_kernel", ca_select_kernel, grid, block, 0, L_dev, ld_l, (int)Tl, Q_dev, ld_q, Tq, (const int32_t*)u.cols.p,
              (const double*)u.wcu.p, u.nu, k, (const int32_t*)kl.p, (const int32_t*)kq.p, period, window, (const int32_t*)xl.p,
              (const int32_t*)xq.p, idx_dev, dist_dev, status_dev);
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the tables go away on return)
    return SD_OK;
}

int sd_ca_weights_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t Cc,
                      const double* wc, int k, int kind, double ridge, int32_t* idx_dev, double* dist_dev, double* weights_dev,
                      int32_t* status_dev) {
    SD_CHECK_ARG(ctx && L_dev && Q_dev && wc && idx_dev && dist_dev && weights_dev && status_dev, "sd_ca_weights: NULL argument");
    const CaPlan pl = ca_weights_plan(coarse_of(ld_l, Tl, ld_q, Tq, Cc, wc, k), kind, ridge);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    CaColumns u;
    SD_TRY(ca_used_columns(ctx, "sd_ca_weights", L_dev, ld_l, Tl, Cc, wc, u));
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    SD_LAUNCH(ctx, "ca_weights_kernel", ca_weights_kernel, grid, block, 0, L_dev, ld_l, (int)Tl, Q_dev, ld_q, (const int32_t*)u.cols.p,
              (const double*)u.wcu.p, u.nu, k, kind, ridge, idx_dev, dist_dev, weights_dev, status_dev);
    SD_HIP(hipStreamSynchronize(ctx->stream));  // (the tables go away on return)
    return SD_OK;
}

int sd_ca_apply_dev(sd_ctx* ctx, const void* F_dev, int f_is_f32, int64_t ld_f, int64_t Tl, int64_t Cf, const int32_t* idx_dev,
                    const double* weights_dev, int64_t Tq, int k, int64_t q0, int64_t q1, double* out_dev, int64_t ld_out) {
    SD_CHECK_ARG(ctx && F_dev && idx_dev && weights_dev && out_dev, "sd_ca_apply: NULL argument");
    CaApplyCall c;
    c.Tl = Tl, c.Cf = Cf, c.ld_f = ld_f, c.Tq = Tq, c.q0 = q0, c.q1 = q1, c.ld_out = ld_out, c.k = k;
    const CaPlan pl = ca_apply_plan(c);
    if (pl.error != SD_OK) return sd_set_error(pl.error, "%s", pl.message);
    SD_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)pl.blocks), block((unsigned)pl.block);
    if (f_is_f32 != 0)
        SD_LAUNCH(ctx, "ca_apply_kernel", ca_apply_kernel<float>, grid, block, 0, (const float*)F_dev, ld_f, (int)Tl, Cf, idx_dev, weights_dev, k,
                  q0, q1, pl.row_groups, out_dev, ld_out);
    else
        SD_LAUNCH(ctx, "ca_apply_kernel", ca_apply_kernel<double>, grid, block, 0, (const double*)F_dev, ld_f, (int)Tl, Cf, idx_dev, weights_dev, k,
                  q0, q1, pl.row_groups, out_dev, ld_out);
    return SD_OK;
}

}  // extern "C"
