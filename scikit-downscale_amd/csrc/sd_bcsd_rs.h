// Register-sort BCSD paths (sd_bcsd_fx.hip: one fused kernel per segment; sd_bcsd_rs.hip: the
// RANK / APPLY / FIT kernels): parameters and launchers.
#pragma once
#include "sd_bcsd_plan.h"
#include "sd_internal.h"

namespace sdrs {

// MODE_RANK + MODE_APPLY = fit+predict (or predict from a state) as two kernels: RANK ranks every x_fut sample
// within its shifted segment by an explicit search, APPLY sorts y_obs (or reads the fitted state), maps the ranks and
// restores the shift.  They serve BcsdPrecipitation, and every BcsdTemperature segment the fused kernel hands back
// (work list).  MODE_FIT = the y side alone, writing the fitted state.
enum { MODE_FIT = 0, MODE_RANK = 3, MODE_APPLY = 4 };

struct Params {
    int kind, G, return_anoms, RS;
    int64_t C, Tf, ntiles;
    const double* X; const double* y; int64_t ld;    // fit fields [Tf, ld]
    const double* Xp; int64_t ld_p;                    // predict field [Tp, ld_p]
    double* out; int64_t ld_out;
    const int32_t* ord_f; const int32_t* off_f;        // fit group table
    const int32_t* ord_p; const int32_t* off_p;        // predict group table
    const int32_t* qidx; const double* qval;           // inverse-CDF tables, indexed off_p[g] + rank
    double* ys; double* x_climo; double* y_climo;      // state: [C][Tf], [C][G], [C][G]
    int32_t* status_fit; int32_t* status_p;
    uint32_t* ranks;                                   // RANK -> APPLY: [C*G][(K+1)/2][64] packed 16-bit ranks
    double* shift;                                     // [C*G][K][64] rolling mean - x_climo of every sample (lane layout)
    int from_state;  // 1 = predict from a fitted state (x_climo, y_climo, ys given), 0 = fit on the fly from X, y
    int identity;    // 1: every group has equal fit / predict length (inverse CDF = identity on ranks)
    long long* trace;  // SD_RS_TRACING builds: per-phase wall-clock stamps of sampled workgroups
    // set from the plan's record: groups served by this launch (0 = all; bit g otherwise) and the per-segment strides of the
    // hand-off slabs (those of the widest kernel of the call, so that launches of different widths share the slabs)
    unsigned long long gmask;
    int slab_nr, slab_k;
    // Work list of (tile, group) items = tile * G + group.  The fused kernel appends the items it cannot serve
    // (tied samples, see sd_bcsd_fx.hip); RANK / APPLY launched with use_worklist walk the list with a
    // fixed grid instead of covering every (tile, group).
    int64_t* worklist;
    int* work_count;  // device counter (items appended, may exceed work_cap: the excess is lost and reported)
    int work_cap;
    int use_worklist;
    // second list of the compacting precipitation kernel (segments with too many wet days for its narrow sort): served by
    // bcsd_fxp_kernel<K, true, true> launched with use_worklist = 2
    int64_t* worklist2;
    int* work_count2;
    // QuantileMapper(detrend=True) (quantile.py:95-98, 128-145): both series lose their least-squares line over the sample
    // index before the CDFs; the predict line comes back afterwards, re-based on the fitted intercept.  RANK / APPLY / FIT
    // only (the fused kernel is bypassed).
    int detrend;
    double* trend_u;       // RANK -> APPLY: [C*G][2] slope, intercept of the predict segment's line
    double* y_trend;       // state [C][G][2]: slope, intercept of the fitted segment's line
    int n_endpoints;  // points of the OLS tail lines (quantile.py:426, 537-541); 0 is taken as the default 10 (sd_bcsd.hip: call_params)
    int dev_flags;  // development library only (SD_FZ_ABLATE): phases skipped to time the rest; results are then wrong
    // request row tables of the LDS-DMA kernel, [G][tmj::kTabInts] next to ord_f / ord_p (sd_bcsd_plan.h: build_row_tables); nullptr
    // where the group table has none (explicit tables, or no group of a length that kernel serves)
    const int32_t* rtab_f; const int32_t* rtab_p;
};

}  // namespace sdrs

// workspace bytes of the RANK -> APPLY hand-off slabs (both multiples of 256)
void sd_bcsd_rs_handoff_bytes(int nmax, int64_t C, int G, size_t* rank_bytes, size_t* shift_bytes);
// The launch a record of the call's plan (sd_bcsd_plan.h) names: sd_bcsd_rs.hip serves RsFit / RsRank / RsApply, sd_bcsd_fx.hip
// the fused kernels (x side, y side, inverse CDF and shift / ratio of a segment in one workgroup pass on the register-resident
// 32-bit key sort of sd_wsort.h; segments they cannot serve are appended to p.worklist for RANK + APPLY).  p: the call's common
// fields; the record sets gmask, RS, use_worklist and the slab strides.
int sd_bcsd_rs_run(sd_ctx* ctx, const BcsdLaunch& L, const sdrs::Params& p);
int sd_bcsd_fx_run(sd_ctx* ctx, const BcsdLaunch& L, const sdrs::Params& p);
// development library (SD_FX_TRACE): phase clocks of the sampled workgroups of the fused kernels to a file; a no-op otherwise
int sd_bcsd_fx_trace(sd_ctx* ctx);
