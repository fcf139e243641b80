/* sd_downscale.h -- C ABI of the MI355X-native pointwise-downscaling engine.
 *
 * Drop-in boundary for scikit-downscale's per-grid-cell statistical hot path.  Every entry point
 * replaces a *batch over the cell axis* of one reference call (citations are file:line under
 * /root/reference/skdownscale/pointwise_models/):
 *
 *   sd_bcsd_fit*            <- core.py:86-96 looping BcsdTemperature.fit (bcsd.py:197-228) or
 *                              BcsdPrecipitation.fit (bcsd.py:115-147) over all cells
 *   sd_bcsd_predict*        <- core.py:137-141 looping BcsdTemperature.predict (bcsd.py:230-269) or
 *                              BcsdPrecipitation.predict (bcsd.py:149-185)
 *   sd_bcsd_fit_predict_dev <- both of the above fused (no persisted quantile state)
 *   sd_analog_fit*          <- AnalogBase.fit (gard.py:58-87)
 *   sd_analog_predict*      <- PureAnalog.predict (gard.py:273-364)
 *   sd_analogreg_predict*   <- AnalogRegression.predict, thresh=None (gard.py:152-224)
 *   sd_zscore_fit*          <- ZScoreRegressor.fit (zscore.py:32-69: _reshape / _calc_stats / _get_params, 123-238)
 *   sd_zscore_predict*      <- ZScoreRegressor.predict (zscore.py:71-112: _get_fut_stats / _expand_params /
 *                              _correct_fut_stats, 241-354)
 *   sd_zscore_state_*       <- the fitted shift_ / scale_ / fit_stats_dict_ (zscore.py:24, 56-67)
 *   sd_grouped_fit*         <- GroupedRegressor.fit with LinearRegression as estimator (grouping.py:53-80) on the groups of
 *                              grouping.PaddedDOYGrouper (grouping.py:106-138), or on disjoint groups (window = 0)
 *   sd_grouped_predict*     <- GroupedRegressor.predict (grouping.py:82-103): the model of each sample's own key
 *   sd_grouped_state_*      <- the fitted estimators_ (coef_, intercept_ of every group; grouping.py:74)
 *   sd_arrm_fit*            <- PiecewiseLinearRegression(fit_option='arrm').fit (arrm.py:144-167): arrm_breakpoints
 *                              (arrm.py:19-105) and pwlf's fit_with_breaks (degree 1) on them
 *   sd_arrm_predict*        <- PiecewiseLinearRegression.predict (arrm.py:169-177)
 *   sd_arrm_state_*         <- fit_breaks_ and the numbers of model_ (beta, ssr)
 *
 * Conventions
 *   - Plain pointers and sizes only.  All fields are float64, time-major with the cell axis
 *     fastest: X[t*ld + c] (the layout core.py:427-440 `_to_feature_x` produces), feature arrays
 *     X[(t*F + f)*ld + c].  `ld` >= C is the row stride in elements (host variants: ld == C).
 *   - `group_id[t]` in [0,G) is the time group (calendar month - 1, groupers.py:11-12); it is the
 *     same for every cell and always lives in HOST memory.
 *   - Host variants (`sd_xxx`) take host pointers and copy in/out; `_dev` variants take device
 *     pointers (HBM-resident fields) and never touch PCIe.  No pointer is retained after a call
 *     returns; persistent state lives behind opaque handles owned by the library.
 *   - Every function returns SD_OK (0) or an SD_ERR_* code; sd_last_error() gives the
 *     thread-local message.  Per-cell conditions (masked / non-finite / bad climatology) are not
 *     errors of the call: they are reported in `cell_status[C]` and the host raises like the
 *     reference does (base.py:18-20, bcsd.py:140-141, core.py:35-37).
 *   - A context is bound to one GPU and one HIP stream; calls on one context are serialised.
 */
#ifndef SD_DOWNSCALE_H
#define SD_DOWNSCALE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_VERSION 105  /* bump on every change of an exported signature: the Python loader refuses other versions */

/* return codes */
#define SD_OK 0
#define SD_ERR_INVALID 1     /* bad argument (NULL, size <= 0, group id out of range ...) */
#define SD_ERR_HIP 2         /* HIP runtime failure; message carries hipGetErrorString */
#define SD_ERR_UNSUPPORTED 3 /* valid request outside the engine's limits (e.g. segment too long) */
#define SD_ERR_NOMEM 4

/* BCSD variants */
#define SD_BCSD_TAS 0 /* BcsdTemperature */
#define SD_BCSD_PR 1  /* BcsdPrecipitation */

/* per-cell status */
#define SD_CELL_OK 0
#define SD_CELL_MASKED 1    /* core.py:35-37: first sample of X is NaN -> cell skipped, output NaN */
#define SD_CELL_NONFINITE 2 /* base.py:18-20: NaN/inf inside an active cell -> ValueError on host */
#define SD_CELL_BAD_CLIMO 3 /* bcsd.py:140-141: y climatology <= 0 with return_anoms */
#define SD_CELL_ONE_CLASS 4 /* gard.py:204-212: a thresholded regression met samples of one class only where the reference's
                             * LogisticRegression.fit raises -> ValueError on host */
#define SD_CELL_EMPTY_RANGE 5 /* arrm.py:95: the smallest upper pick of an ARRM fit is 6, so the lower picks would come from
                               * r2[:0] and the reference's np.argmin raises -> ValueError on host; no model for the cell */

/* PureAnalog kinds (gard.py:258-262) */
#define SD_ANALOG_BEST 0
#define SD_ANALOG_SAMPLE 1
#define SD_ANALOG_WEIGHT 2
#define SD_ANALOG_MEAN 3

/* quantile-mapping regressors (quantile.py:160-395, 556-636) */
#define SD_QM_REGRESSOR 0        /* QuantileMappingReressor */
#define SD_QM_EDCDF_DIFFERENCE 1 /* EquidistantCdfMatcher(kind='difference') */
#define SD_QM_EDCDF_RATIO 2      /* EquidistantCdfMatcher(kind='ratio') */

/* CunnaneTransformer (sd_qm_cunnane): direction and tail handling (quantile.py:424, 485-486, 527-528) */
#define SD_CUNNANE_FORWARD 0 /* transform: values -> plotting positions */
#define SD_CUNNANE_INVERSE 1 /* inverse_transform: plotting positions -> values */
#define SD_EXTRAP_NONE 0     /* extrapolate=None or '1to1': np.interp clamps at both ends */
#define SD_EXTRAP_MIN 1      /* lower tail extended */
#define SD_EXTRAP_MAX 2      /* upper tail extended */
#define SD_EXTRAP_BOTH 3
#define SD_EXTRAP_1TO1 4     /* regressors only: samples beyond the fitted X range keep their offset to it (quantile.py:277-310) */

/* synthetic field kinds (sd_synth_fill) */
/* sd_regrid_create: interpolation method */
#define SD_REGRID_LINEAR 0  /* interp_like(method='linear'): bilinear on a rectilinear grid, one dimension after the other */
#define SD_REGRID_NEAREST 1 /* method='nearest': a midpoint goes to the lower neighbour */

/* sd_resample: reduction over the rows of a bin */
#define SD_RESAMPLE_MEAN 0  /* NaN samples skipped; NaN for a bin without a sample */
#define SD_RESAMPLE_SUM 1   /* NaN samples skipped; 0 for a bin without a sample (pandas' min_count=0) */

/* sd_disagg: how the borrowed daily pattern of a month is brought to the monthly target */
#define SD_DISAGG_SHIFT 0      /* out = x + (target - mean of the borrowed month): temperature */
#define SD_DISAGG_SCALE_MEAN 1 /* out = x * (target / mean); a dry borrowed month gives target on every day: precipitation rates */
#define SD_DISAGG_SCALE_SUM 2  /* out = x * (target / sum); a dry borrowed month gives target / days on every day: precipitation totals */

/* sd_groupby_reduce: reduction over the rows of a group */
#define SD_GROUPBY_MEAN 0  /* NaN samples skipped; NaN for a group without a sample */
#define SD_GROUPBY_SUM 1   /* NaN samples skipped; 0 for a group without a sample (pandas' min_count=0) */
/* sd_groupby_apply: out = src (op) table[group] */
#define SD_GROUPBY_SUB 0
#define SD_GROUPBY_ADD 1
#define SD_GROUPBY_MUL 2
#define SD_GROUPBY_DIV 3

/* sd_rolling: statistic of a window of rows */
#define SD_ROLLING_MEAN 0  /* NaN samples skipped; NaN where fewer than min_periods samples, or none */
#define SD_ROLLING_SUM 1   /* NaN samples skipped; 0 for a window without a sample under min_periods == 0 */
#define SD_ROLLING_VAR 2   /* sum of squared deviations from the window's mean / (n - ddof); NaN where n - ddof <= 0 */
#define SD_ROLLING_STD 3   /* sqrt of SD_ROLLING_VAR */

/* sd_quantile: NumPy's estimation methods of np.nanquantile (h = (n - 1) * q over the n sorted non-NaN samples v) */
#define SD_QUANTILE_LINEAR 0    /* v[floor(h)] and its successor interpolated at h - floor(h) (NumPy's _lerp) */
#define SD_QUANTILE_LOWER 1     /* v[floor(h)] */
#define SD_QUANTILE_HIGHER 2    /* v[ceil(h)] */
#define SD_QUANTILE_NEAREST 3   /* v[rint(h)], half to even */
#define SD_QUANTILE_MIDPOINT 4  /* v[h] where h is whole, else the interpolation at 0.5 */
#define SD_QUANTILE_MEDIAN 5    /* np.nanmedian: the middle sample, or (v[n/2 - 1] + v[n/2]) / 2; q and Q are not read, Q counts as 1 */

/* sd_spells: the comparison of a sample x with its threshold t (one IEEE comparison of doubles) */
#define SD_SPELL_GT 0  /* x > t */
#define SD_SPELL_GE 1  /* x >= t */
#define SD_SPELL_LT 2  /* x < t */
#define SD_SPELL_LE 3  /* x <= t */
/* sd_spells: statistics of a bin, from its state (valid, hits, run, longest, days, spells) */
#define SD_SPELL_VALID 0          /* steps where neither the sample nor the threshold is NaN */
#define SD_SPELL_COUNT 1          /* hits */
#define SD_SPELL_FRACTION 2       /* (double)hits / (double)valid; NaN for a bin without a valid step */
#define SD_SPELL_LONGEST_SPELL 3  /* the longest run of consecutive hits */
#define SD_SPELL_SPELL_DAYS 4     /* steps inside runs of at least min_length hits */
#define SD_SPELL_SPELL_COUNT 5    /* runs of at least min_length hits */
/* sd_skill: statistics of a bin of two fields a and b, from the sums over its valid pairs */
#define SD_SKILL_COUNT 0      /* n: the valid pairs */
#define SD_SKILL_BIAS 1       /* sd / n */
#define SD_SKILL_RATIO 2      /* sa / sb */
#define SD_SKILL_MAE 3        /* sabs / n */
#define SD_SKILL_RMSE 4       /* sqrt(sq / n) */
#define SD_SKILL_CORR 5       /* qab / (sqrt(qaa) * sqrt(qbb)), clamped to [-1, 1] */
#define SD_SKILL_STD_RATIO 6  /* sqrt(qaa / qbb) */
/* sd_twosample: statistics of a bin of two fields a and b, from each field's own sorted non-NaN samples */
#define SD_TWOSAMPLE_KS 0       /* the two-sample Kolmogorov-Smirnov distance */
#define SD_TWOSAMPLE_PERKINS 1  /* the Perkins skill score: the overlap of the two histograms */
#define SD_TWOSAMPLE_NA 2       /* na: the non-NaN samples of a */
#define SD_TWOSAMPLE_NB 3       /* nb: the non-NaN samples of b */

#define SD_SYNTH_GAUSS 0
#define SD_SYNTH_PRECIP 1

typedef struct sd_ctx sd_ctx;
typedef struct sd_bcsd_state sd_bcsd_state;
typedef struct sd_analog_state sd_analog_state;
typedef struct sd_qm_state sd_qm_state;
typedef struct sd_linreg_state sd_linreg_state;
typedef struct sd_zscore_state sd_zscore_state;
typedef struct sd_grouped_state sd_grouped_state;
typedef struct sd_arrm_state sd_arrm_state;
typedef struct sd_regrid sd_regrid;
typedef struct sd_remap sd_remap;
typedef struct sd_comm sd_comm;
#define SD_COMM_ID_BYTES 128 /* RCCL's ncclUniqueId */

/* ---- library / context ---------------------------------------------------------------------- */
int sd_version(void);
const char* sd_last_error(void);
int sd_device_count(int* count);
int sd_ctx_create(int device, sd_ctx** out);
int sd_ctx_destroy(sd_ctx* ctx);
int sd_ctx_synchronize(sd_ctx* ctx);
/* States and per-call scratch recycle device blocks through a per-context cache (at most 1/2 of the HBM, given back when an allocation fails);
 * this returns the cached blocks and the rank workspace to the driver. */
int sd_ctx_release_cached(sd_ctx* ctx);
int sd_ctx_device_info(sd_ctx* ctx, char* name, size_t name_len, int* compute_units, int64_t* hbm_bytes);

/* ---- device memory (so a non-torch host can keep fields resident in HBM) --------------------- */
int sd_dev_alloc(sd_ctx* ctx, size_t bytes, void** dptr);
int sd_dev_free(sd_ctx* ctx, void* dptr);
int sd_memcpy_h2d(sd_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int sd_memcpy_d2h(sd_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* float32 transport: a float32 grid crosses PCIe as float32 and is widened / narrowed on the device (exact
 * widening, round-to-nearest narrowing: what the reference's NumPy promotion / result cast do on the host, core.py:119).
 * n elements; src and dst device pointers, queued on the context's stream. */
int sd_convert_f32_to_f64_dev(sd_ctx* ctx, const float* src_dev, int64_t n, double* dst_dev);
int sd_convert_f64_to_f32_dev(sd_ctx* ctx, const double* src_dev, int64_t n, float* dst_dev);
int sd_memcpy_d2d(sd_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);

/* ---- timing: HIP events on the context's stream ---------------------------------------------- */
int sd_timer_start(sd_ctx* ctx);
int sd_timer_stop(sd_ctx* ctx, float* elapsed_ms); /* synchronises the stream */
/* per-kernel profile: when enabled every launch is bracketed by events (serialising). */
int sd_prof_enable(sd_ctx* ctx, int on);
int sd_prof_reset(sd_ctx* ctx);
int sd_prof_query(sd_ctx* ctx, const char* kernel_name, double* total_ms, int64_t* launches);
int sd_prof_names(sd_ctx* ctx, char* buf, size_t buf_len); /* ';'-separated kernel names */

/* ---- deterministic synthetic fields generated in HBM (mirror: skdownscale_amd/synth.py) ------- */
int sd_synth_fill(sd_ctx* ctx, double* out_dev, int64_t T, int64_t C, int64_t ld, int64_t c_offset, int64_t c_full,
                  int kind, uint64_t seed, uint32_t stream, const double* base_host /* [T] or NULL */, double amp,
                  double cell_scale, double p_dry, int32_t stream2 /* <0: none */, double amp2);

/* ---- BCSD quantile mapping --------------------------------------------------------------------
 * X: [T,C] model-historical field (TAS: used for x_climo; PR: only validated, may be NULL ->
 * mask/validation then use y).  y: [T,C] observations.  group_id: host int32[T].
 * The `return_anoms` argument of the fit entry points and of sd_bcsd_state_import / sd_bcsd_state_info is a bit set:
 * SD_BCSD_RETURN_ANOMS (bcsd.py:27,266-267 / 170-185) | SD_BCSD_QM_DETREND (qm_kwargs={'detrend': True}: quantile.py:95-98,
 * 128-145 -- every group's series loses its least-squares line over the sample index, trend.py:51-83, before the CDFs are
 * built; the predict line is added back re-based on the fitted intercept).  Plain 0 / 1 keep their old meaning.  Detrended
 * mapping serves group segments of up to 19 456 samples (SD_ERR_UNSUPPORTED beyond). */
#define SD_BCSD_RETURN_ANOMS 1
#define SD_BCSD_QM_DETREND 2
int sd_bcsd_fit(sd_ctx* ctx, int kind, const double* X, const double* y, const int32_t* group_id, int G, int64_t T,
                int64_t C, int return_anoms, sd_bcsd_state** out);
int sd_bcsd_fit_dev(sd_ctx* ctx, int kind, const double* X_dev, const double* y_dev, int64_t ld,
                    const int32_t* group_id, int G, int64_t T, int64_t C, int return_anoms, sd_bcsd_state** out);
/* out: [Tp,C]; cell_status: host int32[C] (may be NULL).  Cells whose fit status != OK get NaN. */
int sd_bcsd_predict(sd_ctx* ctx, const sd_bcsd_state* st, const double* Xp, const int32_t* group_id_p, int64_t Tp,
                    double* out, int32_t* cell_status);
int sd_bcsd_predict_dev(sd_ctx* ctx, const sd_bcsd_state* st, const double* Xp_dev, int64_t ld,
                        const int32_t* group_id_p, int64_t Tp, double* out_dev, int64_t ld_out, int32_t* cell_status);
/* fused fit+predict for resident fields: one pass, no persisted state. */
/* Fit on explicitly listed groups: group_order[group_offsets[G]] = time indices group by group (a time step may belong
 * to several groups, or to none: the +-15-day day-of-year windows of time_grouper='daily_nasa-nex', groupers.py:19-89,
 * bcsd.py:36-38,50-55), group_offsets[G+1].  The state's series length (sd_bcsd_state_info T, y_sorted of the export)
 * is the number of listed entries. */
int sd_bcsd_fit_groups(sd_ctx* ctx, int kind, const double* X, const double* y, const int32_t* group_order,
                       const int64_t* group_offsets, int G, int64_t T, int64_t C, int return_anoms, sd_bcsd_state** out);
int sd_bcsd_fit_groups_dev(sd_ctx* ctx, int kind, const double* X_dev, const double* y_dev, int64_t ld, const int32_t* group_order,
                           const int64_t* group_offsets, int G, int64_t T, int64_t C, int return_anoms, sd_bcsd_state** out);
/* Predict with a climate-trend grouper of its own (bcsd.py:247-267): the 9-sample rolling mean runs over the groups of
 * trend_group_id (climate_trend, G_trend groups), the climatologies and the quantile mapping use group_id_p (groups of
 * the fitted state).  BcsdPrecipitation has no trend: same as sd_bcsd_predict. */
int sd_bcsd_predict_trend(sd_ctx* ctx, const sd_bcsd_state* st, const double* Xp, const int32_t* group_id_p,
                          const int32_t* trend_group_id, int G_trend, int64_t Tp, double* out, int32_t* cell_status);
int sd_bcsd_predict_trend_dev(sd_ctx* ctx, const sd_bcsd_state* st, const double* Xp_dev, int64_t ld, const int32_t* group_id_p,
                              const int32_t* trend_group_id, int G_trend, int64_t Tp, double* out_dev, int64_t ld_out,
                              int32_t* cell_status);
int sd_bcsd_fit_predict_dev(sd_ctx* ctx, int kind, const double* X_dev, const double* y_dev, int64_t ld,
                            const int32_t* group_id, int G, int64_t T, int64_t C, int return_anoms,
                            const double* Xp_dev, int64_t ld_p, const int32_t* group_id_p, int64_t Tp,
                            double* out_dev, int64_t ld_out, int32_t* cell_status);
int sd_bcsd_state_info(const sd_bcsd_state* st, int* kind, int* G, int64_t* T, int64_t* C, int* return_anoms);
int sd_bcsd_state_status(const sd_bcsd_state* st, int32_t* cell_status /* host [C] */);
/* Plain-array view of the fitted state (pickling / get_attr): y_sorted is CELL-major [C][T] with the
 * G group segments of a cell stored back to back at group_offsets[g]; climatologies are [C][G]. */
int sd_bcsd_state_export(const sd_bcsd_state* st, double* y_sorted, double* x_climo, double* y_climo,
                         int32_t* cell_status, int64_t* group_offsets /* [G+1] */);
int sd_bcsd_state_import(sd_ctx* ctx, int kind, int G, int64_t T, int64_t C, int return_anoms, const double* y_sorted,
                         const double* x_climo, const double* y_climo, const int32_t* cell_status,
                         const int64_t* group_offsets, sd_bcsd_state** out);
/* SD_BCSD_QM_DETREND states: slope and intercept of the fitted segments' lines, [C][G][2] (x_trend_fit_.lr_model_.coef_ /
 * .intercept_ of every group's QuantileMapper, quantile.py:97,145).  set_trend completes a state made by
 * sd_bcsd_state_import (only the intercepts enter predictions). */
/* Tail handling of the fitted inverse CDF (qm_kwargs={'qt_kwargs': {'extrapolate': ..., 'n_endpoints': ...}}: bcsd.py:59-67 ->
 * quantile.py:418-431, 523-545): which side continues along the least-squares line through the first / last n_endpoints
 * points of the fitted CDF (SD_QT_TAIL_LOWER | SD_QT_TAIL_UPPER = 'both', the default; 'min' = lower only, 'max' = upper only,
 * None / '1to1' = neither: np.interp then holds the end value), and n_endpoints >= 1 (default 10).  Reaches predictions only when
 * a predict group is longer than its fit group.  Applies to later sd_bcsd_predict* calls on the state; group segments of up to
 * 2 112 samples (SD_ERR_UNSUPPORTED beyond for non-default settings).  (`alpha` / `beta` of the CunnaneTransformer never reach
 * the result in the reference -- quantile.py:462 calls plotting_positions(n) with its defaults -- and have no entry here.) */
#define SD_QT_TAIL_LOWER 1
#define SD_QT_TAIL_UPPER 2
int sd_bcsd_state_set_tails(sd_bcsd_state* st, int extrapolate, int n_endpoints);
int sd_bcsd_state_get_trend(const sd_bcsd_state* st, double* y_trend);
int sd_bcsd_state_set_trend(sd_bcsd_state* st, const double* y_trend);
int sd_bcsd_state_destroy(sd_bcsd_state* st);

/* ---- GARD analogs ----------------------------------------------------------------------------
 * X: [T,F,C], y: [T,C], Xq: [Tq,F,C]; out: [Tq,3,C] columns pred / exceedance_prob /
 * prediction_error (gard.py:254-255).  inds: int64 [Tq,k,C] training indices, ascending distance
 * (may be NULL); dist: float64 [Tq,k,C] (may be NULL).  sample_inds: int32 [Tq,C], required for
 * SD_ANALOG_SAMPLE (the host draws them with np.random.randint like gard.py:315).  k == 1 is 'best_analog' whatever
 * `kind` says (gard.py:291-296). */
int sd_analog_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, sd_analog_state** out);
int sd_analog_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                      sd_analog_state** out);
int sd_analog_predict(sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t Tq, int k, int kind,
                      int has_thresh, double thresh, const int32_t* sample_inds, double* out, int64_t* inds,
                      double* dist, int32_t* cell_status);
int sd_analog_predict_dev(sd_ctx* ctx, const sd_analog_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, int k,
                          int kind, int has_thresh, double thresh, const int32_t* sample_inds_dev, double* out_dev,
                          int64_t ld_out, int64_t* inds_dev, double* dist_dev, int32_t* cell_status);
/* fit + predict in one call, no fitted state left behind (AnalogBase.fit, gard.py:58-87, followed by PureAnalog.predict,
 * gard.py:273-364, on the same object): for callers that drop the estimator after predicting.  Results are bit-identical to
 * sd_analog_fit* -> sd_analog_predict*; F == 1, `SD_ANALOG_MEAN` without a threshold (or k == 1) on series the tile-shaped fit
 * serves run as one fused per-cell kernel, everything else takes the two calls internally.  SD_ANALOG_SAMPLE is not served
 * (it needs sample_inds: use the split calls). */
int sd_analog_fit_predict(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, const double* Xq, int64_t Tq,
                          int k, int kind, int has_thresh, double thresh, double* out, int32_t* cell_status);
int sd_analog_fit_predict_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                              const double* Xq_dev, int64_t ld_q, int64_t Tq, int k, int kind, int has_thresh, double thresh,
                              double* out_dev, int64_t ld_out, int32_t* cell_status);
/* AnalogRegression.predict (gard.py:152-224).  has_thresh: exceedance_prob from a logistic regression of (analog value >
 * thresh) on the analogs' features (the reference reports predict_proba(x)[0, 0], the probability of NOT exceeding;
 * 1.0 when every analog exceeds), linear model and RMSE on the exceeding analogs; a query without any exceeding analog
 * sets SD_CELL_ONE_CLASS for its cell (the reference raises there). */
int sd_analogreg_predict(sd_ctx* ctx, const sd_analog_state* st, const double* Xq, int64_t Tq, int k, int has_thresh, double thresh,
                         double* out, int32_t* cell_status);
int sd_analogreg_predict_dev(sd_ctx* ctx, const sd_analog_state* st, const double* Xq_dev, int64_t ld, int64_t Tq,
                             int k, int has_thresh, double thresh, double* out_dev, int64_t ld_out, int32_t* cell_status);
int sd_analog_state_info(const sd_analog_state* st, int64_t* T, int* F, int64_t* C);
int sd_analog_state_destroy(sd_analog_state* st);

/* ---- quantile-mapping regressors ----------------------------------------------------------------
 * Replace core.py:86-96 / 137-141 looping QuantileMappingReressor (quantile.py:160-395) or
 * EquidistantCdfMatcher (quantile.py:556-636) per cell.  X, y: [T, C] float64, cells contiguous; the whole series is one
 * segment.  model: SD_QM_REGRESSOR / SD_QM_EDCDF_DIFFERENCE / SD_QM_EDCDF_RATIO.  extrapolate: SD_EXTRAP_NONE (None),
 * SD_EXTRAP_MIN / MAX / BOTH (synthetic end points at -+1e20 from a least-squares line through the n_endpoints outermost
 * points, quantile.py:312-387) or SD_EXTRAP_1TO1.  Series up to 19 456 samples. */
int sd_qm_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int64_t C, sd_qm_state** out);
int sd_qm_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int64_t C,
                  sd_qm_state** out);
int sd_qm_predict(sd_ctx* ctx, const sd_qm_state* st, int model, int extrapolate, int n_endpoints, const double* Xp, int64_t Tp,
                  double* out, int32_t* cell_status);
int sd_qm_predict_dev(sd_ctx* ctx, const sd_qm_state* st, int model, int extrapolate, int n_endpoints, const double* Xp_dev,
                      int64_t ld, int64_t Tp, double* out_dev, int64_t ld_out, int32_t* cell_status);
/* CunnaneTransformer.transform / inverse_transform (quantile.py:465-545) on the sorted X of a fitted state
 * (sd_qm_fit accepts y = NULL for this use).  X: [Tp, C]; out: [Tp, C].
 * FORWARD: np.interp(x, sorted X, Cunnane positions); a value beyond an extended tail yields -inf / +inf (the
 * reference's own tail code for this direction, quantile.py:497/501, cannot run: it calls .values on an ndarray).
 * INVERSE: np.interp(p, positions, sorted X); beyond an extended tail the centred least-squares line through the
 * n_endpoints first / last (position, value) pairs (quantile.py:532-543). */
int sd_qm_cunnane(sd_ctx* ctx, const sd_qm_state* st, int direction, int extrapolate, int n_endpoints, const double* X,
                  int64_t Tp, double* out, int32_t* cell_status);
int sd_qm_cunnane_dev(sd_ctx* ctx, const sd_qm_state* st, int direction, int extrapolate, int n_endpoints,
                      const double* X_dev, int64_t ld, int64_t Tp, double* out_dev, int64_t ld_out,
                      int32_t* cell_status);
int sd_qm_state_info(const sd_qm_state* st, int64_t* T, int64_t* C);
/* sorted fit series [C][T] (cell-major) and per-cell status; any pointer may be NULL */
int sd_qm_state_export(const sd_qm_state* st, double* x_sorted, double* y_sorted, int32_t* cell_status);
int sd_qm_state_destroy(sd_qm_state* st);

/* ---- PureRegression ----------------------------------------------------------------------------------
 * Replaces core.py:86-96 / 137-141 looping gard.py:410-470: per cell an ordinary least-squares fit of y [T, C] on
 * X [T, F, C] (centred lstsq like sklearn's LinearRegression, minimum-norm for collinear features) and its RMSE
 * (fit_error_); predict writes out [Tq, 3, C] = pred / exceedance_prob / fit_error_ (gard.py:254-255 column order).
 * has_thresh (gard.py:416-437): the linear model uses the samples with y > thresh, exceedance_prob =
 * predict_proba(X)[:, 1] of a logistic regression of (y > thresh) on the features (L2, C = 1: sklearn's defaults); a cell
 * whose samples all exceed drops its threshold (probability 1), one without any exceeding sample gets SD_CELL_ONE_CLASS. */
int sd_linreg_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, int has_thresh, double thresh,
                  sd_linreg_state** out);
int sd_linreg_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                      int has_thresh, double thresh, sd_linreg_state** out);
int sd_linreg_predict(sd_ctx* ctx, const sd_linreg_state* st, const double* Xq, int64_t Tq, double* out,
                      int32_t* cell_status);
int sd_linreg_predict_dev(sd_ctx* ctx, const sd_linreg_state* st, const double* Xq_dev, int64_t ld, int64_t Tq,
                          double* out_dev, int64_t ld_out, int32_t* cell_status);
int sd_linreg_state_info(const sd_linreg_state* st, int64_t* T, int* F, int64_t* C);
/* coef [F][C], intercept [C], fit_error [C], logistic [F+1][C] (coefficients, then the intercept; models with a threshold),
 * thresh_dropped [C], status [C]; any pointer may be NULL */
int sd_linreg_state_export(const sd_linreg_state* st, double* coef, double* intercept, double* fit_error, double* logistic,
                           int32_t* thresh_dropped, int32_t* cell_status);
/* device state from exported numbers (pickling, checkpoint / resume); logistic = thresh_dropped = NULL without a threshold */
int sd_linreg_state_import(sd_ctx* ctx, int64_t T, int F, int64_t C, const double* coef, const double* intercept, const double* fit_error,
                           const double* logistic, const int32_t* thresh_dropped, const int32_t* cell_status, sd_linreg_state** out);
int sd_linreg_state_destroy(sd_linreg_state* st);

/* ---- ZScoreRegressor -----------------------------------------------------------------------------------
 * fit: X, y [T, C].  day_idx: host int32[T], the position of each sample's day of year in the sorted union of the days that
 * occur (D of them, each with a sample); year: host int32[T], the sample's calendar year (two samples on one (year, day) are
 * refused like the reference's alignment does).  Per cell the mean and population std of X and of y over the kept day windows
 * of width window_width (K of them: sd_zscore_plan.h), shift = y_mean - X_mean, scale = y_std / X_std.
 * predict: out [Tp, C] = z * (std * scale) + (mean + shift) with pandas' centred rolling mean / std (ddof = 1) of Xp and the
 * parameters expanded by position (entry t % min(Tp, 364); SD_ERR_INVALID past K).  meani / stdi / meanf / stdf [Tp, C]
 * (predict_stats_dict_) are written when not NULL, with the pitch ld_out in the _dev variant. */
int sd_zscore_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int64_t C, int window_width, const int32_t* day_idx,
                  const int32_t* year, int D, sd_zscore_state** out);
int sd_zscore_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int64_t C, int window_width,
                      const int32_t* day_idx, const int32_t* year, int D, sd_zscore_state** out);
int sd_zscore_predict(sd_ctx* ctx, const sd_zscore_state* st, const double* Xp, int64_t Tp, double* out, double* meani, double* stdi,
                      double* meanf, double* stdf, int32_t* cell_status);
int sd_zscore_predict_dev(sd_ctx* ctx, const sd_zscore_state* st, const double* Xp_dev, int64_t ld, int64_t Tp, double* out_dev,
                          int64_t ld_out, double* meani_dev, double* stdi_dev, double* meanf_dev, double* stdf_dev, int32_t* cell_status);
int sd_zscore_state_info(const sd_zscore_state* st, int64_t* K, int64_t* C, int* window_width);
/* [K][C] planes (any pointer may be NULL) and the per-cell status: pickling and get_attr */
int sd_zscore_state_export(const sd_zscore_state* st, double* x_mean, double* x_std, double* y_mean, double* y_std, double* shift,
                           double* scale, int32_t* cell_status);
int sd_zscore_state_import(sd_ctx* ctx, int64_t K, int64_t C, int window_width, const double* x_mean, const double* x_std,
                           const double* y_mean, const double* y_std, const double* shift, const double* scale,
                           const int32_t* cell_status, sd_zscore_state** out);
int sd_zscore_state_destroy(sd_zscore_state* st);

/* ---- GroupedRegressor (one LinearRegression per group) -------------------------------------------------
 * fit: X [T, F, C], y [T, C], F in [1, 8].  key: host int32[T], the key of every time step in [0, n), shared by all cells
 * (day of year - 1 for grouping.PaddedDOYGrouper, n = the largest day of year).  Group g of [0, n) is fitted per cell by
 * ordinary least squares (sklearn LinearRegression: centred, minimum norm when rank deficient) on the samples whose key
 * lies in {g - window .. g + window} modulo n, every key once; 0 <= window < n, window = 0 gives disjoint groups.  A group
 * whose window holds no sample is not fitted.
 * predict: out [Tq, C], out[t, c] = intercept[key[t], c] + sum_f coef[key[t], f, c] * Xq[t, f, c].  A key outside [0, n) or
 * without a fitted model is SD_ERR_INVALID; sd_last_error names the smallest such key ("no fitted model for key K").
 * Cell status as for sd_linreg_*. */
int sd_grouped_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int F, int64_t C, const int32_t* key, int n, int window,
                   sd_grouped_state** out);
int sd_grouped_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int F, int64_t C,
                       const int32_t* key, int n, int window, sd_grouped_state** out);
int sd_grouped_predict(sd_ctx* ctx, const sd_grouped_state* st, const double* Xq, int64_t Tq, const int32_t* key, double* out,
                       int32_t* cell_status);
int sd_grouped_predict_dev(sd_ctx* ctx, const sd_grouped_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, const int32_t* key,
                           double* out_dev, int64_t ld_out, int32_t* cell_status);
int sd_grouped_state_info(const sd_grouped_state* st, int* n, int* F, int64_t* C, int* window);
/* coef [n, F, C], intercept [n, C] (NaN for groups that are not fitted and for cells with a status), fitted int32[n],
 * cell_status int32[C]; any pointer may be NULL */
int sd_grouped_state_export(const sd_grouped_state* st, double* coef, double* intercept, int32_t* fitted, int32_t* cell_status);
int sd_grouped_state_import(sd_ctx* ctx, int n, int F, int64_t C, int window, const double* coef, const double* intercept,
                            const int32_t* fitted, const int32_t* cell_status, sd_grouped_state** out);
int sd_grouped_state_destroy(sd_grouped_state* st);

/* ---- PiecewiseLinearRegression(fit_option='arrm') ------------------------------------------------------
 * fit: X [T, C], y [T, C] (one feature).  Per cell arrm_breakpoints(X, y, 0.05, max_breakpoints) of the reference: B =
 * 2 * (max_breakpoints / 2) breaks, taken where the correlation of the two independently sorted series over a sliding window is
 * lowest; then the continuous piecewise-linear least-squares fit on those breaks (pwlf fit_with_breaks, degree 1), minimum norm
 * where breaks repeat.  Supported: T >= 50 and 2 <= B <= 16, anything else is SD_ERR_INVALID; series beyond the workgroup sort
 * are SD_ERR_UNSUPPORTED.  r2 (may be NULL): [T, C] diagnostic with rows of C entries (r2_dev too, whatever ld is), r2[t, c] is the squared correlation of the window that the
 * reference writes last to slot t (both loops, without the masks), NaN for a window of equal values, 2 for a slot no window
 * writes.
 * predict: out [Tq, C], out = beta[0] + beta[1] (x - b[0]) + sum_{j=1}^{B-2} beta[j+1] max(x - b[j], 0); the line extends beyond
 * both ends.  Cell status as for sd_linreg_*. */
int sd_arrm_fit(sd_ctx* ctx, const double* X, const double* y, int64_t T, int64_t C, int max_breakpoints, double* r2, sd_arrm_state** out);
int sd_arrm_fit_dev(sd_ctx* ctx, const double* X_dev, const double* y_dev, int64_t ld, int64_t T, int64_t C, int max_breakpoints,
                    double* r2_dev, sd_arrm_state** out);
int sd_arrm_predict(sd_ctx* ctx, const sd_arrm_state* st, const double* Xq, int64_t Tq, double* out, int32_t* cell_status);
int sd_arrm_predict_dev(sd_ctx* ctx, const sd_arrm_state* st, const double* Xq_dev, int64_t ld, int64_t Tq, double* out_dev, int64_t ld_out,
                        int32_t* cell_status);
int sd_arrm_state_info(const sd_arrm_state* st, int* B, int64_t* C, int64_t* T);
/* breaks [B, C] ascending, break_index int32 [B, C] (positions in the sorted X; -1 for cells with a status), beta [B, C],
 * ssr [C] (sum of squared residuals), cell_status int32 [C]; any pointer may be NULL */
int sd_arrm_state_export(const sd_arrm_state* st, double* breaks, int32_t* break_index, double* beta, double* ssr, int32_t* cell_status);
int sd_arrm_state_import(sd_ctx* ctx, int B, int64_t C, int64_t T, const double* breaks, const int32_t* break_index, const double* beta,
                         const double* ssr, const int32_t* cell_status, sd_arrm_state** out);
int sd_arrm_state_destroy(sd_arrm_state* st);

/* ---- regridding: GridArray.interp_like (xarray's interp_like with 1-D coordinates) -------------------------
 * A [T, ny, nx] field on the rectilinear grid (src_y [ny], src_x [nx]) is interpolated onto the grid (dst_y [Ny], dst_x [Nx]); the
 * result is a [T, C] field, C = Ny * Nx, cells fastest, rows ld_out >= C elements apart: what the fit / predict entry points take.
 * Per dimension the rule of scipy.interpolate.interp1d(bounds_error=False, fill_value=nan, assume_sorted=False), the first spatial
 * dimension (y) before the second: bracket hi = clip(searchsorted(x ascending, xn, 'left'), 1, n - 1), lo = hi - 1, value
 * (v[hi] - v[lo]) / (x[hi] - x[lo]) * (xn - x[lo]) + v[lo]; a target on node k >= 1 uses the interval below it; NaN outside the
 * source range; a NaN node of the bracket gives NaN also at weight 0.  SD_REGRID_NEAREST: the nearest node, a midpoint to the lower
 * one, NaN outside the range.  Source coordinates ascend or descend strictly, target coordinates come in any order; a coordinate
 * that is NaN, a source coordinate that is not strictly monotonic and a source dimension of length 1 are SD_ERR_INVALID.
 * sd_regrid_create builds the two separable tables (Ny + Nx entries) and uploads them; a sd_regrid serves any number of calls.
 * src: float64, or float32 with src_is_f32 != 0 (widened in the kernel: the values are those of the widened source). */
int sd_regrid_create(sd_ctx* ctx, int method, int64_t ny, int64_t nx, const double* src_y, const double* src_x, int64_t Ny, int64_t Nx,
                     const double* dst_y, const double* dst_x, sd_regrid** out);
int sd_regrid_destroy(sd_regrid* rg);
int sd_regrid_info(const sd_regrid* rg, int* method, int64_t* ny, int64_t* nx, int64_t* Ny, int64_t* Nx);
int sd_regrid_apply_dev(sd_ctx* ctx, const sd_regrid* rg, const void* src_dev, int src_is_f32, int64_t T, double* out_dev,
                        int64_t ld_out);
/* host buffers: src [T, ny, nx], out [T, Ny * Nx] */
int sd_regrid_apply(sd_ctx* ctx, const sd_regrid* rg, const void* src_host, int src_is_f32, int64_t T, double* out_host);

/* ---- conservative remapping: GridArray.remap_like (fine to coarse, first order, area overlap) -----------------
 * A [T, ny, nx] field (rows of a step contiguous, steps ld >= ny * nx elements apart) on a rectilinear grid is averaged onto the
 * cells of an [Ny, Nx] rectilinear grid; the result is a [T, C] float64 field, C = Ny * Nx, cells fastest, rows ld_out >= C apart.
 * Each dimension is given by its cell bounds (src_yb [ny + 1], src_xb [nx + 1], dst_yb [Ny + 1], dst_xb [Nx + 1]), strictly
 * ascending or descending as stored, in the units whose differences are the weights (the caller transforms latitudes: no sin here).
 * Per dimension the overlap of source cell k with target cell j is w = min(sb_hi, db_hi) - max(sb_lo, db_lo) on the ascending-ordered
 * bounds; only overlaps > 0 count, they form one contiguous run of source cells per target cell, and full[j] is their running sum
 * from +0.0 in stored order (at most n_src + n_dst - 1 entries per dimension; never a per-cell table).  Per step and target (j, i),
 * every product rounded on its own and every sum a running sum from +0.0 in stored order:
 *   cn[x] = sum over the rows y of run j of wy[y] * (v[t, y, x] is NaN ? 0 : v),  cd[x] = sum of wy[y] * (v is NaN ? 0 : 1)
 *   num = sum over the columns x of run i of wx[x] * cn[x],                        den = sum of wx[x] * cd[x]
 *   out = num / den  if den > 0 and den >= min_valid * (full_y[j] * full_x[i]) * (1 - 2^-30),  else NaN
 * min_valid in [0, 1] is the valid share of the covered area a target cell needs (0: any valid sample; the 2^-30 slack lets a fully
 * covered, fully valid cell pass at 1).  A target cell outside the source hull is NaN; a partly covered one is the mean over its
 * covered part.  inf follows IEEE arithmetic.  Longitudes do not wrap.  The result does not depend on the launch geometry or on how
 * the time axis is cut.  src: float64, or float32 with src_is_f32 != 0 (widened in the kernel: the values are those of the widened
 * source).  NaN in the bounds, bounds that are not strictly monotonic, a dimension without a cell, ld < ny * nx, ld_out < C,
 * min_valid outside [0, 1] and a grid too large for 32-bit row, column and table indices are SD_ERR_INVALID.
 * sd_remap_create builds and uploads the two tables; a sd_remap serves any number of calls. */
int sd_remap_create(sd_ctx* ctx, int64_t ny, int64_t nx, const double* src_yb, const double* src_xb, int64_t Ny, int64_t Nx,
                    const double* dst_yb, const double* dst_xb, sd_remap** out);
int sd_remap_destroy(sd_remap* rm);
int sd_remap_info(const sd_remap* rm, int64_t* ny, int64_t* nx, int64_t* Ny, int64_t* Nx, int64_t* y_entries, int64_t* x_entries);
int sd_remap_apply_dev(sd_ctx* ctx, const sd_remap* rm, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, double min_valid,
                       double* out_dev, int64_t ld_out);
/* host buffers: src [T, ny, nx], out [T, Ny * Nx]; upload, run, download */
int sd_remap_apply(sd_ctx* ctx, const sd_remap* rm, const void* src_host, int src_is_f32, int64_t T, double min_valid, double* out_host);

/* ---- resampling of the time axis: GridArray.resample(time=rule).mean() / .sum() -----------------------------
 * A [T, C] field (cells fastest, rows ld >= C elements apart) is reduced over runs of consecutive rows into an [M, C] float64 field
 * (rows ld_out >= C apart): bin m is the rows offsets[m] .. offsets[m + 1] - 1.  The table is a host array of M + 1 entries that
 * starts at 0, never decreases and ends at T (pandas' resampler makes it: counts = series.resample(rule).size(), offsets = [0,
 * cumsum(counts)]); an empty bin has two equal entries.  Both reductions skip NaN samples; a bin without a non-NaN sample -- empty or
 * all NaN -- gives NaN for SD_RESAMPLE_MEAN and 0 for SD_RESAMPLE_SUM, as pandas' DataFrame.resample(rule).mean() / .sum() do.  The
 * samples of a bin are added in time order, so the result of a bin does not depend on what else the call holds.  inf follows IEEE
 * arithmetic.  src: float64, or float32 with src_is_f32 != 0 (widened per sample in the kernel).  An unknown op, sizes <= 0, ld < C,
 * ld_out < C and a table that breaks the rules above are SD_ERR_INVALID. */
int sd_resample_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int64_t* offsets,
                    int64_t M, double* out_dev, int64_t ld_out);
/* host buffers: src [T, C], out [M, C]; upload, run, download */
int sd_resample(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int64_t* offsets, int64_t M,
                double* out_host);

/* ---- temporal disaggregation: GridArray.disaggregate (the last step of BCSD, Wood et al. 2004) ---------------------
 * A monthly target [M, C] float64 (rows ld_t >= C apart) becomes a daily field out [Tout, C] float64 (rows ld_out >= C apart): output
 * row t borrows row src_row[t] of the daily observations obs [To, C] (float64, or float32 with obs_is_f32 != 0, widened per sample;
 * rows ld_obs >= C apart), and bin m is the output rows offsets[m] .. offsets[m + 1] - 1.  Both tables are host arrays: src_row of
 * Tout entries in [0, To), offsets of M + 1 entries that starts at 0, never decreases and ends at Tout.  Per bin and cell, with x_t the
 * borrowed samples in time order, acc their plain running sum without the NaN ones and cnt the number of those (the statistic of
 * sd_resample): SD_DISAGG_SHIFT out_t = x_t + (tgt - acc / cnt); SD_DISAGG_SCALE_MEAN out_t = x_t * (tgt / (acc / cnt)), and tgt on
 * every non-NaN day where acc / cnt == 0; SD_DISAGG_SCALE_SUM out_t = x_t * (tgt / acc), and tgt / cnt on every non-NaN day where
 * acc == 0.  tgt is target[m], or with a climatology climo [G, C] float64 (rows ld_c >= C apart) and group [M] (host, in [0, G)):
 * climo[group[m]] + target[m] for the shift and climo[group[m]] * target[m] for the scale ops; climo and group are both given or both
 * NULL.  A NaN sample stays NaN, a bin without a sample and a bin with a NaN target are NaN, inf follows IEEE arithmetic.  Every
 * operation is a single add, subtract, multiply or divide.  An unknown op, sizes <= 0, a leading dimension below C, climo without
 * group or the reverse, a table that breaks the rules above and a call too large for the grid are SD_ERR_INVALID. */
int sd_disagg_dev(sd_ctx* ctx, int op, const double* target_dev, int64_t ld_t, const void* obs_dev, int obs_is_f32, int64_t ld_obs, int64_t To,
                  int64_t C, const int64_t* src_row, int64_t Tout, const int64_t* offsets, int64_t M, const double* climo_dev_or_null,
                  int64_t ld_c, int64_t G, const int32_t* group_or_null, double* out_dev, int64_t ld_out);
/* host buffers: target [M, C], obs [To, C], climo [G, C] or NULL, out [Tout, C]; upload, run, download */
int sd_disagg(sd_ctx* ctx, int op, const double* target_host, const void* obs_host, int obs_is_f32, int64_t To, int64_t C,
              const int64_t* src_row, int64_t Tout, const int64_t* offsets, int64_t M, const double* climo_host_or_null, int64_t G,
              const int32_t* group_or_null, double* out_host);

/* ---- grouping of the time axis: GridArray.groupby(...).mean() / .sum() and gb - clim, gb + clim, gb * clim, gb / clim ----------
 * Every row t of a [T, C] field (cells fastest, rows ld >= C elements apart; float64, or float32 with src_is_f32 != 0, widened per
 * sample in the kernel) carries a group id group[t] in [0, G); group is a host array of T entries.  Unlike the bins of sd_resample the
 * rows of a group need not be consecutive, and a group may recur in a later call.
 *
 * reduce: the rows of the call are added, in row order, onto row group[t] of the accumulators sum [G, C] float64 and count [G, C]
 * int32 (rows ld_acc >= C apart).  Per (group, cell) the non-NaN samples are added by a plain running sum that starts at the carried
 * value; NaN samples are skipped by a select; count is the number of samples added.  carry == 0: the accumulators start from zero
 * (they need not be initialised); carry != 0: they continue from what an earlier call left.  So cutting [0, T) into any sequence of
 * calls with carry gives the same bits as one call, and the result depends neither on the launch geometry, nor on the layout, nor on
 * the number of cells per lane.  out_dev_or_null != NULL: the result [G, C] float64 (rows ld_out >= C apart) is written from the
 * accumulators after this call's rows: SD_GROUPBY_MEAN sum / count, NaN where count == 0 (a group id that never occurs and an
 * all-NaN group alike); SD_GROUPBY_SUM sum, 0.0 where count == 0 (pandas' min_count=0).  inf follows IEEE arithmetic.  Where the
 * groups are runs of consecutive rows the result is that of sd_resample bit for bit.
 *
 * apply: out[t, c] = src[t, c] (op) table[group[t], c] with table [G, C] float64 (rows ld_t >= C apart) and out [T, C] float64 (rows
 * ld_out >= C apart): one IEEE subtract, add, multiply or divide per element (a zero in the table under SD_GROUPBY_DIV gives inf or
 * NaN, a NaN stays NaN).
 *
 * An unknown op, sizes <= 0, G <= 0, a leading dimension below C, a group id outside [0, G) and a call too large for the grid are
 * SD_ERR_INVALID, refused before anything is allocated or launched. */
int sd_groupby_reduce_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int32_t* group,
                          int64_t G, double* sum_dev, int32_t* count_dev, int64_t ld_acc, int carry, double* out_dev_or_null, int64_t ld_out);
/* host buffers: src [T, C], out [G, C]; one shot: upload, run, download */
int sd_groupby_reduce(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group, int64_t G,
                      double* out_host);
int sd_groupby_apply_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, const int32_t* group,
                         int64_t G, const double* table_dev, int64_t ld_t, double* out_dev, int64_t ld_out);
/* host buffers: src [T, C], table [G, C], out [T, C]; upload, run, download */
int sd_groupby_apply(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group, int64_t G,
                     const double* table_host, double* out_host);

/* ---- rolling windows over the time axis: GridArray.rolling(time=w, center=..., min_periods=...).mean() / .sum() / .var() / .std() ----
 * pandas' fixed integer window per cell.  src is a [T, C] block (cells fastest, rows ld >= C elements apart; float64, or float32 with
 * src_is_f32 != 0, widened per sample in the kernel).  The window of row t is the rows t - back .. t - back + window - 1 (back =
 * window - 1: pandas' trailing window; back = window / 2: center=True), clipped to [0, T), or, with wrap != 0, taken modulo T (an
 * extension: pandas on the series padded from its other end).  The rows t0 .. t0 + n_out - 1 are written to out [n_out, C] float64
 * (rows ld_out >= C apart): a caller may hand over a block with its halo rows and ask for the interior only.
 *
 * A window is evaluated directly, in time order, over its non-NaN samples (n of them): s = ((+0.0 + x_a) + x_b) + ...;
 * SD_ROLLING_SUM s; SD_ROLLING_MEAN s / n, NaN where n == 0; SD_ROLLING_VAR q / (n - ddof) with q = sum of (x_i - s / n)^2 in the
 * same order from +0.0, NaN where n - ddof <= 0; SD_ROLLING_STD its square root.  The result is NaN where n < min_periods.  One IEEE
 * operation per step: a result depends on its own window only, so any cut of the time axis, any layout and any launch geometry give
 * the same bits.  The work is O(window) per output.
 *
 * An unknown op, sizes <= 0, window < 1, back outside [0, window), min_periods outside [0, window], ddof < 0, output rows outside
 * [0, T), wrap with window > T, a leading dimension below C and a call too large for the grid are SD_ERR_INVALID, refused before
 * anything is allocated or launched. */
int sd_rolling_dev(sd_ctx* ctx, int op, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, int64_t window, int64_t back,
                   int64_t min_periods, int64_t ddof, int wrap, int64_t t0, int64_t n_out, double* out_dev, int64_t ld_out);
/* host buffers: src [T, C], out [T, C]; the whole field in one call: upload, run, download */
int sd_rolling(sd_ctx* ctx, int op, const void* src_host, int src_is_f32, int64_t T, int64_t C, int64_t window, int64_t back,
               int64_t min_periods, int64_t ddof, int wrap, double* out_host);

/* ---- order statistics over the time axis: GridArray.quantile / .median (np.nanquantile / np.nanmedian per cell and group) --------
 * src is a [T, C] field (cells fastest, rows ld >= C elements apart; float64, or float32 with src_is_f32 != 0, widened per sample:
 * exact, so the result is that of the widened field).  group: host int32 [T] with every id in [0, G), or NULL: one group (G is then
 * not read and counts as 1).  q: host double [Q], every entry in [0, 1].  out [Q * G, C] float64 (rows ld_out >= C apart): row
 * q * G + g is quantile q of group g.
 *
 * Per (group, cell): v = the samples without NaN, ascending, n of them.  n == 0 gives NaN; with skipna == 0 any NaN in the group gives
 * NaN.  Otherwise h = (double)(n - 1) * q, lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1), a = v[lo], b = v[hi], d = b - a and
 * SD_QUANTILE_LINEAR g >= 0.5 ? b - d * (1 - g) : a + d * g; LOWER v[lo]; HIGHER v[ceil(h)]; NEAREST v[rint(h)] (half to even);
 * MIDPOINT v[lo] where h is whole, else b - d * 0.5; MEDIAN v[n / 2] for odd n, (v[n / 2 - 1] + v[n / 2]) / 2 for even n.  These
 * are the operations of NumPy 2's np.nanquantile(method=...) / np.nanmedian / np.quantile, one IEEE operation each: the result
 * equals NumPy's bit for bit for finite samples and depends neither on the order of a group's rows, nor on the layout, nor on the
 * launch geometry.  +-inf samples are ordinary values of the sort; the interpolation then follows IEEE arithmetic (inf - inf is NaN,
 * as in NumPy).  A group id that never occurs gives NaN.
 *
 * Groups of up to 1 344 rows are sorted one wave per (group, cell) on chip; longer ones, up to 19 456 rows, go through sorted runs in
 * 8 * C * (sum of the groups' lengths, each rounded up to whole runs) bytes of device scratch (SD_ERR_NOMEM where that fails);
 * beyond that the call is SD_ERR_UNSUPPORTED.  An unknown method, sizes <= 0, G <= 0, Q <= 0, a q outside [0, 1] (NaN included:
 * "Quantiles must be in the range [0, 1]"), a leading dimension below C, a group id outside [0, G), a call too large for the grid,
 * ld >= 2^29 and T >= 2^31 are SD_ERR_INVALID, refused before anything is allocated or launched. */
int sd_quantile_dev(sd_ctx* ctx, int method, int skipna, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C,
                    const int32_t* group_or_null, int64_t G, const double* q, int64_t Q, double* out_dev, int64_t ld_out);
/* host buffers: src [T, C], out [Q * G, C]; upload, run, download */
int sd_quantile(sd_ctx* ctx, int method, int skipna, const void* src_host, int src_is_f32, int64_t T, int64_t C, const int32_t* group_or_null,
                int64_t G, const double* q, int64_t Q, double* out_host);

/* ---- threshold and spell indices per period: GridArray.where(op, threshold).resample(time=rule).count() / .longest_spell() ... ----
 * src is a [T, C] field (cells fastest, rows ld >= C elements apart; float64, or float32 with src_is_f32 != 0).  The bins are those of
 * sd_resample: offsets, a host array of M + 1 entries that starts at 0, never decreases and ends at T.  The threshold of row r and
 * cell c is the scalar `threshold` (table NULL; ld_t, group and G are not read), or table[group[r] * ld_t + c] of a [G, C] float64
 * device table (rows ld_t >= C apart; `threshold` is not read); group: host int32 [T] with every id in [0, G), or NULL with G == 1:
 * row 0 for every row, a per-cell threshold.
 *
 * The rule, per cell over the steps of one bin in time order.  x is the sample widened to double, t the threshold as double.  A step
 * is valid when neither x nor t is NaN.  A step is a hit when it is valid and x (op) t holds: one IEEE comparison, +-inf are ordinary
 * values.  An invalid step is not a hit and ends a spell.  Spells are cut at the bin's ends: a bin is evaluated by itself (climdex's
 * spells.can.span.years = FALSE).  The state (valid, hits, run, longest, days, spells), all int32 and all zero at the bin's start, is
 * updated per step for the minimum spell length L = min_length >= 1:
 *     valid += is_valid;  hits += hit;  run = hit ? run + 1 : 0;  longest = max(longest, run)
 *     if (run == L) { days += L; spells += 1; } else if (run > L) days += 1;
 * out holds nstat float64 fields [M, C] (rows ld_out >= C apart, the fields stride_out >= M * ld_out elements apart): field s is the
 * statistic stats[s] (SD_SPELL_VALID .. SD_SPELL_SPELL_COUNT; a host array of nstat codes, 1 <= nstat <= 6), all from one pass over
 * src.  SD_SPELL_FRACTION is one division, NaN for a bin without a valid step; every other statistic of such a bin -- empty or
 * invalid throughout -- is 0.  All values are integers or one division of integers: the result is the same bit for bit whatever the
 * layout, the leading dimensions or the launch geometry.
 *
 * Deviation from NumPy 2: a float32 sample is compared after widening, against a double threshold.  NumPy compares a float32 array
 * with a Python float in float32: np.float32(0.1) > 0.1 is False there and True here.
 *
 * An unknown op or statistic code, nstat outside 1 .. 6, min_length < 1, sizes <= 0, T >= 2^31 (the counts are int32), a leading
 * dimension below C, stride_out < M * ld_out, G < 1, a NULL group with G > 1, a group id outside [0, G) and a table of bins that
 * breaks the rules above are SD_ERR_INVALID, refused before anything is allocated or launched. */
int sd_spells_dev(sd_ctx* ctx, const void* src_dev, int src_is_f32, int64_t ld, int64_t T, int64_t C, int op, double threshold,
                  const double* table_dev_or_null, int64_t ld_t, const int32_t* group_or_null, int64_t G, const int64_t* offsets, int64_t M,
                  int64_t min_length, const int* stats, int nstat, double* out_dev, int64_t ld_out, int64_t stride_out);
/* host buffers: src [T, C], table [G, C] or NULL, out [nstat * M, C]; upload, run, download */
int sd_spells(sd_ctx* ctx, const void* src_host, int src_is_f32, int64_t T, int64_t C, int op, double threshold,
              const double* table_host_or_null, const int32_t* group_or_null, int64_t G, const int64_t* offsets, int64_t M, int64_t min_length,
              const int* stats, int nstat, double* out_host);

/* ---- paired skill statistics per period: GridArray.compare(other).resample(time=rule).bias() / .rmse() / .corr() ... ----
 * a and b are [T, C] fields (cells fastest, rows ld_a, ld_b >= C elements apart; each float64, or float32 with its is_f32 != 0); they
 * may be the same pointer.  The bins are those of sd_resample: offsets, a host array of M + 1 entries that starts at 0, never
 * decreases and ends at T.  Nothing is aligned or broadcast: row r of a is paired with row r of b.
 *
 * The rule, per cell over the steps of one bin in time order.  A float32 sample is widened to double first.  A step is a valid pair
 * when neither a nor b is NaN; +-inf are ordinary values and IEEE arithmetic follows from them.  Every sum starts at +0.0 and adds one
 * term per valid pair in time order, ((+0.0 + t1) + t2) + ...; an invalid pair adds +0.0.  No contraction (-ffp-contract=off): a
 * product and the addition of it are two operations.
 *   pass 1:  n = the valid pairs;  sa = sum a;  sb = sum b;  sd = sum (a - b);  sabs = sum |a - b|;  sq = sum (a - b) * (a - b)
 *   pass 2 (only if SD_SKILL_CORR or SD_SKILL_STD_RATIO is asked for):  ma = sa / n, mb = sb / n;
 *            qaa = sum (a - ma) * (a - ma);  qbb = sum (b - mb) * (b - mb);  qab = sum (a - ma) * (b - mb)
 * out holds nstat float64 fields [M, C] (rows ld_out >= C apart, the fields stride_out >= M * ld_out elements apart): field s is the
 * statistic stats[s] (a host array of nstat codes, 1 <= nstat <= 7; a code may repeat):
 *   SD_SKILL_COUNT      n; 0 for an empty or all-invalid bin
 *   SD_SKILL_BIAS       sd / n
 *   SD_SKILL_RATIO      sa / sb as IEEE gives it
 *   SD_SKILL_MAE        sabs / n
 *   SD_SKILL_RMSE       sqrt(sq / n)
 *   SD_SKILL_CORR       qab / (sqrt(qaa) * sqrt(qbb)) clamped to [-1, 1], NaN staying NaN; NaN where n < 2, qaa == 0 or qbb == 0
 *   SD_SKILL_STD_RATIO  sqrt(qaa / qbb); NaN where n < 2
 * Every statistic but SD_SKILL_COUNT is NaN where n == 0.  Each value is one fixed sequence of IEEE operations: the result is the
 * same bit for bit whatever the layout, the leading dimensions or the launch geometry.
 *
 * An unknown statistic code, nstat outside 1 .. 7, sizes <= 0, T >= 2^31 (the counts are int32), a leading dimension below C,
 * stride_out < M * ld_out, a field too large and a table of bins that breaks the rules above are SD_ERR_INVALID, in this order,
 * refused before anything is allocated or launched. */
int sd_skill_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T,
                 int64_t C, const int64_t* offsets, int64_t M, const int* stats, int nstat, double* out_dev, int64_t ld_out,
                 int64_t stride_out);
/* host buffers: a, b [T, C], out [nstat * M, C]; upload, run, download */
int sd_skill(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C,
             const int64_t* offsets, int64_t M, const int* stats, int nstat, double* out_host);

/* ---- paired skill statistics per group of steps: GridArray.compare(other).groupby("time.month").bias() / .rmse() / .corr() ... ----
 * The fields, the statistics and the output are those of sd_skill, with groups in place of bins: group is a host int32 [T] with every
 * id in [0, G), as for sd_groupby_reduce and sd_quantile, and out holds nstat float64 fields [G, C]: row s * G + g (for a contiguous
 * output) is statistic stats[s] of group g.  Both fields are whole in device memory for the call.
 *
 * The rule: group g is evaluated exactly as sd_skill evaluates one bin whose steps are the rows t with group[t] == g in ascending t.
 * So the call on (a, b) equals sd_skill on the fields gathered group by group, (a[rows], b[rows], offsets) with rows / offsets the
 * stable counting sort of the ids, bit for bit; where the groups are runs of consecutive rows it equals sd_skill with those offsets.
 * A group id that never occurs is an empty bin: SD_SKILL_COUNT is 0, everything else NaN.
 *
 * The refusals of sd_skill that depend on codes and sizes (T, C; G takes the place of M in the stride and size checks), then G <= 0,
 * then a group id outside [0, G) are SD_ERR_INVALID, in this order, refused before anything is allocated or launched.  One launch of
 * skill_groups_kernel; the row table costs 8 * T bytes per tile of cells beside the bytes of sd_skill. */
int sd_skill_groups_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T,
                        int64_t C, const int32_t* group, int64_t G, const int* stats, int nstat, double* out_dev, int64_t ld_out,
                        int64_t stride_out);
/* host buffers: a, b [T, C], out [nstat * G, C]; upload, run, download */
int sd_skill_groups(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C,
                    const int32_t* group, int64_t G, const int* stats, int nstat, double* out_host);

/* ---- distribution scores per period: GridArray.compare(other).ks() / .perkins(width) / .distribution(names) ----
 * a and b are [T, C] fields (cells fastest, rows ld_a, ld_b >= C elements apart; each float64, or float32 with its is_f32 != 0); they
 * may be the same pointer.  The bins are those of sd_skill: offsets, a host array of M + 1 entries that starts at 0, never decreases
 * and ends at T.
 *
 * The rule, per cell and bin.  A float32 sample is widened to double first.  Unlike sd_skill, which drops a step where either sample
 * is NaN, each field contributes its OWN non-NaN samples: na and nb may differ, and a NaN in a does not remove the sample of b at
 * that step (the two-sample definition: scipy.stats.ks_2samp on the two series with NaN dropped).  +-inf are ordinary values.  With
 * a_0 <= ... <= a_{na-1} the sorted samples of a, le(x) the number of samples of b <= x and lt(x) the number < x:
 *   SD_TWOSAMPLE_KS       num = max over i of max((i + 1) * nb - le(a_i) * na, lt(a_i) * na - i * nb) in int64;
 *                         D = (double)num / ((double)na * (double)nb), one division.  Evaluating at the points of a alone is enough
 *                         (Fa - Fb takes its maximum at a jump of Fa and its minimum just before one); ties need no special case;
 *                         the value is symmetric in a and b.
 *   SD_TWOSAMPLE_PERKINS  the histogram bin of a sample is k(x) = floor((x - origin) / width) in double: one subtraction, one
 *                         division, one floor; k is monotone in x and +-inf fall in bins of their own.  With ca_k, cb_k the
 *                         samples of a and b in bin k:  num = sum over the distinct k present in a of min(ca_k * nb, cb_k * na)
 *                         in int64;  PSS = (double)num / ((double)na * (double)nb).  width > 0 and origin are finite doubles,
 *                         read only where this code is asked for.
 *   SD_TWOSAMPLE_NA, SD_TWOSAMPLE_NB  the two counts; 0 for an empty or all-NaN bin.
 * KS and Perkins are NaN where na == 0 or nb == 0.  out holds nstat float64 fields [M, C] (rows ld_out >= C apart, the fields
 * stride_out >= M * ld_out elements apart): field s is the statistic stats[s] (a host array of nstat codes, 1 <= nstat <= 4; a code
 * may repeat).  Everything is integer arithmetic followed by one division: the result is the same bit for bit whatever the layout,
 * the leading dimensions, the path or the launch geometry.
 *
 * Bins of up to 1 216 rows are sorted one wave per (bin, cell) on chip, both fields side by side; longer ones, up to 19 456 rows, go
 * through sorted runs in 16 * C * (sum of the bins' lengths, each rounded up to whole runs) bytes of device scratch (SD_ERR_NOMEM
 * where that fails); a longer bin is SD_ERR_UNSUPPORTED.  Both fields are whole in device memory for the call: one bin over the whole
 * axis needs both whole [T, C] fields there.
 *
 * An unknown statistic code, nstat outside 1 .. 4; with Perkins a width that is not finite or <= 0 or an origin that is not finite;
 * sizes <= 0, T >= 2^31; a leading dimension below C, stride_out < M * ld_out; a field too large; a table of bins that breaks the
 * rules above are SD_ERR_INVALID, in this order, then the bin beyond 19 456 rows (SD_ERR_UNSUPPORTED), then the LDS and grid limits
 * and ld >= 2^29: all refused before anything is allocated or launched. */
int sd_twosample_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b, int64_t T,
                     int64_t C, const int64_t* offsets, int64_t M, const int* stats, int nstat, double width, double origin,
                     double* out_dev, int64_t ld_out, int64_t stride_out);
/* host buffers: a, b [T, C], out [nstat * M, C]; upload, run, download */
int sd_twosample(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C,
                 const int64_t* offsets, int64_t M, const int* stats, int nstat, double width, double origin, double* out_host);

/* ---- distribution scores per group of steps: GridArray.compare(other).groupby("time.season").ks() / .perkins(width) ----
 * sd_twosample with groups in place of bins: group is a host int32 [T] with every id in [0, G), out holds nstat float64 fields [G, C].
 *
 * The rule: group g is evaluated exactly as sd_twosample evaluates one bin whose steps are the rows t with group[t] == g in ascending
 * t; the call equals sd_twosample on the gathered fields (a[rows], b[rows], offsets), bit for bit, and sd_twosample itself where the
 * groups are runs of consecutive rows.  A group id that never occurs is an empty bin: na and nb are 0, KS and Perkins NaN.  The same
 * kernels serve it, reading their rows through the group-sorted row table: groups of up to 1 216 rows on chip, longer ones, up to
 * 19 456 rows, through 16 * C * (sum of the groups' lengths, each rounded up to whole runs) bytes of sorted runs in device scratch.
 * Both fields are whole in device memory for the call.
 *
 * The refusals of sd_twosample that depend on codes and sizes, then G <= 0, then a group id outside [0, G) are SD_ERR_INVALID; then a
 * group of more than 19 456 rows is SD_ERR_UNSUPPORTED; then the LDS and grid limits and ld >= 2^29: in this order, all refused
 * before anything is allocated or launched. */
int sd_twosample_groups_dev(sd_ctx* ctx, const void* a_dev, int a_is_f32, int64_t ld_a, const void* b_dev, int b_is_f32, int64_t ld_b,
                            int64_t T, int64_t C, const int32_t* group, int64_t G, const int* stats, int nstat, double width,
                            double origin, double* out_dev, int64_t ld_out, int64_t stride_out);
/* host buffers: a, b [T, C], out [nstat * G, C]; upload, run, download */
int sd_twosample_groups(sd_ctx* ctx, const void* a_host, int a_is_f32, const void* b_host, int b_is_f32, int64_t T, int64_t C,
                        const int32_t* group, int64_t G, const int* stats, int nstat, double width, double origin, double* out_host);

/* ---- constructed analogs: ConstructedAnalogs (Hidalgo et al. 2008; Maurer et al. 2010), the operation under BCCA, MACA and LOCA ----
 * For each target day: the k library days whose coarse pattern is closest (sd_ca_select_dev), the regression of the target pattern on
 * those k patterns (sd_ca_weights_dev), and the k weights applied to the fine fields of the same days (sd_ca_apply_dev).
 *
 * Inputs.  L [Tl, Cc] float64 the coarse library, Q [Tq, Cc] float64 the coarse targets, F [Tl, Cf] the fine library (float64, or
 * float32 with f_is_f32 != 0, widened to double per sample): device buffers, row-major, rows ld_l / ld_q / ld_f elements apart.
 * wc [Cc] float64 column weights, finite and >= 0; key_l [Tl], key_q [Tq] int32 candidate keys; excl_l [Tl], excl_q [Tq] int32
 * exclusion ids: small tables in HOST memory, like the group ids of the other calls.  k in [1, 32] analogs; ridge >= 0; kind
 * SD_CA_REGRESSION or SD_CA_MEAN; period and window integers.
 *
 * The rule.  No contraction (-ffp-contract=off): a product and the addition of it are two operations.
 *  1. Valid columns.  Column c is used when L[:, c] is finite in every row and wc[c] > 0.  The used columns keep their ascending
 *     order.  If no column is used the call fails with SD_ERR_INVALID.
 *  2. Candidates.  Library day t is a candidate of target q when both hold: window < 0, or min(|a - b|, period - |a - b|) <= window
 *     with a = key_q[q], b = key_l[t] (in int64); and excl_q[q] < 0, or excl_l[t] != excl_q[q].
 *  3. Distance.  d(q, t) = ((+0.0 + wc[c0] * (e0 * e0)) + wc[c1] * (e1 * e1)) + ... over the used columns in ascending order, with
 *     e = Q[q, c] - L[t, c].  The expansion |q|^2 + |l|^2 - 2 q.l is excluded on purpose: on fields near 280 K its cancellation would
 *     decide which of two near-equal days is picked.
 *  4. Selection.  The analogs of q are the k candidates smallest by (d, t) in lexicographic order, listed in that order: ties go to
 *     the lower t, so the result cannot depend on how the library is tiled.
 *  5. kind = SD_CA_MEAN: every weight is 1.0 / k.
 *  6. kind = SD_CA_REGRESSION: with a_i the library row of analog i,
 *       G[i][j] = sum_c wc[c] * (a_i[c] * a_j[c]),  b[i] = sum_c wc[c] * (a_i[c] * Q[q, c]),
 *     both over the used columns in ascending order from +0.0; lambda = ridge * ((G[0][0] + G[1][1] + ...) / k) (the trace summed from
 *     G[0][0] in ascending order), G[i][i] += lambda.  Lower Cholesky factor row by row: for i, for j <= i:
 *       s = G[i][j]; for p < j in ascending order: s -= C[i][p] * C[j][p];  j < i: C[i][j] = s / C[j][j];  j == i: the pivot s must be
 *       > 0 (NaN is not), C[i][i] = sqrt(s).
 *     Forward: for i ascending: s = b[i]; for p < i ascending: s -= C[i][p] * y[p]; y[i] = s / C[i][i].
 *     Back: for i descending: s = y[i]; for p = i + 1 .. k - 1 ascending: s -= C[p][i] * w[p]; w[i] = s / C[i][i].
 *     tests/_constructed_oracle.py is normative for the order of every operation.
 *  7. Status per target, the first that applies: SD_CA_QUERY_NONFINITE a used column of Q[q] is not finite; SD_CA_FEW_CANDIDATES
 *     there are fewer than k candidates; SD_CA_SINGULAR a pivot is not > 0; else SD_CA_OK.  Any status other than OK gives indices -1,
 *     NaN distances and weights, and a NaN output row.
 *  8. Synthesis.  out[q, f] = ((+0.0 + w_0 * F[i_0, f]) + w_1 * F[i_1, f]) + ... in analog order.  NaN in F propagates by IEEE
 *     arithmetic with no special case; -0.0 becomes +0.0.  A row whose first index lies outside [0, Tl) is a NaN row.
 * Every value is one fixed sequence of IEEE operations: the result is the same bit for bit whatever the leading dimensions, the tiling
 * of the library or of the targets, and the cut [q0, q1) of an apply call.
 *
 * sd_ca_select_dev: steps 1 to 4 -> idx int32 [Tq, k], dist float64 [Tq, k], status int32 [Tq] (device, contiguous).
 * sd_ca_weights_dev: steps 5 to 7 from idx -> weights float64 [Tq, k]; updates status, and idx / dist of a singular target.
 * sd_ca_apply_dev: step 8 for the target rows [q0, q1): idx and weights are the whole [Tq, k] tables, out_dev points at row q0, rows
 * ld_out >= Cf apart.
 *
 * NULL pointers, sizes <= 0, k outside [1, 32], a leading dimension below the row length, wc negative or not finite, period <= 0 with
 * window >= 0, an unknown kind, ridge negative or not finite, rows outside [0, Tq) are SD_ERR_INVALID; Tl > 2^24 or Cc > 2^16 are
 * SD_ERR_UNSUPPORTED: all refused before anything is allocated or launched.  Out of scope: MACA's epoch adjustment and multivariate
 * patterns, k > 32.  (LOCA's per-cell choice of analogs is the section below.) */
#define SD_CA_REGRESSION 0
#define SD_CA_MEAN 1
#define SD_CA_OK 0
#define SD_CA_QUERY_NONFINITE 1
#define SD_CA_FEW_CANDIDATES 2
#define SD_CA_SINGULAR 3
int sd_ca_select_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t Cc,
                     const double* wc, int k, const int32_t* key_l, const int32_t* key_q, int64_t period, int64_t window,
                     const int32_t* excl_l, const int32_t* excl_q, int32_t* idx_dev, double* dist_dev, int32_t* status_dev);
int sd_ca_weights_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t Cc,
                      const double* wc, int k, int kind, double ridge, int32_t* idx_dev, double* dist_dev, double* weights_dev,
                      int32_t* status_dev);
int sd_ca_apply_dev(sd_ctx* ctx, const void* F_dev, int f_is_f32, int64_t ld_f, int64_t Tl, int64_t Cf, const int32_t* idx_dev,
                    const double* weights_dev, int64_t Tq, int k, int64_t q0, int64_t q1, double* out_dev, int64_t ld_out);

/* ---- localized analogs: LocalizedAnalogs (LOCA, Pierce et al. 2014): one library day per coarse cell instead of one blend per day ----
 * From the k regional analogs of a target day (sd_ca_select_dev) every coarse cell keeps the one that matches the target best in the
 * neighbourhood of that cell (sd_ca_local_dev); the fine field copies, cell by cell, the fine library of the day chosen for the coarse
 * cell it lies in, shifted or scaled to the coarse target (sd_ca_local_apply_dev).
 *
 * Inputs.  L [Tl, Cc], Q [Tq, Cc], wc [Cc], k and idx [Tq, k] as sd_ca_select_dev left them.  The coarse grid is ny x nx with
 * Cc == ny * nx, column c = i * nx + j (row-major).  Radii ry >= 0 and rx >= 0 in coarse cells.  cell_of [Cf] int32 (device): the
 * coarse column of every fine cell.
 *
 * The rule.  No contraction, as above.  tests/_localized_oracle.py is normative for the order of every operation.
 *  L1. Used columns: step 1 of the constructed rule (no used column: SD_ERR_INVALID).
 *  L2. Local distance of target q, analog slot a in 0 .. k - 1 with t = idx[q, a], and coarse cell (i, j):
 *        dl = +0.0; for i' ascending over max(0, i - ry) .. min(ny - 1, i + ry): for j' ascending over max(0, j - rx) ..
 *        min(nx - 1, j + rx): with c' = i' * nx + j': if c' is used: e = Q[q, c'] - L[t, c'], dl = dl + wc[c'] * (e * e).
 *      A column that is not used is skipped, not weighted 0: its e may be NaN.
 *  L3. Choice.  slot[q, c] is the lowest a at which dl is smallest (a ascending, replaced on strict <: ties go to the regionally
 *      closer day); local_idx[q, c] = idx[q, slot] (int32), local_dist[q, c] that dl.  Every coarse cell gets a choice, the unused
 *      ones too; a neighbourhood without a used column gives +0.0 for every slot, hence slot 0.  A target with idx[q, 0] < 0 (any
 *      status other than OK) -- or, for a table that sd_ca_select_dev did not make, with any index outside [0, Tl) -- gives
 *      local_idx = -1 and local_dist = NaN for the whole row.
 *  L4. Synthesis.  With c = cell_of[f]: out[q, f] = NaN where c lies outside [0, Cc) or local_idx[q, c] outside [0, Tl).
 *      Otherwise t = local_idx[q, c], v = (double) F[t, f], and
 *        SD_CA_ADJUST_NONE:  out = v;
 *        SD_CA_ADJUST_SHIFT: out = v + (Q[q, c] - L[t, c]);
 *        SD_CA_ADJUST_SCALE: r = Q[q, c] / L[t, c] if L[t, c] > 0, else 1.0; if max_scale > 0 and r > max_scale: r = max_scale;
 *                            out = v * r.
 *      NaN in F, Q or L propagates by IEEE arithmetic with no special case (an unused coarse column under SHIFT / SCALE).
 * Every value is one fixed sequence of IEEE operations: the result is the same bit for bit whatever the leading dimensions, the tiling
 * and the cut [q0, q1) of an apply call.
 *
 * sd_ca_local_dev: L1 to L3 -> local_idx int32 [Tq, ny * nx], local_dist float64 [Tq, ny * nx] (device, contiguous).
 * sd_ca_local_apply_dev: L4 for the target rows [q0, q1): local_idx is the whole [Tq, Cc] table, out_dev points at row q0, rows
 * ld_out >= Cf apart.  L_dev and Q_dev may be NULL with SD_CA_ADJUST_NONE only.
 *
 * NULL pointers, sizes <= 0, k outside [1, 32], a negative radius, a leading dimension below the row length, wc negative or not
 * finite, an unknown adjust, max_scale NaN or negative (0: no limit), rows outside [0, Tq) are SD_ERR_INVALID; Tl > 2^24 or a coarse
 * grid of more than SD_CA_LOCAL_MAX_CELLS cells (what the local kernel stages of one target must fit the LDS of a workgroup) are
 * SD_ERR_UNSUPPORTED: all refused before anything is allocated or launched.  Out of scope: LOCA's smoothing across the boundaries
 * between different analog days, its multivariate and bias-correction steps, curvilinear grids. */
#define SD_CA_ADJUST_NONE 0
#define SD_CA_ADJUST_SHIFT 1
#define SD_CA_ADJUST_SCALE 2
#define SD_CA_LOCAL_MAX_CELLS 4096
int sd_ca_local_dev(sd_ctx* ctx, const double* L_dev, int64_t ld_l, int64_t Tl, const double* Q_dev, int64_t ld_q, int64_t Tq, int64_t ny,
                    int64_t nx, const double* wc /* host [ny * nx] */, int k, int64_t ry, int64_t rx, const int32_t* idx_dev /* [Tq, k] */,
                    int32_t* local_idx_dev /* [Tq, ny * nx] */, double* local_dist_dev /* [Tq, ny * nx] */);
int sd_ca_local_apply_dev(sd_ctx* ctx, const void* F_dev, int f_is_f32, int64_t ld_f, int64_t Tl, int64_t Cf, const int32_t* cell_of_dev,
                          const int32_t* local_idx_dev, int64_t Cc, const double* L_dev, int64_t ld_l, const double* Q_dev, int64_t ld_q,
                          int adjust, double max_scale, int64_t Tq, int64_t q0, int64_t q1, double* out_dev, int64_t ld_out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (no PyTorch) -----------------------------------
 * The reference's only parallelism is dask's map_blocks over spatial chunks (core.py:256-262, 300-336) and a client-side
 * collection of the result; here cells are block-partitioned over the ranks of one node, fit / predict need no exchange
 * (cells are independent, core.py:87), and the predicted shards are gathered to a root GPU.
 * Bootstrap: rank 0 calls sd_comm_unique_id and hands the 128 bytes to the other ranks by any channel (the Python side
 * uses a TCP socket next to MASTER_PORT); every rank then calls sd_comm_create on its own context.
 * sd_comm_gather_field: every rank contributes one contiguous [T, cells[rank]] float64 field; the root receives block r at
 * offset sum_{q<r} T * cells[q] of root_dev (layout [rank][T][C_r]: no padding, no concatenation copy).  The transfer is
 * ordered behind the work already queued on the context and runs on the communicator's own stream: with wait = 0 the next
 * chunk of cells can be computed meanwhile, sd_comm_wait joins. */
int sd_comm_unique_id(char* id /* [SD_COMM_ID_BYTES] */);
int sd_comm_create(sd_ctx* ctx, const char* id /* [SD_COMM_ID_BYTES] */, int rank, int world, sd_comm** out);
int sd_comm_destroy(sd_comm* comm);
int sd_comm_info(const sd_comm* comm, int* rank, int* world);
/* what RCCL reports about the communicator: ncclGetVersion's code, ncclCommCount (the ranks RCCL sees) and its device */
int sd_comm_rccl_info(const sd_comm* comm, int* version, int* ranks, int* device);
int sd_comm_barrier(sd_comm* comm);
int sd_comm_allreduce_max(sd_comm* comm, double value, double* result);
int sd_comm_gather_field(sd_comm* comm, const double* local_dev, int64_t T, const int64_t* cells /* [world] */,
                         double* root_dev /* root only */, int root, int wait);
int sd_comm_wait(sd_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* SD_DOWNSCALE_H */
