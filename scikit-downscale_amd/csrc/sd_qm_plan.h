// Launch plan of a quantile-mapping call (QuantileMappingReressor, EquidistantCdfMatcher, CunnaneTransformer): which kernels
// run, with which widths, grids and LDS sizes, and every refusal that depends only on sizes and codes.  All of it is integer
// arithmetic on the call's sizes, the LDS size and the CU count, written once here as a pure host function (no HIP header:
// tests/qm_plan_check.cpp compiles it with g++ alone).  The entry points of sd_qm.hip validate their pointers, build the call,
// plan, allocate and run; the launchers map the plan's widths to instantiations and take every grid, block and LDS size from the
// functions of qm_launches below.
//
// Fit:     tile-shaped first stage where a tile width serves the series (qm_tile_runs_kernel<Kt> + qm_merge_runs_kernel<Kt>: at
//          most 16 runs of 64 * Kt samples), else qm_transpose_kernel + qm_sort_kernel<K>; once for X, once more with y.
// Predict: transpose in, qm_rank_kernel<rank_K> (EquidistantCdfMatcher only), two qm_ppcheck_kernel launches, qm_tails_kernel
//          ('min' / 'max' / 'both'), qm_map_kernel, untranspose, status fold.
// Cunnane: transpose in, qm_cunnane_kernel, untranspose, status fold.
//
// What depends on data stays in the launcher: qm_map_kernel has a FAST instantiation (plotting positions by a correction step
// instead of the division) and a dividing one, and the launcher takes FAST only if qm_ppcheck_kernel has reported from the device
// that the correction step reproduces the division on both grids.  The plan carries only the `divide` switch that rules FAST out.
// The NULL-argument checks stay at the entry points, which read the state to build the call (T, C and whether it holds y: a
// predict on a state fitted without y is refused at the place the entry point always refused it, between the model and the sizes).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"
#include "sd_wave_consts.h"

// ---- sizing constants and functions of the quantile-mapping kernels (one definition each) ----------------------------------------
namespace sdqm {

constexpr int kSortWidths[] = {1, 3, 5, 9, 13, 15, 17, 19};  // qm_sort_kernel<K>, qm_rank_kernel<K>: K samples per thread
constexpr int kTileWidths[] = {13, 15, 17};                  // qm_tile_runs_kernel<K>, qm_merge_runs_kernel<K>
constexpr int kMaxRuns = 16;                                 // runs of 64 * K samples a 1 024-thread workgroup merges
constexpr int kSortThreads = 1024;
constexpr int kMapPerQmr = 16, kMapPerEdcdf = 8;             // kMapPer of qm_map_kernel: samples per thread and pass
constexpr int64_t kGridLimit = (int64_t)1 << 31;

// padded length of the workgroup sort of width K
inline int sort_np(int K, int64_t T) { return (int)((T + K - 1) / K * K); }
// narrowest instantiated width with T <= 1024 * K whose keys fit the LDS; 0: none
inline int sort_width(int64_t T, size_t lds_max) {
    for (int K : kSortWidths)
        if (T <= (int64_t)kSortThreads * K && sdw::block_sort_lds_bytes(sort_np(K, T)) <= lds_max) return K;
    return 0;
}
// narrowest width of the tile-shaped fit stage: at most kMaxRuns runs, and the merge must fit the LDS; 0: none
inline int tile_runs_width(int64_t T, size_t lds_max) {
    for (int K : kTileWidths)
        if (sdw::tile_sort_chunks(K, T) <= kMaxRuns && sdw::block_sort_lds_bytes(sdw::tile_sort_np(K, T)) <= lds_max) return K;
    return 0;
}

}  // namespace sdqm

// ---- the plan --------------------------------------------------------------------------------------------------------------
enum class QmOp { Fit, Predict, Cunnane };

// Switches of the development library (environment variables, read in one place: sd_qm_dev_switches() of sd_internal.h); the
// production library keeps the defaults.
struct QmDevSwitches {
    bool no_tile = false;  // SD_QM_NOTILE: the staging transpose + workgroup sort for every fit
    bool divide = false;   // SD_QM_DIVIDE: the dividing instantiation of qm_map_kernel whatever qm_ppcheck_kernel reports
    bool trace = false;    // SD_QM_TRACE: print the phase clocks of qm_map_kernel
};

struct QmCall {
    QmOp op = QmOp::Fit;
    int64_t T = 0, Tp = 0, C = 0;  // fitted series, new series, cells
    int64_t ld = 0, ld_out = 0;    // leading dimensions of the input field(s) and of the output
    bool has_y = false;            // fit: y given; predict: the state holds sorted y
    int model = SD_QM_REGRESSOR, extrapolate = SD_EXTRAP_NONE, n_endpoints = 10, direction = SD_CUNNANE_FORWARD;
    size_t lds_max = 0;
    int cu_count = 0;
    QmDevSwitches dev;
};

struct QmLaunch {
    int64_t gx, gy;
    int block;
    size_t lds;  // dynamic LDS bytes
};

struct QmPlan {
    int error = SD_OK;  // an error code, with its message: nothing is allocated, nothing runs
    char message[256] = "";
    // fit
    int K = 0;              // width of qm_sort_kernel
    bool tiled = false;     // the tile-shaped first stage runs instead of transpose + sort
    int Kt = 0, nchunks = 0, np = 0;  // its width, runs per cell and padded run length (slots per cell of the runs buffer)
    size_t runs_bytes = 0;
    // predict
    int rank_K = 0;         // width of qm_rank_kernel (0: the regressor needs no ranks)
    bool tails = false;     // qm_tails_kernel runs
    int map_per = 0;        // kMapPer of the qm_map_kernel instantiation
    // predict and Cunnane: dynamic LDS and grid of qm_map_kernel / qm_cunnane_kernel
    size_t lds = 0;
    int64_t nb = 0;
    bool divide = false, trace = false;
};

namespace qm_plan_detail {
using namespace sdqm;

template <class... A>
bool fail(QmPlan* pl, int code, const char* fmt, A... a) {
    snprintf(pl->message, sizeof pl->message, fmt, a...);
    pl->error = code;
    return false;
}
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
// one workgroup per CU when a workgroup takes more than half of the LDS, two otherwise; never more than the cells
inline int64_t per_cell_blocks(const QmCall& c, size_t lds) { return min64(c.C, (int64_t)c.cu_count * (lds > c.lds_max / 2 ? 1 : 2)); }

inline bool plan_fit(const QmCall& c, QmPlan* pl) {
    if (!(c.T >= 2 && c.C > 0 && c.ld >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_fit: bad sizes");
    pl->K = sort_width(c.T, c.lds_max);
    if (pl->K == 0) return fail(pl, SD_ERR_UNSUPPORTED, "sd_qm_fit: series of %lld samples exceed the workgroup sort (19456)", (long long)c.T);
    pl->Kt = c.dev.no_tile ? 0 : tile_runs_width(c.T, c.lds_max);
    pl->tiled = pl->Kt != 0;
    if (pl->tiled) {
        pl->nchunks = (int)sdw::tile_sort_chunks(pl->Kt, c.T);
        pl->np = sdw::tile_sort_np(pl->Kt, c.T);
        pl->runs_bytes = sizeof(double) * (size_t)pl->np * (size_t)c.C;
        if (sdw::tiled_blocks(c.C, pl->nchunks) >= kGridLimit) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_fit: grid too large");
    }
    return true;
}

inline bool plan_predict(const QmCall& c, QmPlan* pl) {
    if (!(c.extrapolate == SD_EXTRAP_1TO1 || (c.extrapolate >= SD_EXTRAP_NONE && c.extrapolate <= SD_EXTRAP_BOTH)))
        return fail(pl, SD_ERR_INVALID, "sd_qm_predict: unknown extrapolate code %d", c.extrapolate);
    if (!(c.n_endpoints >= 2)) return fail(pl, SD_ERR_INVALID, "%s", "Invalid number of n_endpoints, must be >= 2");
    if (!(c.model >= SD_QM_REGRESSOR && c.model <= SD_QM_EDCDF_RATIO)) return fail(pl, SD_ERR_INVALID, "sd_qm_predict: unknown model %d", c.model);
    if (!c.has_y) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_predict: the state was fitted without y");
    if (!(c.Tp > 0 && c.ld >= c.C && c.ld_out >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_predict: bad sizes");
    const bool qmr = c.model == SD_QM_REGRESSOR;
    pl->rank_K = qmr ? 0 : sort_width(c.Tp, c.lds_max);
    if (!qmr && pl->rank_K == 0)
        return fail(pl, SD_ERR_UNSUPPORTED, "sd_qm_predict: series of %lld samples exceed the workgroup sort (19456)", (long long)c.Tp);
    pl->lds = sizeof(double) * (size_t)c.T;  // one table of the fit at a time (qm_map_kernel)
    if (pl->lds > c.lds_max) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_predict: fitted series too long for the LDS-resident search");
    if (c.Tp >= kGridLimit) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_predict: series too long");  // (qm_map_kernel indexes a series with int)
    pl->tails = (c.extrapolate & (SD_EXTRAP_MIN | SD_EXTRAP_MAX)) != 0 && c.extrapolate != SD_EXTRAP_1TO1;
    pl->map_per = qmr ? kMapPerQmr : kMapPerEdcdf;
    pl->nb = per_cell_blocks(c, pl->lds);
    return true;
}

inline bool plan_cunnane(const QmCall& c, QmPlan* pl) {
    if (!(c.direction == SD_CUNNANE_FORWARD || c.direction == SD_CUNNANE_INVERSE))
        return fail(pl, SD_ERR_INVALID, "sd_qm_cunnane: unknown direction %d", c.direction);
    if (!(c.extrapolate >= SD_EXTRAP_NONE && c.extrapolate <= SD_EXTRAP_BOTH))
        return fail(pl, SD_ERR_INVALID, "sd_qm_cunnane: unknown extrapolate code %d", c.extrapolate);
    if (!(c.n_endpoints >= 1)) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_cunnane: n_endpoints must be positive");
    if (!(c.Tp > 0 && c.ld >= c.C && c.ld_out >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_cunnane: bad sizes");
    // forward: the sorted fit values in LDS for the value -> index search; inverse: the bracket is analytic
    pl->lds = c.direction == SD_CUNNANE_FORWARD ? sizeof(double) * (size_t)c.T : 8;
    if (pl->lds > c.lds_max) return fail(pl, SD_ERR_INVALID, "%s", "sd_qm_cunnane: fitted series too long for the LDS-resident search");
    pl->nb = per_cell_blocks(c, pl->lds);
    return true;
}

}  // namespace qm_plan_detail

inline QmPlan qm_plan(const QmCall& c) {
    QmPlan pl;
    pl.divide = c.dev.divide;
    pl.trace = c.dev.trace;
    switch (c.op) {
        case QmOp::Fit: qm_plan_detail::plan_fit(c, &pl); break;
        case QmOp::Predict: qm_plan_detail::plan_predict(c, &pl); break;
        case QmOp::Cunnane: qm_plan_detail::plan_cunnane(c, &pl); break;
    }
    return pl;
}

// ---- geometry of the launches: one function per launch, used by the launchers for grid, block and LDS; the order of the launches and
// their profiler names are the launchers' -----------------------------------------------------------------------------------------
namespace qm_launches {
using namespace sdqm;
inline int64_t strided_cells(int64_t C, int cu_count) { return C < (int64_t)cu_count * 4 ? C : (int64_t)cu_count * 4; }

// qm_transpose_kernel / qm_untranspose_kernel: 32 x 32 tiles of a [T, C] field
inline QmLaunch transpose(int64_t C, int64_t T) { return {(C + 31) / 32, (T + 31) / 32, 256, 0}; }
inline QmLaunch untranspose(int64_t C, int64_t T) { return transpose(C, T); }
// qm_sort_kernel<K> / qm_rank_kernel<K>: cells strided over four workgroups per CU
inline QmLaunch sort(int K, int64_t T, int64_t C, int cu_count) {
    return {strided_cells(C, cu_count), 1, kSortThreads, sdw::block_sort_lds_bytes(sort_np(K, T))};
}
inline QmLaunch rank(int K, int64_t T, int64_t C, int cu_count) { return sort(K, T, C, cu_count); }
inline QmLaunch tile_runs(const QmPlan& pl, int64_t C) {
    return {sdw::tiled_blocks(C, pl.nchunks), 1, sdw::kThreads, sdw::tile_sort_lds_bytes(pl.Kt)};
}
inline QmLaunch merge_runs(const QmPlan& pl, int64_t C, int cu_count) {
    return {strided_cells(C, cu_count), 1, kSortThreads, sdw::block_sort_lds_bytes(pl.np)};
}
inline QmLaunch ppcheck(int64_t n) { return {(n + 255) / 256, 1, 256, 0}; }
inline QmLaunch tails(int64_t C) { return {(C + 255) / 256, 1, 256, 0}; }
inline QmLaunch map(const QmPlan& pl) { return {pl.nb, 1, 1024, pl.lds}; }
inline QmLaunch cunnane(const QmPlan& pl) { return {pl.nb, 1, 1024, pl.lds}; }
inline QmLaunch status_public(int64_t C) { return {(C + 255) / 256, 1, 256, 0}; }

}  // namespace qm_launches
