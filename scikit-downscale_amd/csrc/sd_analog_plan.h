// Launch plan of a GARD analog call (PureAnalog / AnalogRegression): which kernels run, with which widths, grids and LDS sizes.  Everything that can be decided before the first launch is integer arithmetic on the call's sizes, the
// facts of the fitted state and the LDS size, written once here as a pure host function (no HIP header:
// tests/analog_plan_check.cpp compiles it with g++ alone).  The launchers of sd_analog.hip and the sd_analog_*.h headers map
// the plan's decisions to instantiations and take every grid, block and LDS size from the functions of analog_launches below.
//
// Predict paths:
//   F == 1, sorted view in the state, no neighbour outputs, not 'sample_analogs', not a thresholded regression ("window" calls;
//   one persistent workgroup per cell, queries and outputs through cell-major staging, 16 384 cells per chunk):
//     Mean3   analog_f1_mean3_kernel<PER>: mean_analogs without a threshold, or a single analog (PER 8 / 16 / 20 by T)
//     Mean    analog_f1_mean_kernel: AnalogRegression (k >= 3), weighted / thresholded kinds (qsplit workgroups per cell,
//             reg_direct: window summed directly instead of prefix differences)
//     Window  analog_f1_window_kernel: the other kinds, npass value ranges
//   Walk      analog_f1_predict_kernel: every other F == 1 call on a sorted view
//   Slab      F > 1 with the feature-0 sorted copy: analog_slab_topk_kernel (k <= 30, F <= 6) or analog_slab_predict_kernel
//   Bf2       analog_bf2_predict_kernel: the heap scanner over the whole set
//   Bf        analog_bf_predict_kernel: lists in global scratch (k beyond the LDS heaps)
// Fit: F == 1 on a series the workgroup sort serves -> sorted view (tile sort of width K with presorted runs, or the transposes;
// index-tag pass + exact pass, or exact only); F > 1 -> feature-0 sorted copy for the slab search.  Prefix sums are never built
// at fit time: the kernels that read them from memory get them on their first call (need_pq / need_rx).
// Fit + predict: the fused per-cell kernel (K, np, LDS), or fit -> predict (each planned as its own call).
//
// What depends on data stays in the launchers:
//   * the number of cells or batches a kernel hands back (work_count of analog_sort2_kernel, analog_slab_topk_kernel,
//     analog_f1_fused_kernel) and so the grids of the launches that serve them (exact sort: fixed grid over the list; heap
//     kernel and gather / scatter: sized from the count);
//   * the input of analog_handback_whole_grid (the fused kernel's count);
//   * the fall-back when the buffer of presorted runs cannot be allocated: the launcher plans the fit again with no_tile set.
// The NULL-argument checks stay at the entry points, which read the state to build the call.
//
// Limits that a tighter one shadows at the 160 KB of the MI355X, kept as written: T <= 65535 (sorted view, 16-bit heap indices)
// and T <= 20 * 1024 (Mean3) sit behind sort2_width's 19 456; "mean_analogs with k > 1 and prefix sums" is Mean3 for every T a
// sorted view exists for.  A sorted view needs a sort2_width: the single-sort kernel that served series without one is gone --
// with 10 * T <= lds_max and 8 * (T + 1) <= lds_max no T lacks a width once lds_max >= 21 KB (tests/test_analog_plan.py sweeps
// T = 1 .. 20 480 at 21 KB, 64 KB and 160 KB).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"
#include "sd_wave_consts.h"

// ---- sizing constants and functions of the analog kernels (one definition each; the kernels use the same names) ------------
namespace sdan {

constexpr int kMaxF = 8;                 // = sdlsq::kMaxF (static_assert in sd_analog.hip)
constexpr long long kTagMask = 0x3fff;   // 14 bits: series of up to 16 384 samples
constexpr int kRunK = 16;                // keys per lane of the run sort
constexpr int kRun = 64 * kRunK;         // queries per run: 1 024 consecutive time steps
constexpr int kRunRS = kRun + 2;         // LDS row stride in doubles (RS % 4 == 2: rows land 8 or 24 banks apart, like sd_bcsd_rs_row_stride)
constexpr int kRunRSQ = kRun + 32 + 2;   // the same for rows that hold sorted position p at slot p + p / 32 (see analog_query_runs_kernel)
constexpr int kRunsMinTq = 2 * kRun;     // value-ordered runs pay from a few runs on
constexpr int kRegDirectK = 64;          // AnalogRegression windows up to this long are summed directly (reg_batch); longer ones take the prefix sums
constexpr int kPhQ = 16;                 // queries per thread and LDS generation (1024 threads: series up to 16 384 queries per pass)
constexpr int kMean3MaxT = 1024 * 20;    // analog_f1_mean3_kernel<20>: 20 training values per thread
constexpr int kQsplitMinTq = 4096;       // fewer queries: one workgroup per cell
constexpr int kTopKeep = 32, kTopNew = 32;
constexpr int kTopMaxF = 6;              // (7 and 8 features do not fit 256 registers with the matrix-core tiles: the heap kernel)
constexpr int kTopMaxK = 30;             // two spare kept slots tell "every tie of the k-th bucket is here" from "maybe not"
constexpr int kBfThreads = 256;
constexpr int kBfChunk = 1024;
constexpr int64_t kChunkCells = 16384;   // cells per chunk of the staged F == 1 paths
constexpr int64_t kSlabChunkCells = 4096;  // slab search: halved until cells x query batches fit one grid
constexpr int64_t kGridLimit = (int64_t)1 << 31;

// widths instantiated for the fast sort: T <= 1024 * K and the keys must fit the LDS; 0: none
inline int sort2_width(int64_t T, size_t lds_max) {
    const int widths[] = {5, 9, 13, 15, 17, 19};
    for (int K : widths) {
        const int64_t np = (T + K - 1) / K * K;
        if (T <= (int64_t)1024 * K && T <= 65535 && sdw::block_sort_lds_bytes((int)np) <= lds_max) return K;
    }
    return 0;
}
// padded length of analog_sort2_kernel<K> (presorted runs of the tile sort may be padded further) and its LDS
inline int sort2_np(int K, int64_t T, int np_runs) {
    const int np = (int)((T + K - 1) / K * K);
    return np_runs > np ? np_runs : np;
}
inline size_t sort2_lds_bytes(int np) { return sdw::block_sort_lds_bytes(np); }

// analog_tile_sort_kernel<K>: row stride, LDS, slots of presorted runs per cell; workgroups of the kernels tiled like the BCSD
// ones (shared with the quantile-mapping fit: sd_wave_consts.h)
using sdw::tile_sort_rs;
using sdw::tile_sort_lds_bytes;
using sdw::tile_sort_chunks;
using sdw::tile_sort_np;
using sdw::tiled_blocks;
// The tile-shaped first stage of the F == 1 fit: instantiated for the widths of the 40-year daily series and its neighbours.
inline bool tile_sort_applies(int K, int64_t T, int64_t C, size_t lds_max, bool no_tile) {
    if (K != 13 && K != 15 && K != 17) return false;
    const int64_t nchunks = tile_sort_chunks(K, T);
    if (T > kTagMask + 1 || C >= kGridLimit || nchunks > 16) return false;
    if (sort2_lds_bytes(tile_sort_np(K, T)) > lds_max) return false;
    return !no_tile;
}
inline size_t query_runs_lds_bytes() { return sizeof(double) * ((size_t)sdw::kW * kRunRSQ + sdw::kHeadDoubles); }
inline size_t untranspose_runs_lds_bytes() { return sizeof(double) * ((size_t)sdw::kW * kRunRS + sdw::kHeadDoubles); }

// heap [k][64] of (double, IT) + the chunk staging area [F][64] doubles + [64] indices (16-byte aligned pieces)
inline size_t bf2_lds_bytes(int k, int F, size_t it_bytes) {
    const size_t heap = ((size_t)k * 64 * (sizeof(double) + it_bytes) + 15) / 16 * 16;
    return heap + (size_t)F * 64 * sizeof(double) + 64 * sizeof(int32_t);
}
inline size_t topk_lds_bytes(int F) {
    const size_t scan = sizeof(unsigned) * kTopNew * 64 + sizeof(uint16_t) * (kTopKeep + kTopNew) * 64 + sizeof(double) * (size_t)F * 64;
    const size_t fin = (sizeof(double) + sizeof(uint16_t)) * (size_t)kTopKeep * 64;
    return scan > fin ? scan : fin;
}
// LDS of analog_f1_fused_kernel: keys (np + 1 doubles), co-ranks (1025 ints, padded), tags (T x 16 bit); + its static arrays
inline size_t fused_lds_bytes(int np, int64_t T) {
    return sizeof(double) * (size_t)(np + 1) + sizeof(int) * 1026 + ((sizeof(uint16_t) * (size_t)T + 15) & ~(size_t)15);
}
// analog_f1_window_kernel: fewest value ranges such that xs and yx of a range (+ k entries of margin each side) fit the LDS
inline int window_npass(int64_t T, int k, size_t lds_max, size_t* lds) {
    int npass = 1;
    for (;; ++npass) {
        const size_t cap = (size_t)((T + npass - 1) / npass) + 2 * (size_t)k + 1;
        *lds = sizeof(double) * (2 * cap + 1);
        if (*lds <= lds_max || npass >= 64) break;
    }
    return npass;
}
// persistent grids: multiples of 8 workgroups (one range of cells per XCD), no more than the cells rounded up to 8
inline int persistent_blocks(int want, int64_t C) {
    int nb = (want / 8) * 8;
    if (nb < 8) nb = 8;
    const int64_t c8 = ((C + 7) / 8) * 8;
    return (int64_t)nb > c8 ? (int)c8 : nb;
}

}  // namespace sdan

// ---- the plan --------------------------------------------------------------------------------------------------------------
enum class AnalogOp { Fit, Predict, RegPredict, FitPredict };  // Predict / RegPredict: PureAnalog / AnalogRegression from a fitted state

// Switches of the development library (environment variables, read in one place: sd_analog_dev_switches() of sd_internal.h);
// the production library keeps the defaults.
struct AnalogDevSwitches {
    bool no_slab = false;      // SD_ANALOG_NOSLAB: no feature-0 sorted copy, no slab search
    bool heap = false;         // SD_ANALOG_HEAP: the heap kernel for every slab call
    bool no_tile = false;      // SD_ANALOG_NOTILE: the transposes instead of the tile sort (and no fused kernel)
    bool reg_prefix = false;   // SD_ANALOG_REG_PREFIX: prefix differences for every AnalogRegression window
    bool no_runs = false;      // SD_ANALOG_NORUNS: plain staging transposes
    bool runs_always = false;  // SD_ANALOG_RUNS_ALWAYS: value-ordered runs for the Mean3 and fused kernels too
    int slab_classes = -1;     // SD_ANALOG_SLAB_CLASSES: classes of the slab search's query order (-1: by Tq)
    // diagnostics that are runtime arguments of kernels or host printouts
    int ablate = 0;            // SD_ANALOG_ABLATE: timing experiments (results are wrong): 1 no insertions, 2 no epilogue, 4 counts
    int prune_at = -1;         // SD_TOPK_PRUNE_AT (-1: 16)
    bool readlane = false;     // SD_TOPK_READLANE: the v_readlane form of the top-k pre-filter
    bool m3_trace = false;     // SD_M3_TRACE: phase clocks of analog_f1_mean3_kernel
    bool fused_trace = false;  // SD_FUSED_TRACE: phase clocks of analog_f1_fused_kernel
    bool count = false;        // SD_ANALOG_COUNT: print how many cells the fast kernels handed back
};

struct AnalogCall {
    AnalogOp op = AnalogOp::Fit;
    int64_t T = 0, C = 0, Tq = 0;
    int F = 0, k = 0, kind = SD_ANALOG_MEAN;
    bool has_thresh = false;
    bool neighbors = false;    // neighbour indices or distances asked for
    bool has_sample = false;   // sample indices passed
    int64_t ld = 0, ld_q = 0, ld_out = 0;  // leading dimensions of X and y, Xq, out
    size_t lds_max = 0;
    int cu_count = 0;
    // predict: the fitted state
    bool has_xs = false, has_yx = false, has_ybar = false, has_ps = false;  // sorted view (F == 1), feature-0 sorted copy (F > 1)
    bool has_pq = false, has_rx = false;                                    // prefix sums already built
};

enum class AnalogPath { None, Mean3, Mean, Window, Walk, Slab, Bf2, Bf, Fused, Split };

struct AnalogLaunch {
    int64_t gx, gy, gz;
    int block;
    size_t lds;  // dynamic LDS bytes
};

struct AnalogPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    // fit
    bool sorted = false;       // F == 1: sorted view xs / xi / yx / ybar
    int K = 0;                 // width of the sorted view's sort (fit), of the fused kernel (fit + predict)
    bool tiled = false;        // analog_tile_sort_kernel<K> makes the cell-major copies and presorted runs (np_runs slots per cell)
    int np_runs = 0;
    bool tagged = false;       // index-tag pass before the exact pass
    int Ks = 0;                // F > 1: width of the feature-0 sort (0: no slab copy)
    // predict
    AnalogPath path = AnalogPath::None;
    int kind = SD_ANALOG_MEAN;  // k == 1 is 'best_analog' whatever the configured kind (gard.py:291-296)
    int nb = 0, nthr = 0;       // persistent grid and block of the per-cell kernels; scratch lists are [nb][k][nthr]
    int per = 0;                // Mean3: PER
    int qsplit = 1;             // Mean: workgroups per cell where the chunk's grid allows it (analog_qsplit)
    bool reg_direct = false;
    int npass = 0;              // Window
    bool runs_q = false;        // queries staged as value-ordered runs
    int skip_prob = 0;          // the staging transpose derives the probability plane from the predictions
    bool need_pq = false, need_rx = false;  // build the prefix sums / the regression's cross term first
    size_t lds = 0;             // dynamic LDS of the path's main kernel
    int64_t chunk = 0;          // cells per chunk (0: the whole grid in one launch)
    int it_bytes = 0;           // Bf2: 2 (16-bit heap indices, T <= 65535) or 4
    // slab
    bool topk = false;
    int nclass = 0, Kq = 0;
    int prune_at = 16, use_mfma = 1, ablate = 0;
};

// fused fit + predict: more than half of the cells handed back -> the whole grid through the split path
inline bool analog_handback_whole_grid(int64_t handed_back, int64_t C) { return handed_back * 2 > C; }

namespace analog_plan_detail {
using namespace sdan;

template <class... A>
bool fail(AnalogPlan* pl, int code, const char* fmt, A... a) {
    snprintf(pl->message, sizeof pl->message, fmt, a...);
    pl->error = code;
    return false;
}
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

inline bool plan_fit(const AnalogCall& c, const AnalogDevSwitches& d, AnalogPlan* pl) {
    if (!(c.T > 0 && c.C > 0 && c.ld >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_analog_fit: bad sizes");
    if (!(c.F >= 1 && c.F <= kMaxF)) return fail(pl, SD_ERR_INVALID, "sd_analog_fit: F=%d outside [1,%d]", c.F, kMaxF);
    const int K2 = sort2_width(c.T, c.lds_max);
    pl->sorted = c.F == 1 && c.T <= 65535 && K2 != 0 && sizeof(double) * (size_t)(c.T + 1) <= c.lds_max;
    if (pl->sorted) {
        pl->K = K2;
        pl->tiled = tile_sort_applies(K2, c.T, c.C, c.lds_max, d.no_tile);
        if (pl->tiled) {
            pl->np_runs = tile_sort_np(K2, c.T);
            if (tiled_blocks(c.C, tile_sort_chunks(K2, c.T)) >= kGridLimit) return fail(pl, SD_ERR_INVALID, "%s", "analog fit: grid too large");
        }
    }
    pl->Ks = c.F > 1 && !d.no_slab ? K2 : 0;
    // index-tag pass first (series of up to 16 384 samples), then the cells it handed back
    pl->tagged = (pl->sorted || pl->Ks != 0) && c.T <= kTagMask + 1 && c.C < kGridLimit;
    return true;
}

inline bool plan_predict(const AnalogCall& c, const AnalogDevSwitches& d, AnalogPlan* pl) {
    const int mode = c.op == AnalogOp::RegPredict ? 1 : 0;
    const int k = c.k;
    if (!(c.Tq > 0 && c.ld_q >= c.C && c.ld_out >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_analog_predict: bad sizes");
    if (!(k >= 1 && k <= c.T)) return fail(pl, SD_ERR_INVALID, "sd_analog_predict: k=%d must be in [1, T=%lld]", k, (long long)c.T);
    if (!(mode == 1 || (c.kind >= SD_ANALOG_BEST && c.kind <= SD_ANALOG_MEAN))) return fail(pl, SD_ERR_INVALID, "sd_analog_predict: unknown kind %d", c.kind);
    if (mode == 0 && c.kind == SD_ANALOG_SAMPLE && !c.has_sample) return fail(pl, SD_ERR_INVALID, "%s", "sd_analog_predict: sample_analogs needs sample_inds");
    // PureAnalog.predict with a single analog is 'best_analog' whatever the configured kind (gard.py:291-296: n_analogs == 1);
    // the entry point sees k only, so a one-sample training set (k_ = 1 with n_analogs > 1) is treated the same way
    const int kind = pl->kind = mode == 0 && k == 1 ? SD_ANALOG_BEST : c.kind;
    const int64_t T = c.T, Tq = c.Tq;
    const int F = c.F;
    const bool f1 = c.has_xs;
    pl->nthr = f1 ? 1024 : kBfThreads;
    pl->nb = persistent_blocks(c.cu_count * (f1 ? 1 : 4), c.C);
    pl->prune_at = d.prune_at < 0 ? 16 : d.prune_at < 1 ? 1 : d.prune_at > kTopNew ? kTopNew : d.prune_at;
    pl->use_mfma = d.readlane ? 0 : 1;
    pl->ablate = d.ablate;
    // (a thresholded regression needs the analogs themselves: logistic fit and subset OLS, gard.py:201-219)
    const bool window = f1 && (mode == 1 || kind != SD_ANALOG_SAMPLE) && !c.neighbors && c.has_yx && !(mode == 1 && c.has_thresh);
    if (window) {
        size_t lds_win = 0;
        pl->npass = window_npass(T, k, c.lds_max, &lds_win);
        if (lds_win > c.lds_max) return fail(pl, SD_ERR_INVALID, "sd_analog_predict: k=%d too large for the windowed path", k);
        // queries and outputs go through cell-major copies: the column accesses of a cell would be 8-byte requests 8*ld bytes
        // apart (one 64-byte sector each); the tiled transposes stream at HBM speed.  Cells are processed in chunks so that the
        // staging buffers stay small (and cache-resident).
        pl->chunk = kChunkCells;
        // single pass with only xs in LDS (statistics from the prefix sums, or the window of yx read from memory)
        const size_t lds_mean = sizeof(double) * (size_t)(T + 1);
        const bool mean_only = (mode == 1 ? k >= 3 : (kind == SD_ANALOG_MEAN || kind == SD_ANALOG_WEIGHT || k == 1)) && c.has_ybar &&
                               lds_mean <= c.lds_max;
        const bool phases = mean_only && mode == 0 && ((kind == SD_ANALOG_MEAN && !c.has_thresh) || k == 1) && T <= kMean3MaxT;
        // without a threshold the probability column is 1 wherever the prediction is not NaN (gard.py:346; AnalogRegression:
        // gard.py:211-212): the single-pass kernels do not write it either, the staging transpose derives it from the predictions
        pl->skip_prob = mean_only && !c.has_thresh ? 1 : 0;
        // Value-ordered runs pay where a query reads its window of analog values from memory (weights, thresholds, the regression):
        // neighbouring lanes then read overlapping lines.  The three-generation kernel reads nothing per query but LDS words, and
        // its search is bound by its spilled registers, not by bank conflicts: measured equal with sorted queries (33.7 against
        // 33.0 ms per 100 000 cells), while the run staging costs 6 ms more than the plain transposes -- it keeps the time order.
        pl->runs_q = Tq >= kRunsMinTq && !d.no_runs && !(phases && !d.runs_always);
        if (pl->runs_q && tiled_blocks(min64(c.C, pl->chunk), (Tq + kRun - 1) / kRun) >= kGridLimit)
            return fail(pl, SD_ERR_INVALID, "%s", "analog predict: grid too large");
        // AnalogRegression with a short window sums it directly (reg_batch: no prefix arrays to build or to read); the default
        // n_analogs = 200 keeps the prefix differences (two 16-byte loads instead of 200 values per query)
        pl->reg_direct = mean_only && mode == 1 && k <= kRegDirectK && !d.reg_prefix;
        // (the prefix sums serve the regression and the plain mean; weights and thresholds read the analog values themselves)
        pl->need_pq = mean_only && !phases && !pl->reg_direct && (mode == 1 || (kind == SD_ANALOG_MEAN && !c.has_thresh && k > 1)) && !c.has_pq;
        pl->need_rx = mean_only && mode == 1 && !pl->reg_direct && !c.has_rx;
        // workgroups per cell in the single-pass kernel, measured (ms per 16 384 cells) 1/2/4/8: regression 10.8/8.5/8.7/11.0, mean 5.5/5.7/6.4/8.3
        pl->qsplit = mode == 1 && !pl->reg_direct ? 2 : 1;
        if (phases) {
            const int per = (int)((T + 1023) / 1024);
            pl->path = AnalogPath::Mean3;
            pl->per = per <= 8 ? 8 : per <= 16 ? 16 : 20;
            pl->lds = lds_mean;
        } else if (mean_only) {
            pl->path = AnalogPath::Mean;
            pl->lds = lds_mean;
        } else {
            pl->path = AnalogPath::Window;
            pl->lds = lds_win;
        }
    } else if (f1) {
        pl->path = AnalogPath::Walk;
        pl->lds = sizeof(double) * (size_t)T;
    } else if (F > 1 && c.has_ps && bf2_lds_bytes(k, F, 2) <= c.lds_max && sort2_width(Tq, c.lds_max) != 0 && !d.no_slab) {
        // queries go cell-major, are sorted by feature 0 per cell, and every wave scans only the slab of training points its 64
        // neighbouring queries can reach
        const int64_t nbatch = (Tq + 63) / 64;
        pl->path = AnalogPath::Slab;
        pl->chunk = kSlabChunkCells;
        while (pl->chunk > 1 && pl->chunk * nbatch >= kGridLimit) pl->chunk >>= 1;
        pl->Kq = sort2_width(Tq, c.lds_max);
        pl->tagged = Tq <= kTagMask + 1;
        // classes of the query order (analog_slab_s2_kernel); a short series would only get waves that straddle classes
        const int nclass = d.slab_classes >= 0 ? d.slab_classes : (int)min64(8, Tq / 512);
        pl->nclass = nclass < 1 ? 1 : (nclass > 8 ? 8 : nclass);
        // k <= 30: candidate lists pruned by a register sorting network (analog_slab_topk_kernel); the heap kernel takes larger k
        // and the batches the fast kernel hands back
        pl->topk = k <= kTopMaxK && F <= kTopMaxF && !d.heap;
        pl->lds = pl->topk ? topk_lds_bytes(F) : bf2_lds_bytes(k, F, 2);
    } else if (bf2_lds_bytes(k, F, 4) <= c.lds_max) {
        pl->path = AnalogPath::Bf2;
        pl->it_bytes = T <= 65535 ? 2 : 4;
        pl->lds = bf2_lds_bytes(k, F, (size_t)pl->it_bytes);
        if (c.C * ((Tq + 63) / 64) >= kGridLimit) return fail(pl, SD_ERR_INVALID, "%s", "sd_analog_predict: too many (cell, query batch) pairs for one launch");
    } else {
        pl->path = AnalogPath::Bf;
        pl->lds = sizeof(double) * (size_t)F * kBfChunk;
    }
    return true;
}

inline bool plan_fit_predict(const AnalogCall& c, const AnalogDevSwitches& d, AnalogPlan* pl) {
    if (!(c.T > 0 && c.C > 0 && c.Tq > 0 && c.ld >= c.C && c.ld_q >= c.C && c.ld_out >= c.C)) return fail(pl, SD_ERR_INVALID, "%s", "sd_analog_fit_predict: bad sizes");
    if (!(c.F >= 1 && c.F <= kMaxF)) return fail(pl, SD_ERR_INVALID, "sd_analog_fit_predict: F=%d outside [1,%d]", c.F, kMaxF);
    if (!(c.k >= 1 && c.k <= c.T)) return fail(pl, SD_ERR_INVALID, "sd_analog_fit_predict: k=%d must be in [1, T=%lld]", c.k, (long long)c.T);
    if (!(c.kind >= SD_ANALOG_BEST && c.kind <= SD_ANALOG_MEAN && c.kind != SD_ANALOG_SAMPLE))
        return fail(pl, SD_ERR_INVALID, "sd_analog_fit_predict: kind %d (sample_analogs needs the split calls)", c.kind);
    pl->kind = c.k == 1 ? SD_ANALOG_BEST : c.kind;
    const int K = c.F == 1 ? sort2_width(c.T, c.lds_max) : 0;
    const int np = K != 0 ? tile_sort_np(K, c.T) : 0;
    const bool fused = K != 0 && tile_sort_applies(K, c.T, c.C, c.lds_max, d.no_tile) && ((pl->kind == SD_ANALOG_MEAN && !c.has_thresh) || c.k == 1) &&
                       c.Tq <= (int64_t)kPhQ * 1024 && fused_lds_bytes(np, c.T) + 512 <= c.lds_max;
    pl->path = fused ? AnalogPath::Fused : AnalogPath::Split;
    if (!fused) return true;  // fit -> PureAnalog predict -> drop the state: each planned as its own call
    if (tiled_blocks(c.C, tile_sort_chunks(K, c.T)) >= kGridLimit) return fail(pl, SD_ERR_INVALID, "%s", "analog fit: grid too large");
    pl->K = K;
    pl->tiled = true;
    pl->np_runs = np;
    pl->lds = fused_lds_bytes(np, c.T);
    pl->nthr = 1024;
    pl->nb = persistent_blocks(c.cu_count, c.C);
    pl->chunk = kChunkCells;
    pl->skip_prob = !c.has_thresh ? 1 : 0;
    // (the fused kernel gains nothing from value-ordered queries -- see plan_predict -- : development switch only)
    // (at most kPhQ runs of queries here: the staging grids of a chunk cannot reach the grid limit)
    pl->runs_q = c.Tq >= kRunsMinTq && !d.no_runs && d.runs_always;
    return true;
}

}  // namespace analog_plan_detail

inline AnalogPlan analog_plan(const AnalogCall& c, const AnalogDevSwitches& d) {
    AnalogPlan pl;
    switch (c.op) {
        case AnalogOp::Fit: analog_plan_detail::plan_fit(c, d, &pl); break;
        case AnalogOp::Predict:
        case AnalogOp::RegPredict: analog_plan_detail::plan_predict(c, d, &pl); break;
        case AnalogOp::FitPredict: analog_plan_detail::plan_fit_predict(c, d, &pl); break;
    }
    return pl;
}

// ---- geometry of the launches: one function per launch, used by the launchers for grid, block and LDS; the order of the launches and
// their profiler names are the launchers' -----------------------------------------------------------------------------------------
namespace analog_launches {
using namespace sdan;
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

inline AnalogLaunch transpose(int64_t C, int64_t T) { return {(C + 31) / 32, (T + 31) / 32, 1, 256, 0}; }
inline AnalogLaunch tile_sort(int K, int64_t T, int64_t C) {
    return {tiled_blocks(C, tile_sort_chunks(K, T)), 1, 1, sdw::kThreads, tile_sort_lds_bytes(K)};
}
// analog_sort2_kernel<K>: the index-tag pass (tagged), and the exact pass over every cell or over the list the first hands back
inline AnalogLaunch sort2(int K, int64_t T, int64_t C, int np_runs, int cu_count, bool tagged, bool exact) {
    const int64_t nb = min64(C, (int64_t)cu_count * 4);
    const size_t lds = sort2_lds_bytes(sort2_np(K, T, np_runs));
    if (!exact) return {nb, 1, 1, 1024, lds};
    return {tagged ? min64(nb, 256) : nb, 1, 1, 1024, lds};
}
inline AnalogLaunch gather_sorted(int64_t C, int cu_count) { return {min64(C, (int64_t)cu_count * 64), 1, 1, 256, 0}; }
// prefix sums through LDS where the series fits, else read in place (both under one profiler name)
inline AnalogLaunch prefix_sums(int64_t T, int64_t C, int cu_count, size_t lds_max) {
    const size_t lds = sizeof(double) * (size_t)(T + 1);
    return {min64(C, (int64_t)cu_count * 2), 1, 1, 1024, lds + 512 <= lds_max ? lds : 0};
}
inline AnalogLaunch rx(int64_t T, int64_t C, int cu_count) { return {min64(C, (int64_t)cu_count * 2), 1, 1, 1024, sizeof(double) * (size_t)(T + 1)}; }
inline AnalogLaunch status_public(int64_t C) { return {(C + 255) / 256, 1, 1, 256, 0}; }
// query staging of a chunk of cc cells, in and out: value-ordered runs or plain transposes
inline AnalogLaunch stage_in(const AnalogPlan& pl, int64_t Tq, int64_t cc) {
    if (pl.runs_q) return {tiled_blocks(cc, (Tq + kRun - 1) / kRun), 1, 1, sdw::kThreads, query_runs_lds_bytes()};
    return transpose(cc, Tq);
}
inline AnalogLaunch stage_out(const AnalogPlan& pl, int64_t Tq, int64_t cc) {
    const int planes = pl.skip_prob ? 2 : 3;
    if (pl.runs_q) return {tiled_blocks(cc, (Tq + kRun - 1) / kRun), planes, 1, sdw::kThreads, untranspose_runs_lds_bytes()};
    return {(cc + 31) / 32, (Tq + 31) / 32, planes, 256, 0};
}
// workgroups per cell of analog_f1_mean_kernel in a chunk of cc cells on nbc workgroups: only when every XCD still gets whole groups
inline int qsplit(const AnalogPlan& pl, int nbc, int64_t cc, int64_t Tq) {
    const int qs = pl.qsplit;
    return qs < 1 || nbc % (8 * qs) != 0 || cc < (int64_t)nbc || Tq < kQsplitMinTq ? 1 : qs;
}
// the persistent per-cell kernel of a chunk (Mean3 / Mean / Window / Fused), or of the whole grid (Walk / Bf)
inline AnalogLaunch per_cell(const AnalogPlan& pl, int64_t cc) {
    return {persistent_blocks(pl.nb, cc), 1, 1, pl.nthr, pl.lds};
}
inline AnalogLaunch bf2(const AnalogPlan& pl, int64_t C, int64_t Tq) { return {C * ((Tq + 63) / 64), 1, 1, 64, pl.lds}; }
// slab search over a chunk of cc cells
// (analog_slab_s2_kernel, analog_slab_key_kernel, analog_slab_center_kernel: cells strided over a fixed grid)
inline AnalogLaunch slab_aux(int64_t cc, int cu_count) { return {min64(cc, (int64_t)cu_count * 8), 1, 1, 256, 0}; }
inline AnalogLaunch slab_topk(const AnalogPlan& pl, int64_t cc, int64_t Tq) { return {cc * ((Tq + 63) / 64), 1, 1, 64, pl.lds}; }
// the heap kernel over every (cell, query batch) of the chunk, or over the nwork pairs the top-k kernel handed back
inline AnalogLaunch slab_heap(int k, int F, int64_t cc, int64_t Tq, int64_t nwork) {
    return {nwork > 0 ? nwork : cc * ((Tq + 63) / 64), 1, 1, 64, bf2_lds_bytes(k, F, sizeof(uint16_t))};
}

}  // namespace analog_launches
