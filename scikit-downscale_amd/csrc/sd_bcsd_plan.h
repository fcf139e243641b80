// Launch plan of a BCSD call: which kernels run, in which order, over which groups, with which widths, grids and LDS sizes.
// The decision is integer arithmetic on the call's group lengths, pitches, pointer alignment and the LDS size, written once
// here as a pure host function (no HIP header: tests/bcsd_plan_check.cpp compiles it with g++ alone).  The launchers of
// sd_bcsd.hip, sd_bcsd_rs.hip and sd_bcsd_fx.hip map each record to the launch it names.
//
// Paths, fastest first:
//   fused     sd_bcsd_fx.hip: x side, y side, inverse CDF and shift / ratio of a segment in one workgroup pass (segments of up
//             to 1 536 samples, fit + predict or predict from a state, not detrended); the segments it hands back (work list)
//             take RANK + APPLY.  Within it: the LDS-DMA kernel (BcsdTemperature fit + predict on aligned fields), the
//             register-tile kernels (whole-lane FULL groups and the rest), the compacting precipitation kernel.
//   register  sd_bcsd_rs.hip: RANK + APPLY (predict), FIT (fit that keeps a state); segments of up to 2 112 samples.
//   long      bcsd_long_*_kernel (sd_bcsd.hip): one 1024-thread workgroup per (cell, group), 2 113 .. 19 456 samples.
//   generic   bcsd_fit_kernel / bcsd_predict_kernel (sd_bcsd.hip): LDS-bitonic, any segment the LDS holds; also every pitch
//             of 2^29 elements or more (the faster kernels address rows with a 32-bit byte pitch).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sd_downscale.h"
#include "sd_wave_consts.h"

// ---- sizing of the fused kernels (sd_bcsd_fx.hip) -----------------------------------------------------------------------
namespace sdfx {

constexpr int kFront = 4;

// sort keys of the fused kernels: (q << kTagBits) | tag, q the quantised value, tag the sample's position in its row or tile
constexpr unsigned kTagBits = 11, kTagMask = 2047u;
constexpr unsigned kQD = (1u << 21) - 2048u;  // data keys use q <= kQD; pads q = kQD + 1 + slot

constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }

// LDS row layout of the register-tile kernels: sample j of the segment sits in slot 4 + j + j / (K * P), P = 64 / gcd(2K, 64)
template <int K>
struct Lay {
    static constexpr int P = 64 / cgcd(2 * K, 64);
    static constexpr int KP = K * P;
    static constexpr int slot(int j) { return kFront + j + j / KP; }             // j >= 0
    static constexpr int own(int lane) { return kFront + K * lane + lane / P; }  // slot of sample K * lane
};

// slots a row needs: a partly filled lane reads its whole block and the rolling window behind it, so the row reaches
// sample K * ceil(len / K) + 3 of the longest group; one spare slot takes the stores of positions past the segment
template <int K>
int row_slots(int nmax) {
    int need = Lay<K>::slot((nmax + K - 1) / K * K + 3) + 2;
    while (need % 4 != 2) ++need;  // cell rows land 8 or 24 banks apart: conflict-free transposing stores
    return need;
}

// samples per lane (K) of the fused kernels serving segments of up to nmax samples; 0: none does
constexpr int fx_width(int nmax) {
    return nmax < 1 ? 0 : nmax <= 64 * 4 ? 4 : nmax <= 64 * 8 ? 8 : nmax <= 64 * 12 ? 12 : nmax <= 64 * 16 ? 16
         : nmax <= 64 * 20 ? 20 : nmax <= 64 * 24 ? 24 : 0;
}

inline int row_slots(int K, int nmax) {
    switch (K) {
        case 4: return row_slots<4>(nmax);
        case 8: return row_slots<8>(nmax);
        case 12: return row_slots<12>(nmax);
        case 16: return row_slots<16>(nmax);
        case 20: return row_slots<20>(nmax);
        default: return row_slots<24>(nmax);
    }
}

// FULL instantiations serve groups whose segments are whole lanes of K samples and at least this long: every thread's first
// K / 2 - 1 rows of a tile exist, only the last pass is predicated
constexpr int full_min_len(int K) { return sdw::kRowsPerPass * (K / 2 - 1) + 1; }

// width of the compacting precipitation kernel's sort of the wet days (0: no compacting kernel at this K)
constexpr int compact_width(int K) { return K == 20 ? 12 : K == 24 ? 16 : 0; }

namespace tmj {  // tile of the LDS-DMA kernel: chunks of 16 row fragments, one lane of 20 rows per chunk plus the tail chunks
constexpr int kChunkStride = 1024 + 8;
constexpr int kBlock = 20;  // rows per lane (the kernel's K)
constexpr int lanes_of(int n) { return (n + kBlock - 1) / kBlock; }
constexpr int chunks_of(int n) { return lanes_of(n) + 16; }  // n: more than 32 lanes of 20
// Lane l works on rows 20 l .. 20 l + 19: chunk l holds the first 16 of them (slot i = row 20 l + i), its tail of four sits in chunk
// nl + tail_chunk(l) at the slots tail_slot(l) + 4 e (nl = lanes_of(n); the layout and its bank arithmetic: sd_bcsd_fx.hip)
constexpr int tail_chunk(int l) { return (l & 7) + 8 * (l >> 5); }
constexpr int tail_slot(int l) { return (l >> 3) & 3; }
// row of the segment that slot S of chunk Q holds (n - 1 where the slot holds none, chunks past the tile included)
__attribute__((always_inline)) constexpr int row_of_slot(int Q, int S, int nl, int n) {
    int r = 0;
    if (Q < nl) {
        r = kBlock * Q + S;
    } else {
        const int t = Q - nl;
        const int l = (t & 7) + 8 * (S & 3) + 32 * (t >> 3);
        r = l < nl ? kBlock * l + 16 + (S >> 2) : n - 1;
    }
    return r < n ? r : n - 1;
}

// ---- integer formulas of the kernel's keys and tag addresses, as the kernel evaluates them (`_ref`: the forms they replaced,
// kept for tests/fd_keys_check.cpp, which runs both) -----------------------------------------------------------------------------
// v_alignbit_b32 / v_bfe_u32 / v_bfi_b32
constexpr uint32_t alignbit(uint32_t hi, uint32_t lo, unsigned s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> s); }
constexpr uint32_t bfe(uint32_t v, unsigned off, unsigned width) { return (v >> off) & ((1u << width) - 1u); }
constexpr uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return (mask & a) | (~mask & b); }
// key of a sample of the shifted series from the two words (w1: high) of t + 2^21, t = the quantised value in [1, kQD - 1]: the
// mantissa is t in units of 2^-31, q = its bits 51 .. 31, clamped to kQD (NaN: 2^20), above the tag.
constexpr uint32_t key_u2_ref(uint32_t w0, uint32_t w1, uint32_t tag) {
    uint32_t q = alignbit(w1, w0, 31) & 0x1fffffu;
    q = q < kQD ? q : kQD;
    return (q << kTagBits) | tag;
}
// The same in four instructions: alignbit by 20 leaves q in bits 31 .. 11 (the exponent falls off the top) over 11 fraction bits;
// clamped with the fraction bits all ones, the q field is min(q, kQD); the tag (< 2^11) then replaces the fraction bits.
constexpr uint32_t key_u2(uint32_t w0, uint32_t w1, uint32_t tag) {
    const uint32_t a = alignbit(w1, w0, 32 - 1 - kTagBits), top = (kQD << kTagBits) | kTagMask;
    return bfi(kTagMask, tag, a < top ? a : top);
}
// pad key i of lane `lane` (a lane past the data): q = kQD + 1 + K lane + i above the tag K lane + i
constexpr uint32_t pad_key(int lane, int i) {
    const uint32_t tag0 = (uint32_t)(kBlock * lane);
    return (((kQD + 1u + tag0) << kTagBits) | tag0) + (uint32_t)i * ((1u << kTagBits) + 1u);
}
// byte offset (cell 0) of position `tag` = 16 chunk + slot of the tile: chunk * kChunkStride + 64 slot
constexpr uint32_t tag_off_ref(uint32_t tag) { return (tag << 6) + ((tag >> 4) << 3); }
// The same straight from a key (no `& kTagMask` first): the chunk is a bit field of the key, the slot a masked shift.
constexpr uint32_t key_off(uint32_t key) { return bfe(key, 4, kTagBits - 4) * (uint32_t)kChunkStride + ((key << 6) & 0x3c0u); }

// Request row tables of one group: the time index behind every (chunk, slot) of the tile is a function of the group's order table
// alone -- the same for every tile, step and call on that calendar --, so it is tabulated once per cached group table
// (sd_bcsd.hip: upload_group_table) instead of derived by every (tile, month) item:
//   P[16 Q + S]         = ord[row_of_slot(Q, S, nl, n)], Q = 0 .. kTabChunks - 1: every chunk three row registers of a wave name
//                         (8 waves x 12 requests); the late y requests of column `col` read P at 16 * 5 col + 64 j + lane
//   W[wave][j][lane]    = P[16 (wave + 8 (4 j + lane / 16)) + lane % 16]: the chunks wave + 8 k dealt round the waves, in the order
//                         a wave's registers hold them (register j, lane) -- one contiguous 256-byte line per register
// One group's table is [P | W]; a table set holds one per group of the order table (groups no LDS-DMA launch serves stay zero).
constexpr int kTabChunks = 96;
constexpr int kTabP = 16 * kTabChunks;               // entries of P
constexpr int kTabWave = 3 * 64;                     // entries of W per wave
constexpr int kTabW = sdw::kW * kTabWave;            // entries of W
constexpr int kTabInts = kTabP + kTabW;              // 3 072 entries, 12 KB per group
static_assert(sdw::kW - 1 + sdw::kW * (kTabWave / 16 - 1) == kTabChunks - 1, "W names the chunks of P, all of them");
// the segment lengths the LDS-DMA kernel is launched on (bcsd_plan_detail::plan_fx: `fits`)
constexpr bool tab_len_ok(int n) { return n > 32 * kBlock && n <= 64 * kBlock; }
inline void build_row_tables(const int32_t* ord, int n, int32_t* tab) {
    const int nl = lanes_of(n);
    for (int Q = 0; Q < kTabChunks; ++Q)
        for (int S = 0; S < 16; ++S) tab[16 * Q + S] = ord[row_of_slot(Q, S, nl, n)];
    int32_t* W = tab + kTabP;
    for (int wave = 0; wave < sdw::kW; ++wave)
        for (int j = 0; j < 3; ++j)
            for (int lane = 0; lane < 64; ++lane)
                W[wave * kTabWave + 64 * j + lane] = tab[16 * (wave + sdw::kW * (4 * j + lane / 16)) + lane % 16];
}
}  // namespace tmj

// LDS of a workgroup of the LDS-DMA kernel: [head: kHeadDoubles][tile: chunks_of(nmax) x 1 032 B]; the u2 area (8 cells x RSU
// 32-bit words, indexed by tag) overlays the first chunks of the tile
constexpr int fd_u2_stride(int nmax) { return 16 * tmj::chunks_of(nmax); }
constexpr int fd_late_chunks(int rsu) { return (sdw::kW * 4 * rsu + tmj::kChunkStride - 1) / tmj::kChunkStride; }  // rsu = fd_u2_stride(nmax)
constexpr size_t fd_lds_bytes(int nmax) { return (size_t)sdw::kHeadDoubles * sizeof(double) + (size_t)tmj::chunks_of(nmax) * tmj::kChunkStride; }

}  // namespace sdfx

// ---- sizing of the register-sort kernels (sd_bcsd_rs.hip) -----------------------------------------------------------------
// samples per lane (K) of the kernels serving segments of up to nmax samples; 0: none does
constexpr int sd_bcsd_rs_width(int nmax) {
    return nmax < 1 ? 0 : nmax <= 64 * 5 ? 5 : nmax <= 64 * 13 ? 13 : nmax <= 64 * 19 ? 19 : nmax <= 64 * 21 ? 21 : nmax <= 64 * 33 ? 33 : 0;
}

inline int sd_bcsd_rs_row_stride(int nmax) {
    const int K = sd_bcsd_rs_width(nmax);
    const int CH = K >= 14 ? (K + 2) / 3 : K;
    int rs = (nmax + K - 1) / K * K + 1;  // the sort stores the pads of the last run; one readable slot past the end
    const int roll = sdw::kPadFront + nmax + CH + 4;  // time-ordered segment with zero pads for the rolling windows
    if (rs < roll) rs = roll;
    while (rs % 4 != 2) ++rs;  // cell rows land 8 or 24 banks apart: conflict-free transposing stores
    return rs;
}

// ---- sizing of the long-segment and generic kernels (sd_bcsd.hip) ---------------------------------------------------------
// register widths of the long kernels' workgroup sort: n <= 1024 * K and the keys fit the LDS; 0: none does
inline int long_width(int nmax, size_t lds_max) {
    const int widths[] = {3, 5, 9, 13, 15, 17, 19};
    for (int K : widths) {
        const int64_t np = ((int64_t)nmax + K - 1) / K * K;
        if (nmax <= 1024 * K && sizeof(double) * (size_t)(np + 1) + sizeof(int) * 1025 + 64 <= lds_max) return K;
    }
    return 0;
}

// cells per workgroup (W) and row stride of the generic kernels; false: not even one cell fits the LDS
inline bool pick_tile_width(size_t lds_max, int nmax, int tiles, int* W, int* stride) {
    // LDS need: tiles * W * stride * 8 (+ W*64*8 staging when tiles == 2)
    const int st = nmax | 1;  // odd stride: rows of different cells start on different banks
    for (int w = 8; w >= 1; w >>= 1) {
        size_t need = (size_t)tiles * w * st * sizeof(double) + (tiles == 2 ? (size_t)w * 64 * sizeof(double) : 0);
        if (need <= lds_max) {
            *W = w;
            *stride = st;
            return true;
        }
    }
    return false;
}

// ---- the plan --------------------------------------------------------------------------------------------------------------
enum class BcsdOp { Fit, Predict, FitPredict };  // Predict: from a fitted state

// Switches of the development library (environment variables, read in one place: sd_bcsd.hip); the production library keeps
// the defaults.
struct BcsdDevSwitches {
    bool path_v1 = false;      // SD_BCSD_PATH=v1: the generic LDS-bitonic kernels for every call
    bool no_fused = false;     // SD_BCSD_FUSED=0: RANK + APPLY for every segment
    bool no_rs_split = false;  // SD_RS_SPLIT=0: one launch of the widest register-sort kernels for every group
    bool no_dma = false;       // SD_FX_NODMA: the register-tile kernel instead of the LDS-DMA one
    bool no_full = false;      // SD_FX_NOFULL: no whole-lane (FULL) launches
    bool no_compact = false;   // SD_FX_NOCOMPACT: no compacting precipitation kernel
    bool no_tab = false;       // SD_FD_NOTAB: the LDS-DMA kernel derives its request rows itself (no row tables)
};

struct BcsdCall {
    BcsdOp op = BcsdOp::Fit;
    int kind = SD_BCSD_TAS;
    bool detrend = false;
    int G = 0;
    std::vector<int> fit_len;      // [G] samples of every group of the fit table (of the state for a predict)
    std::vector<int> predict_len;  // [G] samples of every group of the predict table (empty for a fit)
    int64_t C = 0;
    int64_t ld = 0, ld_p = 0, ld_out = 0;  // leading dimensions of X and y, Xp, out
    bool aligned16 = true;                 // X, y, Xp and out all start on 16-byte boundaries
    size_t lds_max = 0;
    int cu_count = 0;
    BcsdDevSwitches dev;
};

enum class BcsdKernel {
    FdWhole,     // bcsd_fd_kernel<20, false>: LDS-DMA tiles, whole-lane groups
    FdRagged,    // bcsd_fd_kernel<20, true>: LDS-DMA tiles, the other groups
    FxFull,      // bcsd_fx_kernel<K, true, true>: BcsdTemperature, register tiles, whole-lane groups
    FxGeneral,   // bcsd_fx_kernel<K, IDENT, false>
    FxpFull,     // bcsd_fxp_kernel<K, true, true>: BcsdPrecipitation
    FxpGeneral,  // bcsd_fxp_kernel<K, IDENT, false>
    FxpList,     // bcsd_fxp_kernel<K, true, false> over the compacting kernel's second work list (use_worklist = 2)
    FxcFull,     // bcsd_fxc_kernel<K, compact_width(K), true>: BcsdPrecipitation, only the wet days sorted
    FxcGeneral,  // bcsd_fxc_kernel<K, compact_width(K), false>
    RsFit,       // bcsd_rs_kernel<K, MODE_FIT, ...>
    RsRank,      // bcsd_rs_kernel<K, MODE_RANK, ...>
    RsApply,     // bcsd_rs_kernel<K, MODE_APPLY, ..., IDENT>
    LongFit,     // bcsd_long_fit_kernel<K>
    LongPredict, // bcsd_long_predict_kernel<K>
    Fit,         // bcsd_fit_kernel<W>: generic
    Predict,     // bcsd_predict_kernel<W>: generic
};

// the kernels that write a fitted state (the others produce predictions)
inline bool bcsd_fit_stage(BcsdKernel k) { return k == BcsdKernel::RsFit || k == BcsdKernel::LongFit || k == BcsdKernel::Fit; }

struct BcsdLaunch {
    BcsdKernel kernel;
    int width;                 // K (samples per lane), or W (cells per workgroup) of the generic kernels
    bool ident;                // IDENT: every group has equal fit / predict length
    unsigned long long gmask;  // groups this launch serves (bit g); 0: all
    int rs;                    // Params::RS of the register-sort and fused kernels; row stride of the generic kernels
    int slab_k;                // register-sort kernels: K of the call's widest launch (strides of the RANK -> APPLY slabs)
    int use_worklist;          // 1: the fused kernels' work list, 2: the compacting kernel's second list
    size_t lds;                // dynamic LDS bytes
    int64_t grid_x, grid_y;
    int block;
    const char* name;          // profiler name
    bool row_tables = false;   // LDS-DMA kernel: the request rows come from the group tables' row tables (tmj::build_row_tables)
};

struct BcsdPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    std::string message;
    std::vector<BcsdLaunch> launches;
    bool via_state = false;   // fit + predict through a transient state: the fit stage's launches, then the predict stage's
    bool rank_apply = false;  // RANK / APPLY predict: hand-off workspace, inverse-CDF tables unless identity
    bool identity = false;    // equal fit / predict group lengths
    bool fused = false;       // a fused kernel runs first: work lists in the workspace, RANK / APPLY walk them
    int nmax = 0;             // longest segment of the call, fit or predict
};

namespace bcsd_plan_detail {

constexpr int64_t kPitchLimit = (int64_t)1 << 29;  // the fast kernels address rows with a 32-bit byte pitch
constexpr int kDetrendMax = 1024 * 19;

inline int max_of(const std::vector<int>& v) {
    int m = 0;
    for (int x : v) m = x > m ? x : m;
    return m;
}

inline unsigned long long all_groups(int G) { return G >= 64 ? ~0ull : (1ull << G) - 1ull; }

template <class... A>
bool fail(BcsdPlan* pl, int code, const char* fmt, A... a) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a...);
    pl->error = code;
    pl->message = buf;
    pl->launches.clear();
    return false;
}

// a launch of the 512-thread register-sort or fused kernels: 8 workgroups per 8 tiles and served group, or a fixed grid over a list
inline bool add_tiled(const BcsdCall& c, BcsdPlan* pl, BcsdKernel k, int K, bool ident, unsigned long long gmask, int rs, int slab_k,
                      int use_worklist, size_t lds, const char* name) {
    const int64_t ntiles = (c.C + sdw::kW - 1) / sdw::kW, tx = (ntiles + 7) / 8;
    int64_t nb = 8 * tx * (gmask ? __builtin_popcountll(gmask) : c.G);
    if (use_worklist) nb = 2 * (int64_t)(c.cu_count > 0 ? c.cu_count : 256);
    if (nb >= ((int64_t)1 << 31)) return fail(pl, SD_ERR_INVALID, "%s", "grid too large");
    pl->launches.push_back({k, K, ident, gmask, rs, slab_k, use_worklist, lds, nb, 1, sdw::kThreads, name});
    return true;
}

// RANK / APPLY / FIT over every group (or the work list).  A call that needs the 21-wide kernels and has groups fitting 19
// samples per lane (30-day months of a daily series) gives those to a second launch of the narrower, ~10 % cheaper kernels.
inline bool plan_rs(const BcsdCall& c, BcsdPlan* pl, BcsdKernel k, int nmax, const std::vector<int>& glen, bool ident, int use_worklist) {
    const char* name = k == BcsdKernel::RsFit ? "bcsd_rs_fit_kernel" : k == BcsdKernel::RsRank ? "bcsd_rs_rank_kernel" : "bcsd_rs_apply_kernel";
    const int kmax = sd_bcsd_rs_width(nmax), rs = sd_bcsd_rs_row_stride(nmax);
    const size_t lds = ((size_t)sdw::kW * rs + sdw::kHeadDoubles) * sizeof(double);
    unsigned long long narrow = 0ull, wide = 0ull;
    if (!use_worklist && kmax == 21 && c.G <= 64 && !c.dev.no_rs_split)
        for (int g = 0; g < c.G; ++g) (glen[g] <= 64 * 19 ? narrow : wide) |= 1ull << g;
    if (narrow != 0ull && wide != 0ull)
        return add_tiled(c, pl, k, 21, ident, wide, rs, kmax, 0, lds, name) && add_tiled(c, pl, k, 19, ident, narrow, rs, kmax, 0, lds, name);
    return add_tiled(c, pl, k, kmax, ident, 0ull, rs, kmax, use_worklist, lds, name);
}

// the fused kernels of a call with segments of up to nmax <= 1 536 samples (glen: longest segment of every group)
inline bool plan_fx(const BcsdCall& c, BcsdPlan* pl, int nmax, const std::vector<int>& glen, bool ident, bool from_state) {
    const int K = sdfx::fx_width(nmax), rs = sdfx::row_slots(K, nmax);
    const size_t lds = ((size_t)sdw::kW * rs + sdw::kHeadDoubles) * sizeof(double);
    if (lds > c.lds_max) return fail(pl, SD_ERR_UNSUPPORTED, "segment of %d samples needs %zu bytes of LDS", nmax, lds);
    const bool tas = c.kind == SD_BCSD_TAS;
    const auto tiled = [&](BcsdKernel k, bool id, unsigned long long gmask, const char* name) {
        return add_tiled(c, pl, k, K, id, gmask, rs, 0, 0, lds, name);
    };
    const auto general = [&](unsigned long long gmask) {
        return tas ? tiled(BcsdKernel::FxGeneral, ident, gmask, "bcsd_fx_kernel") : tiled(BcsdKernel::FxpGeneral, ident, gmask, "bcsd_fxp_kernel");
    };
    const auto full_tile = [&](unsigned long long gmask) {
        return tas ? tiled(BcsdKernel::FxFull, true, gmask, "bcsd_fx_kernel_full") : tiled(BcsdKernel::FxpFull, true, gmask, "bcsd_fxp_kernel_full");
    };
    // Groups whose segments are whole lanes of K samples (10 of the 12 months of a daily series at K = 20) take the FULL
    // instantiation -- no per-sample predicates --, the others a second launch of the general one.
    unsigned long long full = 0ull, rest = 0ull;
    if (ident && c.G <= 64 && !c.dev.no_full)
        for (int g = 0; g < c.G; ++g) (glen[g] % K == 0 && glen[g] >= sdfx::full_min_len(K) ? full : rest) |= 1ull << g;
    if (ident && sdfx::compact_width(K) != 0 && !tas && !from_state && c.G <= 64 && !c.dev.no_compact) {
        // BcsdPrecipitation fit + predict: only the wet days are sorted; segments with too many of them for the narrow network
        // come back on the second list and take the K-wide kernel
        if ((full | rest) == 0ull) rest = all_groups(c.G);
        if (full != 0ull && !tiled(BcsdKernel::FxcFull, true, full, "bcsd_fxc_kernel_full")) return false;
        if (rest != 0ull && !tiled(BcsdKernel::FxcGeneral, true, rest, "bcsd_fxc_kernel")) return false;
        return add_tiled(c, pl, BcsdKernel::FxpList, K, true, 0ull, rs, 0, 2, lds, "bcsd_fxp_kernel_list");
    }
    // BcsdTemperature fit + predict on fields that allow 16-byte requests of whole cell pairs: the kernel whose tiles land by
    // LDS-DMA, the whole-lane months in one launch, the others (February, December) in a second one of the ragged instantiation.
    // Each set is checked on its own longest and shortest group: more than 32 lanes of data in every group, at most 64, the u2
    // area under 40 chunks, two workgroups per CU.  A set that does not qualify takes the register-tile kernel.
    const bool dma = ident && K == 20 && tas && !from_state && c.C >= sdw::kW && c.C % 2 == 0 && c.ld % 2 == 0 && c.ld_p % 2 == 0 &&
                     c.ld_out % 2 == 0 && c.aligned16 && !c.dev.no_dma;
    int nmx[2] = {0, 0};  // longest segment of the whole-lane set, of the rest
    const auto fits = [&](unsigned long long mask, int s) {
        int nmn = 1 << 30;
        for (int g = 0; g < c.G; ++g)
            if ((mask >> g) & 1ull) {
                nmx[s] = glen[g] > nmx[s] ? glen[g] : nmx[s];
                nmn = glen[g] < nmn ? glen[g] : nmn;
            }
        const int n = nmx[s], late = sdfx::fd_late_chunks(sdfx::fd_u2_stride(n)), nch = sdfx::tmj::chunks_of(n);
        return nmn > 640 && nch <= 80 && late <= 40 && nch - late <= 40 && 2 * sdfx::fd_lds_bytes(n) <= c.lds_max;
    };
    const auto fd = [&](unsigned long long mask, int s, BcsdKernel k, const char* name) {
        if (!add_tiled(c, pl, k, 20, true, mask, sdfx::fd_u2_stride(nmx[s]), 0, 0, sdfx::fd_lds_bytes(nmx[s]), name)) return false;
        pl->launches.back().row_tables = !c.dev.no_tab;  // (`fits` admits the lengths of tmj::tab_len_ok only)
        return true;
    };
    const bool fd_full = dma && full != 0ull && fits(full, 0), fd_rest = dma && rest != 0ull && fits(rest, 1);
    if (full == 0ull && !fd_rest) return general(0ull);
    if (full != 0ull && !(fd_full ? fd(full, 0, BcsdKernel::FdWhole, "bcsd_fd_kernel") : full_tile(full))) return false;
    if (fd_rest) return fd(rest, 1, BcsdKernel::FdRagged, "bcsd_fd_kernel_ragged");
    return rest == 0ull || general(rest);
}

}  // namespace bcsd_plan_detail

namespace bcsd_plan_detail {

// predict by the register-sort path: the fused kernels first where they serve the segments, RANK + APPLY over their work list
// (or over every segment)
inline bool plan_rank_apply(const BcsdCall& c, BcsdPlan* pl, bool from_state) {
    const int nmax = pl->nmax;
    std::vector<int> glen((size_t)c.G);  // longest segment of every group, fit or predict
    for (int g = 0; g < c.G; ++g) glen[g] = c.fit_len[g] > c.predict_len[g] ? c.fit_len[g] : c.predict_len[g];
    pl->rank_apply = true;
    pl->identity = c.fit_len == c.predict_len;  // no inverse-CDF tables needed
    pl->fused = !c.dev.no_fused && !c.detrend && sdfx::fx_width(nmax) != 0;  // detrend: RANK / APPLY carry the trend lines
    if (pl->fused && !plan_fx(c, pl, nmax, glen, pl->identity, from_state)) return false;
    const int list = pl->fused ? 1 : 0;
    return plan_rs(c, pl, BcsdKernel::RsRank, nmax, glen, false, list) && plan_rs(c, pl, BcsdKernel::RsApply, nmax, glen, pl->identity, list);
}

inline bool fail_detrend(BcsdPlan* pl, int nmax) {
    return fail(pl, SD_ERR_UNSUPPORTED, "detrended quantile mapping serves group segments of up to %d samples (longest here: %d)", kDetrendMax, nmax);
}

inline bool fail_lds(const BcsdCall& c, BcsdPlan* pl, int nmax) {
    return fail(pl, SD_ERR_UNSUPPORTED, "BCSD segment of %d samples does not fit the %zu-byte LDS", nmax, c.lds_max);
}

inline bool register_path(const BcsdCall& c, int nmax, int64_t ld_max) {
    return !c.dev.path_v1 && ld_max < kPitchLimit && sd_bcsd_rs_width(nmax) != 0;
}

inline bool long_path(const BcsdCall& c, int nmax) { return !c.dev.path_v1 && nmax > 64 * 33 && long_width(nmax, c.lds_max) != 0; }

// the fit stage: writes the state (x_climo, y_climo, sorted y)
inline bool plan_fit(const BcsdCall& c, BcsdPlan* pl) {
    const int nmax = max_of(c.fit_len);
    if (register_path(c, nmax, c.ld)) return plan_rs(c, pl, BcsdKernel::RsFit, nmax, c.fit_len, false, 0);
    if (long_path(c, nmax)) {
        const int K = long_width(nmax, c.lds_max), np = (nmax + K - 1) / K * K;
        pl->launches.push_back({BcsdKernel::LongFit, K, false, 0ull, 0, 0, 0, sizeof(double) * (size_t)(np + 1) + sizeof(int) * 1025, c.C, c.G,
                                1024, "bcsd_long_fit_kernel"});
        return true;
    }
    int W = 0, stride = 0;
    if (!pick_tile_width(c.lds_max, nmax, 1, &W, &stride)) return fail_lds(c, pl, nmax);
    if (c.detrend) return fail_detrend(pl, nmax);
    pl->launches.push_back({BcsdKernel::Fit, W, false, 0ull, stride, 0, 0, (size_t)W * stride * sizeof(double), (c.C + W - 1) / W, c.G, 64 * W,
                            "bcsd_fit_kernel"});
    return true;
}

// the predict stage from a fitted state
inline bool plan_predict(const BcsdCall& c, BcsdPlan* pl, int64_t ld_max) {
    const int np = max_of(c.predict_len);
    if (register_path(c, pl->nmax, ld_max)) return plan_rank_apply(c, pl, true);
    const bool lng = long_path(c, pl->nmax);
    if (c.detrend && !lng) return fail_detrend(pl, pl->nmax);
    if (lng) {
        const int K = long_width(np, c.lds_max), npad = (np + K - 1) / K * K;
        pl->launches.push_back({BcsdKernel::LongPredict, K, false, 0ull, 0, 0, 0, sizeof(double) * (size_t)(npad + 1) + sizeof(int) * 1025, c.C,
                                c.G, 1024, "bcsd_long_predict_kernel"});
        return true;
    }
    int W = 0, stride = 0;
    if (!pick_tile_width(c.lds_max, np, 2, &W, &stride)) return fail_lds(c, pl, np);
    pl->launches.push_back({BcsdKernel::Predict, W, false, 0ull, stride, 0, 0, (size_t)2 * W * stride * sizeof(double) + (size_t)W * 64 * sizeof(double),
                            (c.C + W - 1) / W, c.G, 64 * W, "bcsd_predict_kernel"});
    return true;
}

}  // namespace bcsd_plan_detail

inline BcsdPlan bcsd_plan(const BcsdCall& c) {
    using namespace bcsd_plan_detail;
    BcsdPlan pl;
    pl.nmax = max_of(c.fit_len) > max_of(c.predict_len) ? max_of(c.fit_len) : max_of(c.predict_len);
    switch (c.op) {
        case BcsdOp::Fit: plan_fit(c, &pl); break;
        case BcsdOp::Predict: plan_predict(c, &pl, c.ld_p > c.ld_out ? c.ld_p : c.ld_out); break;
        case BcsdOp::FitPredict: {
            const int64_t ld_p = c.ld_p > c.ld_out ? c.ld_p : c.ld_out;
            if (register_path(c, pl.nmax, c.ld > ld_p ? c.ld : ld_p)) {
                plan_rank_apply(c, &pl, false);  // no persisted state: HBM traffic = 3 reads + 1 write per sample
            } else {
                pl.via_state = true;
                if (plan_fit(c, &pl)) plan_predict(c, &pl, ld_p);
            }
            break;
        }
    }
    return pl;
}
