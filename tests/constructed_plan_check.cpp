// Host driver of the constructed-analog launch plans (scikit-downscale_amd/csrc/sd_constructed_plan.h) for
// tests/test_constructed_plan.py: reads one request per line on stdin.
//   "consts"  -> "consts sel_q=.. sel_l=.. sel_cols=.. sel_block=.. sel_lds=.. wgt_block=.. wgt_cols=.. wgt_entries=.. wgt_per_thread=..
//                app_cells=.. app_rows=.. app_waves=.. app_block=.. max_k=.. max_tl=.. max_cc=.."
//   "select Tl Tq Cc ld_l ld_q k period window <wc>"   <wc>: "ones", or "set <i> <value>": ones but wc[i] = value (strtod: nan, inf, -1)
//        -> "error <code> <message>" or "plan block=.. lds_bytes=.. blocks=.. q_tiles=.. l_tiles=.."
//   "weights Tl Tq Cc ld_l ld_q k kind ridge <wc>"  -> "error ..." or "plan block=.. blocks=.."
//   "apply Tl Cf ld_f Tq q0 q1 ld_out k"            -> "error ..." or "plan block=.. blocks=.. ctiles=.. row_groups=.."
//   "cover_select Tl Tq"  -> walks every workgroup, wave and slot of ca_select_kernel's merge and every (tile, lane) of its sweep:
//        "cover q_min=.. q_max=.. q_outside=.. t_min=.. t_max=.. t_outside=..": how often the least and the most visited target and
//        library day are visited, and how many visits fall outside them
//   "cover_apply Cf Tq q0 q1" -> walks every workgroup, wave and lane as ca_apply_kernel decodes them:
//        "cover min=.. max=.. outside=.. tiles_in_first=..": how often the least and most written (row, cell) of [q0, q1) x Cf is written,
//        the writes outside, and the distinct cell tiles among the first row_groups workgroups of XCD 0 (1: an XCD walks the row groups of one tile first)
//   each answer ends with "end".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <set>
#include <string>
#include <vector>

#include "sd_constructed_plan.h"

static double number() {
    std::string w;
    std::cin >> w;
    return strtod(w.c_str(), nullptr);
}

static std::vector<double> column_weights(int64_t Cc) {
    std::vector<double> wc((size_t)std::max<int64_t>(0, std::min<int64_t>(Cc, sdca::kMaxCc)), 1.0);
    std::string mode;
    std::cin >> mode;
    if (mode == "set") {
        int64_t i;
        std::cin >> i;
        const double v = number();
        if (i >= 0 && i < (int64_t)wc.size()) wc[(size_t)i] = v;
    }
    return wc;
}

static bool refused(const CaPlan& pl) {
    if (pl.error == SD_OK) return false;
    printf("error %d %s\nend\n", pl.error, pl.message);
    return true;
}

int main() {
    using namespace sdca;
    std::string word;
    while (std::cin >> word) {
        if (word == "consts") {
            printf("consts sel_q=%d sel_l=%d sel_cols=%d sel_block=%d sel_lds=%lld wgt_block=%d wgt_cols=%d wgt_entries=%d wgt_per_thread=%d "
                   "app_cells=%d app_rows=%d app_waves=%d app_block=%d max_k=%d max_tl=%lld max_cc=%lld\nend\n",
                   kSelQ, kSelL, kSelCols, kSelBlock, (long long)sel_lds_bytes(), kWgtBlock, kWgtCols, kWgtEntries, kWgtPerThread, kAppCells,
                   kAppRows, kAppWaves, kAppBlock, kMaxK, (long long)kMaxTl, (long long)kMaxCc);
        } else if (word == "select" || word == "weights") {
            CaCoarse c;
            int64_t period = 0, window = 0;
            int kind = 0;
            double ridge = 0.0;
            std::cin >> c.Tl >> c.Tq >> c.Cc >> c.ld_l >> c.ld_q >> c.k;
            if (word == "select") {
                std::cin >> period >> window;
            } else {
                std::cin >> kind;
                ridge = number();
            }
            const std::vector<double> wc = column_weights(c.Cc);
            c.wc = wc.data();
            const CaPlan pl = word == "select" ? ca_select_plan(c, period, window) : ca_weights_plan(c, kind, ridge);
            if (refused(pl)) continue;
            if (word == "select")
                printf("plan block=%d lds_bytes=%lld blocks=%lld q_tiles=%lld l_tiles=%lld\nend\n", pl.block, (long long)pl.lds_bytes,
                       (long long)pl.blocks, (long long)pl.q_tiles, (long long)pl.l_tiles);
            else
                printf("plan block=%d blocks=%lld\nend\n", pl.block, (long long)pl.blocks);
        } else if (word == "apply") {
            CaApplyCall c;
            std::cin >> c.Tl >> c.Cf >> c.ld_f >> c.Tq >> c.q0 >> c.q1 >> c.ld_out >> c.k;
            const CaPlan pl = ca_apply_plan(c);
            if (refused(pl)) continue;
            printf("plan block=%d blocks=%lld ctiles=%lld row_groups=%lld\nend\n", pl.block, (long long)pl.blocks, (long long)pl.ctiles,
                   (long long)pl.row_groups);
        } else if (word == "cover_select") {
            CaCoarse c;
            std::cin >> c.Tl >> c.Tq;
            c.Cc = c.ld_l = c.ld_q = 1, c.k = 1;
            const double one = 1.0;
            c.wc = &one;
            const CaPlan pl = ca_select_plan(c, 1, -1);
            if (refused(pl)) continue;
            std::vector<int> q_seen((size_t)c.Tq, 0), t_seen((size_t)c.Tl, 0);
            long long q_outside = 0, t_outside = 0;
            const int waves = kSelBlock / kLanes, per_wave = kSelQ / waves;
            for (int64_t b = 0; b < pl.blocks; ++b)
                for (int wave = 0; wave < waves; ++wave)
                    for (int u = 0; u < per_wave; ++u) {
                        const int64_t q = b * kSelQ + wave * per_wave + u;
                        if (q >= c.Tq) continue;  // (the kernel's guard)
                        if (q < 0) ++q_outside;
                        else ++q_seen[(size_t)q];
                    }
            for (int64_t t0 = 0; t0 < c.Tl; t0 += kSelL)  // the merge of one target over the sweep
                for (int h = 0; h < kSelL; h += kLanes)
                    for (int lane = 0; lane < kLanes; ++lane) {
                        const int64_t t = t0 + h + lane;
                        if (t >= c.Tl) continue;  // (the kernel's guard)
                        if (t < 0) ++t_outside;
                        else ++t_seen[(size_t)t];
                    }
            printf("cover q_min=%d q_max=%d q_outside=%lld t_min=%d t_max=%d t_outside=%lld\nend\n", *std::min_element(q_seen.begin(), q_seen.end()),
                   *std::max_element(q_seen.begin(), q_seen.end()), q_outside, *std::min_element(t_seen.begin(), t_seen.end()),
                   *std::max_element(t_seen.begin(), t_seen.end()), t_outside);
        } else if (word == "cover_apply") {
            CaApplyCall c;
            std::cin >> c.Cf >> c.Tq >> c.q0 >> c.q1;
            c.Tl = 1, c.ld_f = c.ld_out = c.Cf, c.k = 1;
            const CaPlan pl = ca_apply_plan(c);
            if (refused(pl)) continue;
            const int64_t rows = c.q1 - c.q0;
            std::vector<int> seen((size_t)(rows * c.Cf), 0);
            long long outside = 0;
            std::set<int64_t> first_tiles;
            const int per_wave = kAppRows / kAppWaves;
            for (int64_t b = 0; b < pl.blocks; ++b) {
                const int64_t slot = b / kXcds, rg = slot % pl.row_groups, tile = slot / pl.row_groups * kXcds + b % kXcds;
                if (tile * kAppCells >= c.Cf) continue;  // (the kernel's guard: the padding of the last round of tiles)
                if (b % kXcds == 0 && slot < pl.row_groups) first_tiles.insert(tile);
                for (int wave = 0; wave < kAppWaves; ++wave) {
                    const int64_t qa = c.q0 + rg * kAppRows + (int64_t)wave * per_wave;
                    for (int64_t q = qa; q < std::min<int64_t>(qa + per_wave, c.q1); ++q)
                        for (int lane = 0; lane < kLanes; ++lane) {
                            const int64_t f = tile * kAppCells + lane;
                            if (f >= c.Cf) continue;  // (the kernel's guard)
                            if (q < c.q0 || q >= c.q1 || f < 0) ++outside;
                            else ++seen[(size_t)((q - c.q0) * c.Cf + f)];
                        }
                }
            }
            printf("cover min=%d max=%d outside=%lld tiles_in_first=%zu\nend\n", *std::min_element(seen.begin(), seen.end()),
                   *std::max_element(seen.begin(), seen.end()), outside, first_tiles.size());
        } else {
            printf("error -1 unknown request %s\nend\n", word.c_str());
        }
    }
    return 0;
}
