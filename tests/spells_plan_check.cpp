// Host driver of the threshold / spell launch plan (scikit-downscale_amd/csrc/sd_spells_plan.h) for tests/test_spells_plan.py: reads one
// request per line on stdin.  CALL = "op f32 T C ld has_table G ld_t has_group M min_length nstat s0 s1 s2 s3 s4 s5 ld_out stride_out
// src_aligned16 table_aligned16 out_aligned16".
//   "plan CALL"    the tables are made here: offsets[m] = m * T / M, group[r] = r % G (none where has_group is 0)
//        -> "error <code> <message>" or "plan cols=.. block=.. ctiles=.. bin_groups=.. blocks=.. bins_per_group=.. bins_per_wave=.. batch=..";
//   "tables CALL g[0] .. g[T - 1] o[0] .. o[M]"    (the group ids only where has_group is 1)
//        -> the same, with the tables of the request;
//   "cover CALL"
//        -> walks every workgroup, wave and lane of the plan as spells_kernel decodes them and prints
//           "cover cells_min=.. cells_max=.. bins_min=.. bins_max=.. outside=..": how often the least and the most covered cell and
//           bin of the call are written, and how many writes fall outside them (small sizes only);
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_spells_plan.h"

static SpellsCall read_call() {
    SpellsCall c;
    int f32 = 0, ht = 0, hg = 0, sa = 1, ta = 1, oa = 1;
    std::cin >> c.op >> f32 >> c.T >> c.C >> c.ld >> ht >> c.G >> c.ld_t >> hg >> c.M >> c.min_length >> c.nstat;
    for (int& s : c.stats) std::cin >> s;
    std::cin >> c.ld_out >> c.stride_out >> sa >> ta >> oa;
    c.src_is_f32 = f32 != 0, c.has_table = ht != 0, c.has_group = hg != 0;
    c.src_aligned16 = sa != 0, c.table_aligned16 = ta != 0, c.out_aligned16 = oa != 0;
    return c;
}

int main() {
    using namespace sdsp;
    const int64_t kMostMade = 50000000;  // tables longer than this are not made: the plan has to refuse before it reads them
    std::string word;
    while (std::cin >> word) {
        const SpellsCall c = read_call();
        std::vector<int32_t> group;
        std::vector<int64_t> off;
        if (word == "tables") {
            group.resize((size_t)(c.has_group && c.T > 0 ? c.T : 0));
            off.resize((size_t)(c.M > 0 ? c.M + 1 : 0));
            for (int32_t& v : group) std::cin >> v;
            for (int64_t& v : off) std::cin >> v;
        } else {
            if (c.has_group && c.T > 0 && c.T <= kMostMade && c.G > 0)
                for (int64_t r = 0; r < c.T; ++r) group.push_back((int32_t)(r % c.G));
            if (c.M > 0 && c.M <= kMostMade && c.T > 0)
                for (int64_t m = 0; m <= c.M; ++m) off.push_back((int64_t)((__int128)m * c.T / c.M));
        }
        const SpellsPlan pl = spells_plan(c, group.empty() ? nullptr : group.data(), off.empty() ? nullptr : off.data());
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        if (word != "cover") {
            printf("plan cols=%d block=%d ctiles=%lld bin_groups=%lld blocks=%lld bins_per_group=%d bins_per_wave=%d batch=%d\nend\n", pl.cols,
                   pl.block, (long long)pl.ctiles, (long long)pl.bin_groups, (long long)pl.blocks, kBinsPerGroup, kBinsPerWave, kBatch);
            continue;
        }
        // the decode of spells_kernel (lane_place): cell tile fastest, then the run of bins; a wave takes kBinsPerWave consecutive bins
        std::vector<int> cells((size_t)c.C, 0), bins((size_t)c.M, 0);
        long long outside = 0;
        for (int64_t b = 0; b < pl.blocks; ++b) {
            const int64_t ctile = b % pl.ctiles, run = b / pl.ctiles;
            for (int thread = 0; thread < pl.block; ++thread) {
                const int lane = thread % kLanes, wave = thread / kLanes;
                const int64_t c0 = (ctile * kLanes + lane) * pl.cols;
                if (c0 >= c.C) continue;
                const int64_t m0 = run * kBinsPerGroup + (int64_t)wave * kBinsPerWave;
                for (int k = 0; k < kBinsPerWave; ++k) {
                    const int64_t m = m0 + k;
                    if (m >= c.M) break;
                    for (int v = 0; v < pl.cols; ++v) {
                        if (c0 + v >= c.C || run >= pl.bin_groups) {
                            ++outside;
                            continue;
                        }
                        if (m == 0) ++cells[(size_t)(c0 + v)];
                        if (c0 + v == 0) ++bins[(size_t)m];
                    }
                }
            }
        }
        int cmin = cells[0], cmax = cells[0], bmin = bins[0], bmax = bins[0];
        for (int v : cells) cmin = v < cmin ? v : cmin, cmax = v > cmax ? v : cmax;
        for (int v : bins) bmin = v < bmin ? v : bmin, bmax = v > bmax ? v : bmax;
        printf("cover cells_min=%d cells_max=%d bins_min=%d bins_max=%d outside=%lld\nend\n", cmin, cmax, bmin, bmax, outside);
    }
    return 0;
}
