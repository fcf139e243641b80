// Host driver of the paired skill launch plan (scikit-downscale_amd/csrc/sd_skill_plan.h) for tests/test_skill_plan.py: reads one
// request per line on stdin.  CALL = "a_f32 b_f32 T C ld_a ld_b M nstat s0 s1 s2 s3 s4 s5 s6 ld_out stride_out a_aligned16 b_aligned16
// out_aligned16".
//   "plan CALL"    the table is made here: offsets[m] = m * T / M
//        -> "error <code> <message>" or "plan cols=.. block=.. ctiles=.. bin_groups=.. blocks=.. bins_per_group=.. bins_per_wave=.. batch=..";
//   "tables CALL o[0] .. o[M]"
//        -> the same, with the table of the request;
//   "cover CALL"
//        -> walks every workgroup, wave and lane of the plan as skill_kernel decodes them and prints
//           "cover min=.. max=.. outside=..": how often the least and the most covered (bin, cell) of the call is written, and how
//           many writes fall outside the call (small sizes only);
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_skill_plan.h"

static SkillCall read_call() {
    SkillCall c;
    int af = 0, bf = 0, aa = 1, ba = 1, oa = 1;
    std::cin >> af >> bf >> c.T >> c.C >> c.ld_a >> c.ld_b >> c.M >> c.nstat;
    for (int& s : c.stats) std::cin >> s;
    std::cin >> c.ld_out >> c.stride_out >> aa >> ba >> oa;
    c.a_is_f32 = af != 0, c.b_is_f32 = bf != 0;
    c.a_aligned16 = aa != 0, c.b_aligned16 = ba != 0, c.out_aligned16 = oa != 0;
    return c;
}

int main() {
    using namespace sdsk;
    const int64_t kMostMade = 50000000;  // tables longer than this are not made: the plan has to refuse before it reads them
    std::string word;
    while (std::cin >> word) {
        const SkillCall c = read_call();
        std::vector<int64_t> off;
        if (word == "tables") {
            off.resize((size_t)(c.M > 0 ? c.M + 1 : 0));
            for (int64_t& v : off) std::cin >> v;
        } else if (c.M > 0 && c.M <= kMostMade && c.T > 0) {
            for (int64_t m = 0; m <= c.M; ++m) off.push_back((int64_t)((__int128)m * c.T / c.M));
        }
        const SkillPlan pl = skill_plan(c, off.empty() ? nullptr : off.data());
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        if (word != "cover") {
            printf("plan cols=%d block=%d ctiles=%lld bin_groups=%lld blocks=%lld bins_per_group=%d bins_per_wave=%d batch=%d\nend\n", pl.cols,
                   pl.block, (long long)pl.ctiles, (long long)pl.bin_groups, (long long)pl.blocks, kBinsPerGroup, kBinsPerWave, kBatch);
            continue;
        }
        // the decode of skill_kernel (lane_place): cell tile fastest, then the run of bins; a wave takes kBinsPerWave consecutive bins
        std::vector<int> written((size_t)(c.M * c.C), 0);
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
                        if (c0 + v >= c.C)
                            ++outside;
                        else
                            ++written[(size_t)(m * c.C + c0 + v)];
                    }
                }
            }
        }
        int lo = written[0], hi = written[0];
        for (int v : written) lo = v < lo ? v : lo, hi = v > hi ? v : hi;
        printf("cover min=%d max=%d outside=%lld\nend\n", lo, hi, outside);
    }
    return 0;
}
