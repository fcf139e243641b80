// Host driver of the resampling launch plan (scikit-downscale_amd/csrc/sd_resample_plan.h) for tests/test_resample_plan.py: reads one
// request per line on stdin.
//   "plan op f32 T C ld M ld_out src_aligned16 out_aligned16"
//        -> "error <code> <message>" or "plan cols=.. block=.. ctiles=.. bin_groups=.. blocks=.. bins_per_group=.. bins_per_wave=.. batch=..";
//   "offsets op f32 T C ld M ld_out src_aligned16 out_aligned16 o[0] .. o[M]"   (M >= 1)
//        -> the same, after resample_check_offsets;
//   "cover op f32 T C ld M ld_out src_aligned16 out_aligned16"
//        -> walks every workgroup, wave and lane of the plan as resample_kernel decodes them and prints
//           "cover cells_min=.. cells_max=.. bins_min=.. bins_max=.. outside=..": how often the least and the most covered cell and
//           bin of the call are written, and how many writes fall outside them (small sizes only);
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_resample_plan.h"

static ResampleCall read_call() {
    ResampleCall c;
    int f32 = 0, sa = 1, oa = 1;
    std::cin >> c.op >> f32 >> c.T >> c.C >> c.ld >> c.M >> c.ld_out >> sa >> oa;
    c.src_is_f32 = f32 != 0, c.src_aligned16 = sa != 0, c.out_aligned16 = oa != 0;
    return c;
}

int main() {
    using namespace sdrs;
    std::string word;
    while (std::cin >> word) {
        const ResampleCall c = read_call();
        ResamplePlan pl = resample_plan(c);
        if (word == "offsets") {
            std::vector<int64_t> off((size_t)(c.M > 0 ? c.M + 1 : 0));
            for (int64_t& v : off) std::cin >> v;
            pl = resample_check_offsets(pl, c, off.data());
        }
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        if (word != "cover") {
            printf("plan cols=%d block=%d ctiles=%lld bin_groups=%lld blocks=%lld bins_per_group=%d bins_per_wave=%d batch=%d\nend\n", pl.cols,
                   pl.block, (long long)pl.ctiles, (long long)pl.bin_groups, (long long)pl.blocks, kBinsPerGroup, kBinsPerWave, kBatch);
            continue;
        }
        // the decode of resample_kernel: cell tile fastest, then the run of bins; a wave takes kBinsPerWave consecutive bins
        std::vector<int> cells((size_t)c.C, 0), bins((size_t)c.M, 0);
        long long outside = 0;
        for (int64_t b = 0; b < pl.blocks; ++b) {
            const int64_t ctile = b % pl.ctiles, group = b / pl.ctiles;
            for (int thread = 0; thread < pl.block; ++thread) {
                const int lane = thread % kLanes, wave = thread / kLanes;
                const int64_t c0 = (ctile * kLanes + lane) * pl.cols;
                if (c0 >= c.C) continue;
                const int64_t m0 = group * kBinsPerGroup + (int64_t)wave * kBinsPerWave;
                for (int k = 0; k < kBinsPerWave; ++k) {
                    const int64_t m = m0 + k;
                    if (m >= c.M) break;
                    for (int v = 0; v < pl.cols; ++v) {
                        if (c0 + v >= c.C || group >= pl.bin_groups) {
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
