// Host driver of the disaggregation launch plan (scikit-downscale_amd/csrc/sd_disagg_plan.h) for tests/test_disagg_plan.py: reads one
// request per line on stdin.  A call is
//   "op f32 To C Tout M ld_t ld_obs ld_out has_climo has_group G ld_c target_a16 obs_a16 out_a16 climo_a16".
//   "plan <call>"
//        -> "error <code> <message>" or "plan cols=.. block=.. ctiles=.. bin_groups=.. blocks=.. bins_per_group=.. bins_per_wave=.. batch=..";
//   "tables <call> src_row[0] .. src_row[Tout - 1] o[0] .. o[M] (group[0] .. group[M - 1] with has_group)"   (small sizes only)
//        -> the same, after disagg_check_tables;
//   "cover <call> o[0] .. o[M]"
//        -> walks every workgroup, wave and lane of the plan as disagg_kernel decodes them, with the bins of this offsets table, and
//           prints "cover written_min=.. written_max=.. outside=..": how often the least and the most written (row, cell) of the
//           [Tout, C] output is stored, and how many stores fall outside it (small sizes only);
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_disagg_plan.h"

static DisaggCall read_call() {
    DisaggCall c;
    int f32 = 0, hc = 0, hg = 0, ta = 1, oa = 1, ua = 1, ca = 1;
    std::cin >> c.op >> f32 >> c.To >> c.C >> c.Tout >> c.M >> c.ld_t >> c.ld_obs >> c.ld_out >> hc >> hg >> c.G >> c.ld_c >> ta >> oa >> ua >> ca;
    c.obs_is_f32 = f32 != 0, c.has_climo = hc != 0, c.has_group = hg != 0;
    c.target_aligned16 = ta != 0, c.obs_aligned16 = oa != 0, c.out_aligned16 = ua != 0, c.climo_aligned16 = ca != 0;
    return c;
}

int main() {
    using namespace sddg;
    std::string word;
    while (std::cin >> word) {
        const DisaggCall c = read_call();
        DisaggPlan pl = disagg_plan(c);
        std::vector<int64_t> rows, off;
        std::vector<int32_t> group;
        if (word == "tables") {
            rows.resize((size_t)(c.Tout > 0 ? c.Tout : 0));
            for (int64_t& v : rows) std::cin >> v;
        }
        if (word == "tables" || word == "cover") {
            off.resize((size_t)(c.M > 0 ? c.M + 1 : 0));
            for (int64_t& v : off) std::cin >> v;
        }
        if (word == "tables") {
            if (c.has_group) {
                group.resize((size_t)(c.M > 0 ? c.M : 0));
                for (int32_t& v : group) std::cin >> v;
            }
            pl = disagg_check_tables(pl, c, rows.data(), off.data(), c.has_group ? group.data() : nullptr);
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
        // the decode of disagg_kernel: cell tile fastest, then the run of bins; a wave takes kBinsPerWave consecutive bins and stores the
        // rows of each in batches of kBatch
        std::vector<int> written((size_t)(c.Tout * c.C), 0);
        long long outside = 0;
        for (int64_t b = 0; b < pl.blocks; ++b) {
            const int64_t ctile = b % pl.ctiles, bins = b / pl.ctiles;
            for (int thread = 0; thread < pl.block; ++thread) {
                const int lane = thread % kLanes, wave = thread / kLanes;
                const int64_t c0 = (ctile * kLanes + lane) * pl.cols;
                if (c0 >= c.C) continue;
                const int64_t m0 = bins * kBinsPerGroup + (int64_t)wave * kBinsPerWave;
                for (int k = 0; k < kBinsPerWave; ++k) {
                    const int64_t m = m0 + k;
                    if (m >= c.M) break;
                    const int64_t r0 = off[(size_t)m], r1 = off[(size_t)m + 1];
                    for (int64_t r = r0; r < r1; r += kBatch)
                        for (int u = 0; u < kBatch; ++u) {
                            if (r + u >= r1) break;
                            for (int v = 0; v < pl.cols; ++v) {
                                if (c0 + v >= c.C || r + u < 0 || r + u >= c.Tout)
                                    ++outside;
                                else
                                    ++written[(size_t)((r + u) * c.C + c0 + v)];
                            }
                        }
                }
            }
        }
        int wmin = written[0], wmax = written[0];
        for (int v : written) wmin = v < wmin ? v : wmin, wmax = v > wmax ? v : wmax;
        printf("cover written_min=%d written_max=%d outside=%lld\nend\n", wmin, wmax, outside);
    }
    return 0;
}
