// Host driver of the rolling launch plan (scikit-downscale_amd/csrc/sd_rolling_plan.h) for tests/test_rolling_plan.py: reads one
// request per line on stdin.  A call is "op f32 T C ld window back min_periods ddof wrap t0 n_out ld_out src_a16 out_a16".
//   "plan <call>"
//        -> "error <code> <message>" or "plan cols=.. block=.. staged=.. run=.. lds_rows=.. lds_bytes=.. ctiles=.. row_groups=.. blocks=..
//           budget=.. batch=..";
//   "cover <call>"   (small sizes only)
//        -> walks every workgroup, wave and lane of the plan as rolling_kernel decodes them and prints "cover owned_min=.. owned_max=..
//           unstaged=.. outside=.. lds_rows_max=..": how many lanes own the least and the most owned (output row, cell); how many
//           window positions of a staged workgroup were not staged by it before they are read (or hold another row than the window
//           wants); how many accesses fall outside the source, the output or the staged rows of the plan; and the most rows a workgroup
//           stages;
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_rolling_plan.h"

static RollingCall read_call() {
    RollingCall c;
    int f32 = 0, wrap = 0, a = 1, b = 1;
    std::cin >> c.op >> f32 >> c.T >> c.C >> c.ld >> c.window >> c.back >> c.min_periods >> c.ddof >> wrap >> c.t0 >> c.n_out >> c.ld_out >> a >> b;
    c.src_is_f32 = f32 != 0, c.wrap = wrap != 0, c.src_aligned16 = a != 0, c.out_aligned16 = b != 0;
    return c;
}

static int64_t row_mod(int64_t p, int64_t T) { return p < 0 ? p + T : p >= T ? p - T : p; }

int main() {
    using namespace sdrl;
    std::string word;
    while (std::cin >> word) {
        const RollingCall c = read_call();
        const RollingPlan pl = rolling_plan(c);
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        if (word == "plan") {
            printf("plan cols=%d block=%d staged=%d run=%d lds_rows=%lld lds_bytes=%lld ctiles=%lld row_groups=%lld blocks=%lld budget=%lld batch=%d\nend\n",
                   pl.cols, pl.block, (int)pl.staged, pl.run, (long long)pl.lds_rows, (long long)pl.lds_bytes, (long long)pl.ctiles,
                   (long long)pl.row_groups, (long long)pl.blocks, (long long)kLdsBudget, kBatch);
            continue;
        }
        // the decode of rolling_kernel: cell tile fastest, then the run of pl.run output rows; wave k takes the rows k, k + kWaves, ...
        std::vector<int> owned((size_t)(c.n_out * c.C), 0);
        long long outside = 0, unstaged = 0, lds_rows_max = 0;
        for (int64_t b = 0; b < pl.blocks; ++b) {
            const int64_t ctile = b % pl.ctiles, rgroup = b / pl.ctiles;
            const int64_t ta = c.t0 + rgroup * pl.run, stop = ta + pl.run, tb = stop < c.t0 + c.n_out ? stop : c.t0 + c.n_out;
            const int64_t first = ta - c.back, staged = (tb - ta) + c.window - 1;
            // the staging: wave by wave, batches of kBatch rows, a row past the end is the last one again
            std::vector<int64_t> held((size_t)(pl.staged ? staged : 0), -1);  // the source row a staged row holds
            if (pl.staged) {
                if (staged > pl.lds_rows || staged * kLanes * pl.cols * (c.src_is_f32 ? 4 : 8) > kLdsBudget) ++outside;
                lds_rows_max = staged > lds_rows_max ? staged : lds_rows_max;
                for (int wave = 0; wave < kWaves; ++wave)
                    for (int64_t j0 = (int64_t)wave * kBatch; j0 < staged; j0 += kWaves * kBatch)
                        for (int u = 0; u < kBatch; ++u) {
                            const int64_t j = j0 + u < staged - 1 ? j0 + u : staged - 1;
                            const int64_t p = first + j, row = c.wrap ? row_mod(p, c.T) : (p < 0 ? 0 : p > c.T - 1 ? c.T - 1 : p);
                            if (row < 0 || row >= c.T) ++outside;
                            held[(size_t)j] = row;
                        }
            }
            for (int thread = 0; thread < pl.block; ++thread) {
                const int lane = thread % kLanes, wave = thread / kLanes;
                const int64_t c0 = (ctile * kLanes + lane) * pl.cols;
                if (c0 >= c.C) continue;
                for (int64_t t = ta + wave; t < tb; t += kWaves) {
                    int64_t p0 = t - c.back, p1 = p0 + c.window;
                    if (!c.wrap) p0 = p0 < 0 ? 0 : p0, p1 = p1 > c.T ? c.T : p1;
                    if (p0 >= p1) ++outside;
                    for (int64_t p = p0; p < p1; ++p) {
                        const int64_t row = c.wrap ? row_mod(p, c.T) : p;
                        if (row < 0 || row >= c.T) ++outside;
                        if (lane == 0 && pl.staged && (p - first < 0 || p - first >= staged || held[(size_t)(p - first)] != row)) ++unstaged;
                    }
                    for (int v = 0; v < pl.cols; ++v) {
                        if (c0 + v >= c.C || t - c.t0 < 0 || t - c.t0 >= c.n_out)
                            ++outside;
                        else
                            ++owned[(size_t)((t - c.t0) * c.C + c0 + v)];
                    }
                }
            }
        }
        int omin = owned[0], omax = owned[0];
        for (int v : owned) omin = v < omin ? v : omin, omax = v > omax ? v : omax;
        printf("cover owned_min=%d owned_max=%d unstaged=%lld outside=%lld lds_rows_max=%lld\nend\n", omin, omax, unstaged, outside, lds_rows_max);
    }
    return 0;
}
