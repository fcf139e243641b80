// Host driver of the grouped launch plans of GridArray.compare(other).groupby(...) (skill_groups_plan in
// scikit-downscale_amd/csrc/sd_skill_plan.h, twosample_groups_plan in sd_twosample_plan.h) for tests/test_skill_groups_plan.py: reads one
// request per line on stdin.  IDS = "n id[0] .. id[n - 1]": the group ids of the T = n rows, or "0" for ids made here (t % G, only
// where T and G allow a table; else the plan gets no table and has to refuse before it reads one).
//   "skill a_f32 b_f32 T C ld_a ld_b G nstat s0 .. s6 ld_out stride_out a_aligned16 b_aligned16 out_aligned16 IDS"
//        -> "error <code> <message>" or "plan cols=.. block=.. ctiles=.. bin_groups=.. blocks=.. bins_per_wave=.. few_groups=..", then
//           (ids given) "rows r[0] .. r[T - 1]" and "offsets o[0] .. o[G]": the tables of groupby_tables the launcher uploads;
//   "cover ..." (the same arguments)
//        -> walks every workgroup, wave and lane of the plan as skill_groups_kernel decodes them and prints "cover min=.. max=..
//           outside=..": how often the least and the most covered (group, cell) is written and how many writes fall outside;
//   "twosample a_f32 b_f32 T C ld_a ld_b G nstat s0 .. s3 width origin ld_out stride_out a_aligned16 b_aligned16 lds_max cu_count IDS"
//        -> "error <code> <message>" or "plan <twosample_describe>", then "rows .." and "offsets .." as above;
//   "sizes ..." (the arguments of twosample with "G n[0] .. n[G - 1]" in place of IDS: the rows of each group; T is their sum)
//        -> the same for ids dealt round-robin to the groups that still lack rows, so that no group is a run of consecutive rows;
//   each answer ends with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sd_skill_plan.h"
#include "sd_twosample_plan.h"

static const int64_t kMostMade = 50000000;  // ids of more rows are not made

static std::vector<int32_t> read_ids(int64_t T, int64_t G, bool* given) {
    int64_t n = 0;
    std::cin >> n;
    *given = n > 0;
    std::vector<int32_t> ids((size_t)n);
    for (int32_t& v : ids) std::cin >> v;
    if (n == 0 && G > 0 && T > 0 && T <= kMostMade)
        for (int64_t t = 0; t < T; ++t) ids.push_back((int32_t)(t % G));
    return ids;
}

static void print_tables(const std::vector<int64_t>& rows, const std::vector<int64_t>& offsets) {
    printf("rows");
    for (int64_t r : rows) printf(" %lld", (long long)r);
    printf("\noffsets");
    for (int64_t o : offsets) printf(" %lld", (long long)o);
    printf("\n");
}

static void skill_request(bool cover) {
    using namespace sdsk;
    SkillCall c;
    int af = 0, bf = 0, aa = 1, ba = 1, oa = 1;
    std::cin >> af >> bf >> c.T >> c.C >> c.ld_a >> c.ld_b >> c.M >> c.nstat;
    for (int& s : c.stats) std::cin >> s;
    std::cin >> c.ld_out >> c.stride_out >> aa >> ba >> oa;
    c.a_is_f32 = af != 0, c.b_is_f32 = bf != 0;
    c.a_aligned16 = aa != 0, c.b_aligned16 = ba != 0, c.out_aligned16 = oa != 0;
    bool given = false;
    const std::vector<int32_t> ids = read_ids(c.T, c.M, &given);
    const SkillGroupsPlan pl = skill_groups_plan(c, ids.empty() ? nullptr : ids.data());
    if (pl.error != SD_OK) {
        printf("error %d %s\nend\n", pl.error, pl.message);
        return;
    }
    if (!cover) {
        printf("plan cols=%d block=%d ctiles=%lld bin_groups=%lld blocks=%lld bins_per_wave=%d few_groups=%lld\n", pl.cols, pl.block,
               (long long)pl.ctiles, (long long)pl.bin_groups, (long long)pl.blocks, pl.bins_per_wave, (long long)sdgb::kFewGroups);
        if (given) {
            std::vector<int64_t> rows((size_t)c.T), offsets((size_t)c.M + 1);
            groupby_tables(ids.data(), c.T, c.M, rows.data(), offsets.data());
            print_tables(rows, offsets);
        }
        printf("end\n");
        return;
    }
    // the decode of skill_groups_kernel (lane_place<V, BPW>): cell tile fastest, then the run of groups; a wave takes bins_per_wave
    // consecutive groups
    std::vector<int> written((size_t)(c.M * c.C), 0);
    long long outside = 0;
    for (int64_t b = 0; b < pl.blocks; ++b) {
        const int64_t ctile = b % pl.ctiles, run = b / pl.ctiles;
        for (int thread = 0; thread < pl.block; ++thread) {
            const int lane = thread % kLanes, wave = thread / kLanes;
            const int64_t c0 = (ctile * kLanes + lane) * pl.cols;
            if (c0 >= c.C) continue;
            const int64_t g0 = run * (kWaves * pl.bins_per_wave) + (int64_t)wave * pl.bins_per_wave;
            for (int k = 0; k < pl.bins_per_wave; ++k) {
                const int64_t g = g0 + k;
                if (g >= c.M) break;
                for (int v = 0; v < pl.cols; ++v) {
                    if (c0 + v >= c.C)
                        ++outside;
                    else
                        ++written[(size_t)(g * c.C + c0 + v)];
                }
            }
        }
    }
    int lo = written[0], hi = written[0];
    for (int v : written) lo = v < lo ? v : lo, hi = v > hi ? v : hi;
    printf("cover min=%d max=%d outside=%lld\nend\n", lo, hi, outside);
}

static void twosample_request(bool by_sizes) {
    TwosampleCall c;
    int af = 0, bf = 0, aa = 1, ba = 1;
    std::cin >> af >> bf >> c.T >> c.C >> c.ld_a >> c.ld_b >> c.M >> c.nstat;
    for (int& s : c.stats) std::cin >> s;
    std::cin >> c.width >> c.origin >> c.ld_out >> c.stride_out >> aa >> ba >> c.lds_max >> c.cu_count;
    c.a_is_f32 = af != 0, c.b_is_f32 = bf != 0;
    c.a_aligned16 = aa != 0, c.b_aligned16 = ba != 0;
    std::vector<int32_t> ids;
    bool print = true;
    if (by_sizes) {
        int64_t G = 0;
        std::cin >> G;
        std::vector<int64_t> left((size_t)G);
        for (int64_t& n : left) std::cin >> n;
        for (bool any = true; any;) {  // one row to every group that still lacks some, again and again
            any = false;
            for (int64_t g = 0; g < G; ++g)
                if (left[(size_t)g] > 0) --left[(size_t)g], ids.push_back((int32_t)g), any = true;
        }
        print = false;
    } else {
        bool given = false;
        ids = read_ids(c.T, c.M, &given);
    }
    std::vector<int64_t> rows, offsets;
    const TwosamplePlan pl = twosample_groups_plan(c, ids.empty() ? nullptr : ids.data(), &rows, &offsets);
    if (pl.error != SD_OK) {
        printf("error %d %s\nend\n", pl.error, pl.message);
        return;
    }
    char buf[512];
    twosample_describe(pl, buf, sizeof buf);
    printf("plan %s\n", buf);
    if (print && c.T <= 4096) print_tables(rows, offsets);
    printf("end\n");
}

int main() {
    std::string word;
    while (std::cin >> word) {
        if (word == "skill" || word == "cover")
            skill_request(word == "cover");
        else
            twosample_request(word == "sizes");
    }
    return 0;
}
