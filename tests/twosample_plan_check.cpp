// Host driver of the two-sample launch plan (scikit-downscale_amd/csrc/sd_twosample_plan.h) for tests/test_twosample_plan.py: reads one
// request per line on stdin.  CALL = "a_f32 b_f32 T C ld_a ld_b M nstat s0 s1 s2 s3 width origin ld_out stride_out a_aligned16
// b_aligned16 lds_max cu_count" (width and origin as strtod reads them: "nan" and "inf" are numbers here).
//   "plan CALL"    the table is made here: offsets[m] = m * T / M
//        -> "error <code> <message>" or "plan path=.. n_max=.. K=.. rs=.. lds=.. per_cu=.. ntiles=.. blocks=.. vec_a=.. vec_b=.. chunks=..
//           run_slots=.. np_max=.. select_lds=.. select_blocks=.." and the words of twosample_describe on a second line;
//   "tables CALL o[0] .. o[M]"
//        -> the same, with the table of the request;
//   "widths"  (no CALL) -> "widths K:lds:per_cu ..." of every segment width on a 160 KB CU;
//   each answer ends with "end".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "sd_twosample_plan.h"

static TwosampleCall read_call() {
    TwosampleCall c;
    int af = 0, bf = 0, aa = 1, ba = 1;
    long long lds = 0;
    std::string width, origin;
    std::cin >> af >> bf >> c.T >> c.C >> c.ld_a >> c.ld_b >> c.M >> c.nstat;
    for (int& s : c.stats) std::cin >> s;
    std::cin >> width >> origin >> c.ld_out >> c.stride_out >> aa >> ba >> lds >> c.cu_count;
    c.width = strtod(width.c_str(), nullptr), c.origin = strtod(origin.c_str(), nullptr);
    c.a_is_f32 = af != 0, c.b_is_f32 = bf != 0;
    c.a_aligned16 = aa != 0, c.b_aligned16 = ba != 0;
    c.lds_max = (size_t)lds;
    return c;
}

int main() {
    const int64_t kMostMade = 50000000;  // tables longer than this are not made: the plan has to refuse before it reads them
    std::string word;
    while (std::cin >> word) {
        if (word == "widths") {
            printf("widths");
            for (int K : sdts::kSegWidths) printf(" %d:%zu:%d", K, sdts::seg_lds_bytes(K), sdqt::per_cu(sdts::seg_lds_bytes(K), 160 * 1024, sdw::kThreads));
            printf("\nend\n");
            continue;
        }
        const TwosampleCall c = read_call();
        std::vector<int64_t> off;
        if (word == "tables") {
            off.resize((size_t)(c.M > 0 ? c.M + 1 : 0));
            for (int64_t& v : off) std::cin >> v;
        } else if (c.M > 0 && c.M <= kMostMade && c.T > 0) {
            for (int64_t m = 0; m <= c.M; ++m) off.push_back((int64_t)((__int128)m * c.T / c.M));
        }
        const TwosamplePlan pl = twosample_plan(c, off.empty() ? nullptr : off.data());
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        char words[512];
        twosample_describe(pl, words, sizeof words);
        printf("plan path=%d n_max=%lld K=%d rs=%d lds=%zu per_cu=%d ntiles=%lld blocks=%lld vec_a=%d vec_b=%d chunks=%lld run_slots=%lld np_max=%d "
               "select_lds=%zu select_blocks=%lld\n%s\nend\n",
               pl.path, (long long)pl.n_max, pl.K, pl.rs, pl.lds, pl.per_cu, (long long)pl.ntiles, (long long)pl.blocks, (int)pl.vec_a, (int)pl.vec_b,
               (long long)pl.chunks, (long long)pl.run_slots, pl.np_max, pl.select_lds, (long long)pl.select_blocks, words);
    }
    return 0;
}
