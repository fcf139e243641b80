// What the launch plans of the binned time-axis kernels share (resample_kernel: sd_resample_plan.h, disagg_kernel: sd_disagg_plan.h,
// the groupby kernels: sd_groupby_plan.h),
// as pure host functions (no HIP header: the plan drivers under tests/ compile it with g++ alone).  Both kernels walk a [rows, C]
// field, cells fastest, by bins of consecutive rows that pandas made on the host: a table offsets [M + 1], bin m = rows
// offsets[m] .. offsets[m + 1] - 1; an empty bin has offsets[m] == offsets[m + 1].
//
// bins_plan:      the geometry of such a kernel -- cells per lane, block, cell tiles of kLanes * cols cells by runs of kBinsPerGroup
//                 bins -- with the refusal of a grid that is too large.  The kernels keep nothing in LDS and their grids do not depend
//                 on the CU count.
// check_offsets:  the refusals of the table itself: it starts at 0, never decreases and ends at the rows of the field it cuts, so that
//                 every row a kernel reads or writes lies inside that field.
// fail:           a plan of any kind (an int error and a char message[]) turned into a refusal.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/sd_downscale.h"

namespace sdbn {
constexpr int kLanes = 64;
constexpr int kWaves = 4;         // waves of a workgroup: the same cells, consecutive runs of bins
constexpr int kBinsPerWave = 2;   // whole bins of one wave, one after the other
constexpr int kBatch = 8;         // rows whose loads are in flight before their arithmetic
constexpr int kBinsPerGroup = kWaves * kBinsPerWave;  // bins of a workgroup
constexpr int64_t kGridLimit = (int64_t)1 << 31;

struct BinsPlan {
    int error = SD_OK;  // an error code, with its message: nothing runs
    char message[256] = "";
    int cols = 0;       // adjacent cells of a lane: one load of cols source elements per row, one store of cols doubles per bin or row
    int block = 0;      // threads of a workgroup
    int64_t ctiles = 0;      // cell tiles of kLanes * cols cells
    int64_t bin_groups = 0;  // runs of kBinsPerGroup bins
    int64_t blocks = 0;      // ctiles * bin_groups, cell tile fastest
};

template <class Plan, class... A>
Plan fail(Plan pl, int code, const char* fmt, A... a) {
    snprintf(pl.message, sizeof pl.message, fmt, a...);
    pl.error = code;
    return pl;
}

// C > 0 cells, M > 0 bins; fits(cols): every access of cols adjacent cells of the call is whole and aligned.  Four cells per lane for
// a float32 source, else two, else one: a load of cols source elements and a store of cols doubles are aligned accesses of up to 16
// bytes (four doubles go as two 16-byte halves).
template <class Fits>
BinsPlan bins_plan(const char* who, bool src_is_f32, int64_t C, int64_t M, Fits fits) {
    BinsPlan pl;
    pl.cols = (src_is_f32 && fits(4)) ? 4 : fits(2) ? 2 : 1;
    pl.block = kLanes * kWaves;
    pl.ctiles = (C - 1) / (kLanes * pl.cols) + 1;
    pl.bin_groups = (M - 1) / kBinsPerGroup + 1;
    if (pl.bin_groups > (kGridLimit - 1) / pl.ctiles)  // blocks < 2^31
        return fail(pl, SD_ERR_INVALID, "%s: grid too large", who);
    pl.blocks = pl.ctiles * pl.bin_groups;
    return pl;
}

// offsets [M + 1] of an accepted plan; rows: what the table has to end at, and its name in the message ("T", "Tout")
inline BinsPlan check_offsets(BinsPlan pl, const char* who, const int64_t* offsets, int64_t M, const char* rows_name, int64_t rows) {
    if (pl.error != SD_OK) return pl;
    if (offsets[0] != 0) return fail(pl, SD_ERR_INVALID, "%s: offsets[0] = %lld, expected 0", who, (long long)offsets[0]);
    for (int64_t m = 0; m < M; ++m)
        if (offsets[m + 1] < offsets[m])
            return fail(pl, SD_ERR_INVALID, "%s: offsets decrease at bin %lld (%lld after %lld)", who, (long long)m, (long long)offsets[m + 1],
                        (long long)offsets[m]);
    if (offsets[M] != rows)
        return fail(pl, SD_ERR_INVALID, "%s: offsets[M] = %lld, expected %s = %lld", who, (long long)offsets[M], rows_name, (long long)rows);
    return pl;
}
}  // namespace sdbn
