// Workgroup shape and LDS layout constants of the BCSD register-sort kernels (sd_wave.h) and the sizing of the sorts the analog and
// quantile-mapping families share, kept free of HIP headers so that the host-only launch plans (sd_bcsd_plan.h, sd_analog_plan.h,
// sd_qm_plan.h) can size their launches from them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdw {

constexpr int kWave = 64;
constexpr int kW = 8;          // cells per workgroup
constexpr int kThreads = 512;  // 8 waves
constexpr int kRowsPerPass = kThreads / 4;  // 4 lanes (16 B each) cover the 8 cells of one row
// LDS layout of a workgroup: [column-sum exchange: 64 doubles][1/c table: 16][per-cell flags: 8][tile: kW rows of RS].
// The small areas come first so that no row starts at LDS address 0: the searches keep "address of element - 1"
// positions and compare them as unsigned numbers.
constexpr int kHeadDoubles = 64 + 16 + 8;
// zero slots in front of a time-ordered segment in its LDS row (the rolling windows, sd_wave.h: zero_pads)
constexpr int kPadFront = 4;

// ---- sizing of the sorts the families share (analog and quantile mapping; one definition each) ------------------------------
// workgroup merge sort of sd_sortnet.h on 1 024 threads: np + 1 keys and nthr + 1 co-ranks
inline size_t block_sort_lds_bytes(int np) { return sizeof(double) * (size_t)(np + 1) + sizeof(int) * 1025; }
// tile-shaped sorts (analog_tile_sort_kernel<K>, qm_tile_runs_kernel<K>): runs of 64 * K keys; row stride >= 64 * K + 1 slots with
// RS % 4 == 2, LDS, chunks of a series and its padded length (slots of presorted runs per cell)
constexpr int tile_sort_rs(int K) { return kWave * K + 2 + ((4 - (kWave * K + 2) % 4) + 2) % 4; }
inline size_t tile_sort_lds_bytes(int K) { return sizeof(double) * ((size_t)kW * tile_sort_rs(K) + kHeadDoubles); }
inline int64_t tile_sort_chunks(int K, int64_t T) { return (T + kWave * K - 1) / (kWave * (int64_t)K); }
inline int tile_sort_np(int K, int64_t T) { return (int)(tile_sort_chunks(K, T) * kWave * K); }
// workgroups of the kernels tiled like the BCSD ones: 8 per 8 tiles of 8 cells and row block
inline int64_t tiled_blocks(int64_t C, int64_t rows) {
    const int64_t ntiles = (C + kW - 1) / kW, tx = (ntiles + 7) / 8;
    return 8 * tx * rows;
}

}  // namespace sdw
