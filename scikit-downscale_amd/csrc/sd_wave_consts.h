// Workgroup shape and LDS layout constants of the BCSD register-sort kernels (sd_wave.h), kept free of HIP headers so that the
// host-only launch plan (sd_bcsd_plan.h) can size its launches from them.
#pragma once

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

}  // namespace sdw
