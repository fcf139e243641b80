// Day-window plan of a ZScoreRegressor fit (zscore.py:123-189 of the reference), as a pure host function (no HIP header:
// tests/zscore_plan_check.cpp compiles it with g++ alone).  sd_zscore.hip builds its tables from it.
//
// Input: per sample its day index d in [0, D) (the position of its day of year in the sorted union of the days that occur) and
// its year.  The reference pivots the samples into a [day, year] grid M (missing where a year lacks a day), then builds the
// extended day axis R = M[-ceil(w/2):] ++ M ++ M[:w/2] (Python slices, clipped to D), takes the centred window of width w at
// every position p of R -- R[p - w/2 .. p + (w-1)/2], positions outside R missing -- and keeps the positions n .. L-n-1,
// n = w/2 + 1.  A kept window never reaches outside R (p - w/2 >= 1 and p + (w-1)/2 <= L - 2), so each one is the multiset of
// the w days at its R positions; a day that occurs twice in it (D < w) counts twice.  The statistics of a window are those of
// every sample of its days, so per-day partial statistics merged over the window's days give them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sd_downscale.h"

struct ZscorePlan {
    int err = SD_OK;
    std::string msg;
    int D = 0, w = 0;
    int L = 0;                    // length of R
    int n = 0;                    // w/2 + 1: kept positions are n .. L-n-1
    int K = 0;                    // kept windows
    std::vector<int32_t> rday;    // [L] day index of every R position
    std::vector<int32_t> label;   // [K] day index of every kept position (its label is that day's day of year)
    std::vector<int32_t> win;     // [K][w] day indices of every kept window, in R order
    std::vector<int64_t> cnt;     // [D] samples of each day (years that have it)
    std::vector<int32_t> order;   // [T] sample indices ordered by (day, time)
    std::vector<int64_t> off;     // [D+1] offsets of the days in `order`
    int nmax = 0;                 // most samples of one day
};

static inline ZscorePlan zscore_plan_error(int code, std::string msg) {
    ZscorePlan p;
    p.err = code;
    p.msg = std::move(msg);
    return p;
}

static inline ZscorePlan zscore_plan(const int32_t* day_idx, const int32_t* year, int64_t T, int D, int w) {
    char buf[160];
    if (w <= 0) {
        snprintf(buf, sizeof buf, "window_width must be positive, got %d", w);
        return zscore_plan_error(SD_ERR_INVALID, buf);
    }
    if (T < 1 || D < 1 || day_idx == nullptr || year == nullptr) return zscore_plan_error(SD_ERR_INVALID, "zscore plan: bad sizes");
    ZscorePlan p;
    p.D = D;
    p.w = w;
    p.cnt.assign(D, 0);
    for (int64_t t = 0; t < T; ++t) {
        if (day_idx[t] < 0 || day_idx[t] >= D) {
            snprintf(buf, sizeof buf, "day_idx[%lld] = %d outside [0,%d)", (long long)t, day_idx[t], D);
            return zscore_plan_error(SD_ERR_INVALID, buf);
        }
        p.cnt[day_idx[t]]++;
    }
    for (int d = 0; d < D; ++d)
        if (p.cnt[d] == 0) {
            snprintf(buf, sizeof buf, "day %d of [0,%d) has no sample: D must be the number of distinct days", d, D);
            return zscore_plan_error(SD_ERR_INVALID, buf);
        }
    // two samples on one (year, day) cell of M: the reference's alignment of the yearly groups fails (sub-daily data)
    std::vector<std::pair<int32_t, int32_t>> yd((size_t)T);
    for (int64_t t = 0; t < T; ++t) yd[t] = {year[t], day_idx[t]};
    std::sort(yd.begin(), yd.end());
    for (int64_t t = 1; t < T; ++t)
        if (yd[t] == yd[t - 1]) {
            snprintf(buf, sizeof buf, "two samples fall on day index %d of year %d: the day-of-year grid needs at most one sample per day",
                     yd[t].second, yd[t].first);
            return zscore_plan_error(SD_ERR_INVALID, buf);
        }
    // R = M[-ceil(w/2):] ++ M ++ M[:w/2]
    const int late = std::min((w + 1) / 2, D), early = std::min(w / 2, D);
    for (int i = D - late; i < D; ++i) p.rday.push_back(i);
    for (int i = 0; i < D; ++i) p.rday.push_back(i);
    for (int i = 0; i < early; ++i) p.rday.push_back(i);
    p.L = (int)p.rday.size();
    p.n = w / 2 + 1;
    p.K = std::max(p.L - 2 * p.n, 0);
    for (int k = 0; k < p.K; ++k) {
        const int pos = p.n + k;
        p.label.push_back(p.rday[pos]);
        for (int j = pos - w / 2; j <= pos + (w - 1) / 2; ++j) p.win.push_back(p.rday[j]);  // inside R: see the header comment
    }
    if (p.K == 0) {  // (the reference keeps an empty series here, and every predict then fails in its expansion)
        snprintf(buf, sizeof buf, "no day window is kept: %d distinct days are too few for window_width %d", D, w);
        return zscore_plan_error(SD_ERR_UNSUPPORTED, buf);
    }
    p.off.assign(D + 1, 0);
    for (int d = 0; d < D; ++d) {
        p.off[d + 1] = p.off[d] + p.cnt[d];
        p.nmax = std::max<int>(p.nmax, (int)p.cnt[d]);
    }
    p.order.resize((size_t)T);
    std::vector<int64_t> cur(p.off.begin(), p.off.end() - 1);
    for (int64_t t = 0; t < T; ++t) p.order[cur[day_idx[t]]++] = (int32_t)t;
    return p;
}

// Positional expansion of the fitted parameters over a predict series of Tp samples (zscore.py:273-319): sample t takes
// entry t % min(Tp, 364); the reference's .iloc fails when that reaches past the K fitted entries.
static inline int zscore_expand_period(int64_t Tp) { return (int)std::min<int64_t>(Tp, 364); }
static inline bool zscore_expand_ok(int64_t Tp, int K) { return zscore_expand_period(Tp) <= K; }
