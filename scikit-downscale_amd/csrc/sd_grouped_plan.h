// Host-side plan of a grouped (day-of-year window) regression, as pure host functions (no HIP header: a g++ test can compile
// them alone).  sd_grouped.hip builds its tables and picks the tile of its window kernel from it.
//
// Input: one key per time step, key[t] in [0, n), shared by all cells, and the half width `window` of the circular window:
// group g is fitted on the samples whose key lies in {g - window .. g + window} (mod n), every key once
// (grouping.py:106-138 of the reference: a boolean membership table, so 2 * window + 1 > n is every key once).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sd_downscale.h"

// time steps ordered by (key, time) + offsets: a stable counting sort
struct GroupedKeyTable {
    int err = SD_OK;
    std::string msg;
    std::vector<int32_t> order;  // [T]
    std::vector<int64_t> off;    // [n+1]
    std::vector<double> cnt;     // [n] samples of each key
    int first_bad = -1;          // smallest key outside [0, n) (err != SD_OK)
};

static inline GroupedKeyTable grouped_key_table(const int32_t* key, int64_t T, int n) {
    GroupedKeyTable p;
    p.off.assign((size_t)n + 1, 0);
    bool bad = false;
    int32_t worst = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int32_t k = key[t];
        if (k < 0 || k >= n) {
            worst = bad ? std::min(worst, k) : k;
            bad = true;
        } else {
            ++p.off[(size_t)k + 1];
        }
    }
    if (bad) {
        p.err = SD_ERR_INVALID;
        p.first_bad = worst;
        p.msg = "key " + std::to_string(worst) + " outside [0, " + std::to_string(n) + ")";
        return p;
    }
    p.cnt.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        p.cnt[(size_t)k] = (double)p.off[(size_t)k + 1];
        p.off[(size_t)k + 1] += p.off[(size_t)k];
    }
    p.order.resize((size_t)T);
    std::vector<int64_t> at(p.off.begin(), p.off.end() - 1);
    for (int64_t t = 0; t < T; ++t) p.order[(size_t)at[(size_t)key[t]]++] = (int32_t)t;
    return p;
}

// statistics per (cell, key) besides the count (shared by all cells): sum x_f, sum y, sum x_f x_g (g >= f), sum x_f y
static inline int grouped_nstat(int F) { return F + 1 + F * (F + 1) / 2 + F; }

// distinct keys of one window
static inline int grouped_window_keys(int n, int window) { return std::min(2 * window + 1, n); }

// group g is fitted when its window holds a sample
static inline std::vector<int32_t> grouped_fitted(const std::vector<double>& cnt, int window) {
    const int n = (int)cnt.size(), W = grouped_window_keys(n, window);
    std::vector<int32_t> fitted((size_t)n);
    for (int g = 0; g < n; ++g) {
        double c = 0.0;
        for (int j = 0; j < W; ++j) c += cnt[(size_t)(((g - window + j) % n + n) % n)];
        fitted[(size_t)g] = c > 0.0 ? 1 : 0;
    }
    return fitted;
}

// Tile of the window kernel: a workgroup of kGroupedThreads threads owns `cells` adjacent cells and a run of `run` consecutive
// groups; the statistics of the run's `slots` = min(run + 2 * window, n) keys are staged in LDS once (slots * nstat * cells
// doubles) and every group re-adds its window from there, so a key's statistics are fetched slots / run times.  Fewer cells
// per workgroup leave room for more keys (F = 8 holds 53 doubles per (cell, key)); the table is then read in shorter row
// fragments, which is the cheaper side of the trade: the table is n / T of the input.  A run is not made longer than
// 4 * window groups (fetch factor 1.5): the grid needs workgroups too.  The first choice stays within 64 KB so that two
// workgroups share a compute unit; the whole LDS is used when no tile fits otherwise.
constexpr int kGroupedThreads = 256;

struct GroupedWindowTile {
    int cells = 0, run = 0, slots = 0;  // cells == 0: the window does not fit in LDS
    size_t lds = 0;
};

static inline GroupedWindowTile grouped_window_tile(int F, int n, int window, size_t lds_max) {
    const int nstat = grouped_nstat(F);
    GroupedWindowTile best;
    double best_fetch = 0.0;
    const size_t budgets[2] = {std::min<size_t>(lds_max, (size_t)64 << 10), lds_max};
    for (size_t budget : budgets) {
        for (int cells = 64; cells >= 1; cells /= 2) {
            const size_t per_key = sizeof(double) * (size_t)nstat * cells;
            const int cap = (int)std::min<size_t>(budget / per_key, (size_t)n);
            int run = cap >= n ? n : cap - 2 * window;
            if (run < 1) continue;
            run = std::min(run, std::max(4 * window, kGroupedThreads / cells));
            GroupedWindowTile t;
            t.cells = cells;
            t.run = run;
            t.slots = std::min(run + 2 * window, n);
            t.lds = per_key * (size_t)t.slots;
            const double fetch = (double)t.slots / run;
            if (best.cells == 0 || fetch < 0.75 * best_fetch) {  // halve the row fragment only for a clear gain
                best = t;
                best_fetch = fetch;
            }
            if (best_fetch <= 2.0) return best;
        }
        if (best.cells != 0) return best;
    }
    return best;
}
