// Host check of the request row tables of the LDS-DMA kernel (sd_bcsd_plan.h: tmj::build_row_tables) against the chunk layout
// restated here from its description, not from row_of_slot:
//   lane l of a cell's wave owns rows 20 l .. 20 l + 19 of the segment (nl = ceil(m / 20) lanes hold data)
//   chunk l               slot i              row 20 l + i,       i = 0 .. 15
//   chunk nl + t(l)       slot s2(l) + 4 e    row 20 l + 16 + e,  e = 0 .. 3,  t(l) = (l & 7) + 8 (l >> 5), s2(l) = (l >> 3) & 3
//   every other slot (rows past the segment, tail slots of lanes without data, chunks past the tile): the last row, m - 1
// in: lines "m seed"; out: "ok m" or "FAIL m: <what>" per line, then "end"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <random>
#include <vector>

#include "sd_bcsd_plan.h"

using namespace sdfx::tmj;

static std::vector<int> layout(int m) {  // row behind every slot of P
    const int nl = (m + 19) / 20;
    std::vector<int> row((size_t)kTabP, m - 1);
    for (int l = 0; l < nl; ++l) {
        for (int i = 0; i < 16; ++i)
            if (20 * l + i < m) row[(size_t)(16 * l + i)] = 20 * l + i;
        const int t = (l & 7) + 8 * (l >> 5), s2 = (l >> 3) & 3;
        for (int e = 0; e < 4; ++e)
            if (20 * l + 16 + e < m) row[(size_t)(16 * (nl + t) + s2 + 4 * e)] = 20 * l + 16 + e;
    }
    return row;
}

static const char* check(int m, unsigned seed) {
    if (!tab_len_ok(m)) return "length outside the kernel's range";
    static_assert(kTabP == 16 * 96 && kTabW == 8 * 3 * 64 && kTabInts == kTabP + kTabW, "table sizes");
    const std::vector<int> row = layout(m);
    // (a) an injective order table: the tables name rows, so rows can be counted
    std::vector<int32_t> ord((size_t)m), tab((size_t)kTabInts, -1);
    for (int r = 0; r < m; ++r) ord[(size_t)r] = 7 + 3 * r;
    build_row_tables(ord.data(), m, tab.data());
    std::vector<int> seen((size_t)m, 0);
    for (int e = 0; e < kTabP; ++e) {
        if (tab[(size_t)e] != ord[(size_t)row[(size_t)e]]) return "P differs from the layout";
        ++seen[(size_t)((tab[(size_t)e] - 7) / 3)];
    }
    int fillers = 0;
    for (int e = 0; e < kTabP; ++e) fillers += row[(size_t)e] == m - 1;
    for (int r = 0; r + 1 < m; ++r)
        if (seen[(size_t)r] != 1) return "a row of the segment is not in exactly one slot";
    if (seen[(size_t)(m - 1)] != kTabP - (m - 1) || fillers != seen[(size_t)(m - 1)]) return "the other slots do not all hold the last row";
    // (b) a random order table with repeats: P by the layout, W the stated permutation of P, every entry in range
    const int T = 14600;
    std::mt19937 rng(seed);
    for (int r = 0; r < m; ++r) ord[(size_t)r] = (int32_t)(rng() % (unsigned)T);
    tab.assign((size_t)kTabInts, -1);
    build_row_tables(ord.data(), m, tab.data());
    for (int e = 0; e < kTabP; ++e)
        if (tab[(size_t)e] != ord[(size_t)row[(size_t)e]]) return "P differs from the layout (random order)";
    for (int wave = 0; wave < 8; ++wave)
        for (int j = 0; j < 3; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int q = wave + 8 * (4 * j + lane / 16);
                if (q >= kTabChunks) return "W names a chunk past P";
                if (tab[(size_t)(kTabP + (wave * 3 + j) * 64 + lane)] != tab[(size_t)(16 * q + lane % 16)]) return "W is not the stated permutation of P";
            }
    for (int e = 0; e < kTabInts; ++e)
        if (tab[(size_t)e] < 0 || tab[(size_t)e] >= T) return "entry out of range";
    // (c) row_of_slot itself, which the kernel without tables evaluates, against the layout
    for (int Q = 0; Q < kTabChunks; ++Q)
        for (int S = 0; S < 16; ++S)
            if (row_of_slot(Q, S, lanes_of(m), m) != row[(size_t)(16 * Q + S)]) return "row_of_slot differs from the layout";
    return nullptr;
}

int main() {
    int m;
    unsigned seed;
    while (std::cin >> m >> seed) {
        const char* what = check(m, seed);
        if (what) printf("FAIL %d: %s\n", m, what);
        else printf("ok %d\n", m);
    }
    printf("end\n");
    return 0;
}
