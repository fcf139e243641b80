// Host check of the searched K = 20 tables of the register wave sort (csrc/sd_wsort_nets20.h through csrc/sd_wsort.h):
//   * SortNet<20> sorts all 2^20 0-1 inputs (0-1 principle; 64 inputs per word: min = and, max = or);
//   * BitonicNet<20> sorts all 382 cyclic-bitonic 0-1 inputs of length 20, the contract its comment states;
//   * cost in vector instructions (compare-exchange 2, 3-sorter 3): sorter <= 142, merger <= 75, and what the generated header
//     says about itself; dependency depth, for the record;
//   * every operation names distinct registers below 20, minimum to the lowest index (a sorted lane stays sorted);
//   * a sorter with 3-sorters (inline assembly the compiler's hazard recognizer does not see) is followed by the fence before
//     the DPP reads of merge level 1: the constants wave_sort and dpp_fence are keyed off.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "sd_wsort.h"

using sdws::CmpList;

static constexpr int K = 20;
static constexpr sdws::SortNet<K> snet{};
static constexpr sdws::BitonicNet<K> bnet{};

constexpr int cost(const CmpList& c) {
    int n = 0;
    for (int i = 0; i < c.n; ++i) n += c.c[i] == sdws::kNone ? 2 : 3;
    return n;
}
constexpr int depth(const CmpList& c) {
    int d[K] = {}, top = 0;
    for (int i = 0; i < c.n; ++i) {
        const int r[3] = {c.a[i], c.b[i], c.c[i]};
        int t = 0;
        for (int j = 0; j < 3; ++j)
            if (r[j] != sdws::kNone && d[r[j]] > t) t = d[r[j]];
        for (int j = 0; j < 3; ++j)
            if (r[j] != sdws::kNone) d[r[j]] = t + 1;
        top = t + 1 > top ? t + 1 : top;
    }
    return top;
}
constexpr bool well_formed(const CmpList& c) {
    for (int i = 0; i < c.n; ++i) {
        if (c.a[i] >= c.b[i] || c.b[i] >= K) return false;
        if (c.c[i] != sdws::kNone && (c.b[i] >= c.c[i] || c.c[i] >= K)) return false;
    }
    return true;
}

static_assert(sdws::kSearchedNets20, "this check is about the searched tables");
static_assert(cost(snet.c) <= 142, "SortNet<20>: at most 142 vector instructions");
static_assert(cost(bnet.c) <= 75, "BitonicNet<20>: at most 75 vector instructions");
static_assert(cost(snet.c) == sdws::kSortNet20Cost && cost(bnet.c) == sdws::kBitonicNet20Cost, "the generated header's own figures");
static_assert(well_formed(snet.c) && well_formed(bnet.c), "registers a < b < c < 20");
// the DPP hazard: a sorter with 3-sorters is fenced before merge level 1, and dpp_fence emits its s_nop for this K
static_assert(sdws::kFenceAfterSorter<K> == sdws::uses_sort3(snet.c), "wave_sort fences behind a sorter with 3-sorters");
static_assert(!sdws::uses_sort3(snet.c) || sdws::kDppFence<K>, "dpp_fence<20> must not be a no-op behind the sorter");
static_assert(!sdws::uses_sort3(bnet.c) || sdws::kDppFence<K>, "dpp_fence<20> must not be a no-op behind the merger");
// every other width keeps its construction: no 3-sorter in a Batcher sorter, so no fence (and no code change) there
static_assert(!sdws::kFenceAfterSorter<12> && !sdws::kFenceAfterSorter<16> && !sdws::kFenceAfterSorter<24>, "other widths unchanged");

static void apply(const CmpList& c, uint64_t* v) {
    for (int i = 0; i < c.n; ++i) {
        if (c.c[i] == sdws::kNone) {
            const uint64_t a = v[c.a[i]], b = v[c.b[i]];
            v[c.a[i]] = a & b;
            v[c.b[i]] = a | b;
        } else {
            const uint64_t x = v[c.a[i]], y = v[c.b[i]], z = v[c.c[i]];
            v[c.a[i]] = x & y & z;
            v[c.b[i]] = (x & y) | ((x | y) & z);
            v[c.c[i]] = x | y | z;
        }
    }
}

static long unsorted(const uint64_t* v) {
    uint64_t bad = 0;
    for (int i = 0; i + 1 < K; ++i) bad |= v[i] & ~v[i + 1];  // a one in front of a zero
    return __builtin_popcountll(bad);
}

int main() {
    long bad_sorter = 0, bad_merger = 0;
    // all 2^20 inputs: word w holds the inputs 64 w .. 64 w + 63; bit i of an input's number is key i
    for (uint64_t w = 0; w < (1u << K) / 64; ++w) {
        uint64_t v[K];
        for (int i = 0; i < K; ++i) {
            v[i] = 0;
            for (int t = 0; t < 64; ++t) v[i] |= (uint64_t)(((w * 64 + t) >> i) & 1) << t;
        }
        apply(snet.c, v);
        bad_sorter += unsorted(v);
    }
    // cyclic-bitonic 0-1 inputs: one run of ones anywhere on the ring, and the complements
    std::set<uint32_t> seqs;
    for (int start = 0; start < K; ++start)
        for (int len = 0; len <= K; ++len) {
            uint32_t s = 0;
            for (int t = 0; t < len; ++t) s |= 1u << ((start + t) % K);
            seqs.insert(s);
            seqs.insert(~s & ((1u << K) - 1));
        }
    const std::vector<uint32_t> all(seqs.begin(), seqs.end());
    for (size_t lo = 0; lo < all.size(); lo += 64) {
        uint64_t v[K] = {};
        for (size_t t = 0; t < 64 && lo + t < all.size(); ++t)
            for (int i = 0; i < K; ++i) v[i] |= (uint64_t)((all[lo + t] >> i) & 1) << t;
        apply(bnet.c, v);
        bad_merger += unsorted(v);
    }
    std::printf("SortNet<20>: %d instructions in %d operations, depth %d, %ld inputs: %s\n", cost(snet.c), snet.c.n, depth(snet.c), 1l << K, bad_sorter ? "FAILED" : "ok");
    std::printf("BitonicNet<20>: %d instructions in %d operations, depth %d, %zu cyclic-bitonic inputs: %s\n", cost(bnet.c), bnet.c.n, depth(bnet.c), all.size(),
                bad_merger || all.size() != 382 ? "FAILED" : "ok");
    std::printf("local part of one sort: %d instructions\n", cost(snet.c) + 6 * cost(bnet.c));
    return bad_sorter || bad_merger || all.size() != 382;
}
