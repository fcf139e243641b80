// Host check of the issue order the register wave sort uses for its merge levels 4 .. 6 (csrc/sd_wsort.h, LevelSched): the op
// lists the kernels execute are run here on a model of the 64 lanes x K registers and compared with the stage-by-stage form.
//   * dataflow: every fetch reads its register after the write of the stage before and before the write of its own stage (in all
//     lanes at once: a fetch is one wave-wide instruction), and every med3 consumes the fetch of its own stage and register;
//   * every 0-1 input of a merge level (two sorted runs of M lanes, any numbers of zeros), through the level before it, whose
//     merger issues the first fetches: sorted, and equal to the stage-by-stage form;
//   * random 32-bit keys with duplicates and pads through the whole sort: the same registers as the stage-by-stage form.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sd_wsort.h"

using sdws::CmpList;
using sdws::SchedOp;

// ---- the value model: T = unsigned (keys) or uint64_t (64 independent 0-1 cases, one per bit: min = and, max = or) ----
struct KeyOps {
    typedef unsigned T;
    static T lo(T a, T b) { return std::min(a, b); }
    static T hi(T a, T b) { return std::max(a, b); }
};
struct BitOps {
    typedef uint64_t T;
    static T lo(T a, T b) { return a & b; }
    static T hi(T a, T b) { return a | b; }
};

template <typename O>
static void net_op(const CmpList& c, int i, typename O::T* v) {
    typedef typename O::T T;
    if (c.c[i] == sdws::kNone) {
        const T a = v[c.a[i]], b = v[c.b[i]];
        v[c.a[i]] = O::lo(a, b);
        v[c.b[i]] = O::hi(a, b);
    } else {
        const T x = v[c.a[i]], y = v[c.b[i]], z = v[c.c[i]];
        v[c.a[i]] = O::lo(O::lo(x, y), z);
        v[c.b[i]] = O::hi(O::lo(x, y), O::lo(O::hi(x, y), z));
        v[c.c[i]] = O::hi(O::hi(x, y), z);
    }
}

template <typename O, int K>
struct Wave {
    typedef typename O::T T;
    T k[64][K];
    T t[64][2 * K];
};

// the stage-by-stage form, written independently of the header's device code
template <typename O, int K>
static void serial_stage(Wave<O, K>& w, int X, int bit, bool rev) {
    static typename O::T old[64][K];
    std::copy(&w.k[0][0], &w.k[0][0] + 64 * K, &old[0][0]);
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < K; ++i) {
            const typename O::T a = old[l][i], b = old[l ^ X][rev ? K - 1 - i : i];
            w.k[l][i] = ((l >> bit) & 1) ? O::hi(a, b) : O::lo(a, b);
        }
}
template <typename O, int K>
static void serial_level(Wave<O, K>& w, int L) {
    static const sdws::BitonicNet<K> bnet{};
    const int M = 1 << (L - 1);
    serial_stage<O, K>(w, 2 * M - 1, L - 1, true);
    for (int h = M / 2, b = L - 2; h >= 1; h >>= 1, --b) serial_stage<O, K>(w, h, b, false);
    for (int l = 0; l < 64; ++l)
        for (int c = 0; c < bnet.c.n; ++c) net_op<O>(bnet.c, c, w.k[l]);
}

// one op list, op by op over all lanes (an instruction is wave-wide)
template <typename O, int K, typename S>
static void run_list(Wave<O, K>& w, const S& s, bool next) {
    static const sdws::BitonicNet<K> bnet{};
    typename O::T f[64];
    for (int o = 0; o < s.n; ++o) {
        const SchedOp& op = s.op[o];
        switch (op.kind) {
            case sdws::kOpFetchNext:
                if (!next) break;
                // fall through
            case sdws::kOpFetch:
                for (int l = 0; l < 64; ++l) f[l] = w.k[l ^ op.c][op.a];
                for (int l = 0; l < 64; ++l) w.t[l][op.b] = f[l];
                break;
            case sdws::kOpMed:
                for (int l = 0; l < 64; ++l)
                    w.k[l][op.a] = ((l >> op.c) & 1) ? O::hi(w.k[l][op.a], w.t[l][op.b]) : O::lo(w.k[l][op.a], w.t[l][op.b]);
                break;
            case sdws::kOpNet:
                for (int l = 0; l < 64; ++l) net_op<O>(bnet.c, op.a, w.k[l]);
                break;
            default: break;
        }
    }
}

// wave_sort's levels 4 .. 6 as the header chains them
template <typename O, int K, bool P>
static void piped_levels(Wave<O, K>& w, int lanes_used) {
    static const sdws::LevelSched<K, 4, false, P> s4{};
    static const sdws::LevelSched<K, 5, P, P> s5{};
    static const sdws::LevelSched<K, 6, P, false> s6{};
    if (lanes_used > 8) {
        const bool l5 = lanes_used > 16, l6 = lanes_used > 32;
        run_list<O, K>(w, s4, l5);
        if (l5) {
            run_list<O, K>(w, s5, l6);
            if (l6) run_list<O, K>(w, s6, false);
        }
    }
}

// the sort up to level 3, the same in both forms, then the levels 4 .. 6 in either form
template <int K>
static void sort_front(Wave<KeyOps, K>& w, int lanes_used) {
    static const sdws::SortNet<K> snet{};
    for (int l = 0; l < 64; ++l)
        for (int c = 0; c < snet.c.n; ++c) net_op<KeyOps>(snet.c, c, w.k[l]);
    for (int L = 1; L <= 3; ++L)
        if (lanes_used > (1 << (L - 1))) serial_level<KeyOps, K>(w, L);
}
template <int K>
static void serial_levels(Wave<KeyOps, K>& w, int lanes_used) {
    for (int L = 4; L <= 6; ++L)
        if (lanes_used > (1 << (L - 1))) serial_level<KeyOps, K>(w, L);
}

// ---- dataflow of the lists: versions of the key registers (number of writes by cross-lane stages in the current level) ----
template <int K>
struct Flow {
    int ver[K] = {};              // med3 writes so far in this level
    int net_seen[K] = {};         // merger operations that touched the register so far
    int t_reg[2 * K], t_ver[2 * K], t_x[2 * K], t_net[2 * K];
    Flow() { std::fill(t_reg, t_reg + 2 * K, -1); }
};

template <int K, int L, typename S>
static int check_flow(const S& s, Flow<K>& fl, bool pre, bool next) {
    static const sdws::BitonicNet<K> bnet{};
    int bad = 0;
    const int M = 1 << (L - 1);
    int xs[6], bits[6], S_ = 0;
    xs[S_] = 2 * M - 1, bits[S_] = L - 1, ++S_;
    for (int h = M / 2, b = L - 2; h >= 1; h >>= 1, --b) xs[S_] = h, bits[S_] = b, ++S_;
    int net_total[K] = {};
    for (int c = 0; c < bnet.c.n; ++c) {
        ++net_total[bnet.c.a[c]], ++net_total[bnet.c.b[c]];
        if (bnet.c.c[c] != sdws::kNone) ++net_total[bnet.c.c[c]];
    }
    if (!pre) std::fill(fl.t_reg, fl.t_reg + 2 * K, -1);
    std::fill(fl.ver, fl.ver + K, 0);
    std::fill(fl.net_seen, fl.net_seen + K, 0);
    int first_med = -1, last_fetch0 = -1, net_next = 0;
    for (int o = 0; o < s.n; ++o) {
        const SchedOp& op = s.op[o];
        if (op.kind == sdws::kOpFetch) {
            // reads register a as stage ver[a] left it: the fetch of stage v comes after the write of stage v-1 and before the
            // write of stage v, and before the merger
            bad += op.a >= K || op.b >= 2 * K || fl.ver[op.a] >= S_ || op.c != xs[fl.ver[op.a]] || fl.net_seen[op.a] != 0;
            fl.t_reg[op.b] = op.a, fl.t_ver[op.b] = fl.ver[op.a], fl.t_x[op.b] = op.c, fl.t_net[op.b] = 0;
            if (fl.ver[op.a] == 0) last_fetch0 = o;
        } else if (op.kind == sdws::kOpFetchNext) {
            // reads a register the merger has finished, for stage 0 of the next level
            if (!next) continue;  // not executed
            bad += op.a >= K || fl.ver[op.a] != S_ || fl.net_seen[op.a] != net_total[op.a] || op.c != 4 * M - 1 || op.b != K + op.a;
            fl.t_reg[op.b] = op.a, fl.t_ver[op.b] = -1, fl.t_x[op.b] = op.c, fl.t_net[op.b] = 1;
        } else if (op.kind == sdws::kOpMed) {
            const int v = fl.ver[op.a];
            const int want = v == 0 ? K - 1 - op.a : op.a;
            bad += v >= S_ || op.c != bits[v] || fl.net_seen[op.a] != 0;
            // the temporary holds the partner register of this very stage
            bad += fl.t_reg[op.b] != want || fl.t_x[op.b] != xs[v];
            if (v == 0 && pre) bad += fl.t_ver[op.b] != -1;  // fetched from the finished register of the level before
            else bad += fl.t_ver[op.b] != v || fl.t_net[op.b] != 0;
            if (v == 0 && first_med < 0) first_med = o;
            fl.t_reg[op.b] = -1;  // consumed once
            ++fl.ver[op.a];
        } else if (op.kind == sdws::kOpNet) {
            bad += op.a != net_next++;  // the merger's operations in their own order
            const int r[3] = {bnet.c.a[op.a], bnet.c.b[op.a], bnet.c.c[op.a]};
            for (int j = 0; j < 3; ++j)
                if (r[j] != sdws::kNone) {
                    bad += fl.ver[r[j]] != S_;  // all stages done
                    ++fl.net_seen[r[j]];
                }
        }
    }
    bad += net_next != bnet.c.n;
    for (int i = 0; i < K; ++i) bad += fl.ver[i] != S_;
    // a med3 of stage 0 overwrites a register the partner lane fetches in stage 0: all those fetches come first
    if (!pre) bad += !(last_fetch0 < first_med);
    // with NEXT every register has been fetched for the next level, and only then
    for (int i = 0; i < K; ++i) bad += next != (fl.t_reg[K + i] == i && fl.t_ver[K + i] == -1);
    return bad;
}

// ---- every 0-1 input of level L: two sorted runs of M lanes with z1 and z2 zeros; 64 cases per word, 64 / (2M) pairs per wave ----
template <int K, int L, bool P>
static long zero_one(bool l5, bool l6, int& bad) {
    static Wave<BitOps, K> a;
    static const sdws::LevelSched<K, 4, false, P> s4{};
    static const sdws::LevelSched<K, 5, P, P> s5{};
    static const sdws::LevelSched<K, 6, P, false> s6{};
    const int M = 1 << (L - 1), pairs = 64 / (2 * M), run = M * K;
    // a word holds 64 cases: one z1 for all of them, z2 = 64 c + bit (a z2 beyond the run is the run of zeros once more)
    const int chunks = run / 64 + 1;
    const long total = (long)(run + 1) * chunks;
    long done = 0;
    while (done < total) {
        for (int p = 0; p < pairs; ++p) {
            const long unit = std::min(done + p, total - 1);
            const int z1 = (int)(unit / chunks), c = (int)(unit % chunks);
            for (int j = 0; j < run; ++j) {
                const int d = j - 64 * c;
                a.k[p * 2 * M + j / K][j % K] = j >= z1 ? ~0ull : 0ull;
                a.k[p * 2 * M + M + j / K][j % K] = d < 0 ? 0ull : d >= 63 ? ~0ull : (2ull << d) - 1;
            }
        }
        // the list of the level before runs first on the sorted runs (it leaves them as they are) and issues the first fetches
        if (L == 4) run_list<BitOps, K>(a, s4, false);
        if (L == 5) run_list<BitOps, K>(a, s4, true), run_list<BitOps, K>(a, s5, l6);
        if (L == 6) run_list<BitOps, K>(a, s4, true), run_list<BitOps, K>(a, s5, true), run_list<BitOps, K>(a, s6, false);
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < K; ++i) {
                // sorted inside every run of 2M lanes (never a one in front of a zero): for 0-1 keys that is the result of the
                // stage-by-stage form, whose networks tests/wsort_nets_check.cpp proves
                const int pos = l * K + i;
                if (pos % (2 * M * K) != 0) {
                    const uint64_t prev = i ? a.k[l][i - 1] : a.k[l - 1][K - 1];
                    bad += (prev & ~a.k[l][i]) != 0;
                }
            }
        done += pairs;
    }
    (void)l5;
    return total * 64;
}

template <int K, bool P>
static int check() {
    int bad = 0;
    static const sdws::LevelSched<K, 4, false, P> s4{};
    static const sdws::LevelSched<K, 5, P, P> s5{};
    static const sdws::LevelSched<K, 6, P, false> s6{};
    const int used[6] = {1, 2, 3, 33, 62, 64};
    std::mt19937 rng(1000 + K);
    static Wave<KeyOps, K> a, b;
    long cases01 = 0;
    const int trials = P ? 500 : 2000;  // per lanes_used; the chained form is an A/B switch, not what ships
    int flags01 = -1;
    for (int u = 0; u < 6; ++u) {
        const int lanes_used = used[u];
        const bool l4 = lanes_used > 8, l5 = lanes_used > 16, l6 = lanes_used > 32;
        if (l4) {
            Flow<K> fl;
            bad += check_flow<K, 4>(s4, fl, false, P && l5);
            if (l5) bad += check_flow<K, 5>(s5, fl, P, P && l6);
            if (l6) bad += check_flow<K, 6>(s6, fl, P, false);
            if (flags01 != l5 * 2 + l6) {  // the 0-1 inputs depend on lanes_used only through the levels that run
                flags01 = l5 * 2 + l6;
                cases01 += zero_one<K, 4, P>(l5, l6, bad);
                if (l5) cases01 += zero_one<K, 5, P>(l5, l6, bad);
                if (l6) cases01 += zero_one<K, 6, P>(l5, l6, bad);
            }
        }
        for (int trial = 0; trial < trials; ++trial) {
            // few distinct values in every third trial, so most keys have duplicates; pads (maximal keys) beyond lanes_used
            const unsigned mask = trial % 3 == 0 ? 0x3fu : trial % 3 == 1 ? 0xffffu : 0x7fffffffu;
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < K; ++i) a.k[l][i] = l < lanes_used ? (unsigned)rng() & mask : 0xffffffffu;
            if (trial % 2)
                for (int i = K - 1 - trial % K; i < K; ++i) a.k[lanes_used - 1][i] = 0xffffffffu;  // a ragged last lane
            sort_front<K>(a, lanes_used);
            b = a;
            piped_levels<KeyOps, K, P>(a, lanes_used);
            serial_levels<K>(b, lanes_used);
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < K; ++i) bad += a.k[l][i] != b.k[l][i];
            for (int p = 1; p < lanes_used * K; ++p) bad += a.k[(p - 1) / K][(p - 1) % K] > a.k[p / K][p % K];
        }
    }
    std::printf("K=%d%s: lists of %d + %d + %d ops, %ld 0-1 cases, %d random waves: %s\n", K, P ? ", first fetches under the merger before" : "", s4.n, s5.n, s6.n, cases01, 6 * trials, bad ? "FAILED" : "ok");
    return bad;
}

// argv[1]: the K to check (12, 20 or 24; all of them without an argument)
int main(int argc, char** argv) {
    const int only = argc > 1 ? std::atoi(argv[1]) : 0;
    int bad = 0;
    if (!only || only == 12) bad += check<12, false>() + check<12, true>();
    if (!only || only == 20) bad += check<20, false>() + check<20, true>();
    if (!only || only == 24) bad += check<24, false>() + check<24, true>();
    return bad ? 1 : 0;
}
