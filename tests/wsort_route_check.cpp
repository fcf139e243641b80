// Host check of the route policies of the register wave sort (csrc/sd_wsort.h: via_lds(policy, L, x)): for every policy and K = 20
// the op lists of the merge levels 4 .. 6 (LevelSched) are run on a model of the 64 lanes x K registers.
//   * routes: lane ^ 4, 16, 31, 63 go through the LDS pipe under every policy, the levels 1 .. 3 never do otherwise, and policy p
//     moves exactly the stages its description names (-60 / -120 / -180 DPP moves per sort at K = 20);
//   * comparators: per key register the same sequence of operations as under policy 0 -- med3 with the same partner register of
//     the same lane ^ x and the same direction bit, then the same operations of the local merger;
//   * waits: the LDS pipe answers in order; every med3 fed through it comes behind a counted wait that leaves at most kMaxLgkm
//     requests outstanding and covers the request it reads;
//   * values: random keys, runs of equal keys, reversed input and pads -- sorted, and equal to the stage-by-stage form.
// out: one line per policy, "policy p: ... ok" or "... FAILED"; exit status 1 on any failure
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "sd_wsort.h"

using sdws::CmpList;
using sdws::SchedOp;

constexpr int K = 20;

static void net_op(const CmpList& c, int i, unsigned* v) {
    if (c.c[i] == sdws::kNone) {
        const unsigned a = v[c.a[i]], b = v[c.b[i]];
        v[c.a[i]] = std::min(a, b);
        v[c.b[i]] = std::max(a, b);
    } else {
        unsigned s[3] = {v[c.a[i]], v[c.b[i]], v[c.c[i]]};
        std::sort(s, s + 3);
        v[c.a[i]] = s[0], v[c.b[i]] = s[1], v[c.c[i]] = s[2];
    }
}

struct Wave {
    unsigned k[64][K];
    unsigned t[64][2 * K];
};

// the stage-by-stage form, written independently of the header's device code
static void serial_stage(Wave& w, int X, int bit, bool rev) {
    static unsigned old[64][K];
    std::copy(&w.k[0][0], &w.k[0][0] + 64 * K, &old[0][0]);
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < K; ++i) {
            const unsigned a = old[l][i], b = old[l ^ X][rev ? K - 1 - i : i];
            w.k[l][i] = ((l >> bit) & 1) ? std::max(a, b) : std::min(a, b);
        }
}
static void serial_level(Wave& w, int L) {
    static const sdws::BitonicNet<K> bnet{};
    const int M = 1 << (L - 1);
    serial_stage(w, 2 * M - 1, L - 1, true);
    for (int h = M / 2, b = L - 2; h >= 1; h >>= 1, --b) serial_stage(w, h, b, false);
    for (int l = 0; l < 64; ++l)
        for (int c = 0; c < bnet.c.n; ++c) net_op(bnet.c, c, w.k[l]);
}
static void sort_front(Wave& w, int lanes_used) {
    static const sdws::SortNet<K> snet{};
    for (int l = 0; l < 64; ++l)
        for (int c = 0; c < snet.c.n; ++c) net_op(snet.c, c, w.k[l]);
    for (int L = 1; L <= 3; ++L)
        if (lanes_used > (1 << (L - 1))) serial_level(w, L);
}

// one op list, op by op over all lanes (an instruction is wave-wide)
template <typename S>
static void run_list(Wave& w, const S& s) {
    static const sdws::BitonicNet<K> bnet{};
    unsigned f[64];
    for (int o = 0; o < s.n; ++o) {
        const SchedOp& op = s.op[o];
        if (op.kind == sdws::kOpFetch) {
            for (int l = 0; l < 64; ++l) f[l] = w.k[l ^ op.c][op.a];
            for (int l = 0; l < 64; ++l) w.t[l][op.b] = f[l];
        } else if (op.kind == sdws::kOpMed) {
            for (int l = 0; l < 64; ++l)
                w.k[l][op.a] = ((l >> op.c) & 1) ? std::max(w.k[l][op.a], w.t[l][op.b]) : std::min(w.k[l][op.a], w.t[l][op.b]);
        } else if (op.kind == sdws::kOpNet) {
            for (int l = 0; l < 64; ++l) net_op(bnet.c, op.a, w.k[l]);
        }
    }
}

// what happens to every key register, in order: (kind, partner register, lane xor, direction bit) or (kind, merger operation)
struct Event {
    int kind, reg, x, bit;
    bool operator==(const Event& o) const { return kind == o.kind && reg == o.reg && x == o.x && bit == o.bit; }
};
template <typename S>
static std::vector<std::vector<Event>> events(const S& s) {
    static const sdws::BitonicNet<K> bnet{};
    std::vector<std::vector<Event>> ev(K);
    int t_reg[2 * K], t_x[2 * K];
    std::fill(t_reg, t_reg + 2 * K, -1);
    std::fill(t_x, t_x + 2 * K, -1);
    for (int o = 0; o < s.n; ++o) {
        const SchedOp& op = s.op[o];
        if (op.kind == sdws::kOpFetch) t_reg[op.b] = op.a, t_x[op.b] = op.c;
        else if (op.kind == sdws::kOpMed) ev[op.a].push_back({sdws::kOpMed, t_reg[op.b], t_x[op.b], op.c});
        else if (op.kind == sdws::kOpNet) {
            const int r[3] = {bnet.c.a[op.a], bnet.c.b[op.a], bnet.c.c[op.a]};
            for (int j = 0; j < 3; ++j)
                if (r[j] != sdws::kNone) ev[r[j]].push_back({sdws::kOpNet, op.a, 0, 0});
        }
    }
    return ev;
}

// the requests to the LDS pipe of one list under `policy`: numbered in issue order, answered in order.  Returns the number of
// faults; *lds: requests, *dpp: DPP moves, *waits: counted waits, *most: the largest count a wait leaves outstanding
template <typename S>
static int check_waits(const S& s, int policy, int L, int* lds, int* dpp, int* waits, int* most) {
    int bad = 0, issued = 0, answered = 0;  // answered: requests known to have returned (a counted wait says so)
    int seq[2 * K];
    std::fill(seq, seq + 2 * K, -1);
    for (int o = 0; o < s.n; ++o) {
        const SchedOp& op = s.op[o];
        if (op.kind == sdws::kOpFetch) {
            if (sdws::via_lds(policy, L, op.c)) seq[op.b] = issued++, ++*lds;
            else seq[op.b] = -1, ++*dpp;
        } else if (op.kind == sdws::kOpWait) {
            bad += op.a > sdws::kMaxLgkm;
            answered = std::max(answered, issued - (int)op.a);
            *most = std::max(*most, (int)op.a);
            ++*waits;
        } else if (op.kind == sdws::kOpMed) {
            bad += seq[op.b] >= answered;  // reads a request no counted wait covers (a DPP move has seq -1)
        }
    }
    return bad;
}

template <int P>
static int check_policy(const std::vector<std::vector<Event>> (&ref)[3], std::vector<std::vector<Event>> (&mine)[3]) {
    static const sdws::LevelSched<K, 4, false, false, P> s4{};
    static const sdws::LevelSched<K, 5, false, false, P> s5{};
    static const sdws::LevelSched<K, 6, false, false, P> s6{};
    int bad = 0;
    // routes
    const int xs[] = {1, 2, 3, 4, 7, 8, 15, 16, 31, 63};
    int moved = 0;
    for (int L = 1; L <= 6; ++L)
        for (int x : xs) {
            const bool always = x == 4 || x == 16 || x == 31 || x == 63, got = sdws::via_lds(P, L, x);
            bool want = always;
            if (L >= 4) {
                want |= P >= 1 && ((L == 4 && x == 15) || (L >= 5 && x == 8));
                want |= P >= 2 && x == 2;
                want |= P >= 3 && x == 1;
            }
            bad += got != want;
            // stages of the sort that exist: lane ^ (2M - 1) first, then lane ^ h, h < M
            const int M = 1 << (L - 1);
            const bool exists = x == 2 * M - 1 || (x < M && (x & (x - 1)) == 0);
            moved += exists && got && !always;
        }
    bad += moved != 3 * P;  // three stages per step of the policy: K fewer DPP moves each
    mine[0] = events(s4), mine[1] = events(s5), mine[2] = events(s6);
    for (int i = 0; i < 3; ++i) bad += !(mine[i] == ref[i]);
    int lds = 0, dpp = 0, waits = 0, most = 0;
    bad += check_waits(s4, P, 4, &lds, &dpp, &waits, &most);
    bad += check_waits(s5, P, 5, &lds, &dpp, &waits, &most);
    bad += check_waits(s6, P, 6, &lds, &dpp, &waits, &most);
    bad += lds + dpp != 15 * K;  // the levels 4 .. 6 have 4 + 5 + 6 stages
    // values: through the whole sort, against the stage-by-stage form
    static Wave a, b;
    std::mt19937 rng(77 + P);
    int waves = 0;
    for (int lanes_used : {64, 62, 57, 33, 17, 9}) {
        for (int kind = 0; kind < 6; ++kind) {
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < K; ++i) {
                    const unsigned pos = (unsigned)(l * K + i);
                    unsigned v;
                    switch (kind) {
                        case 0: v = (unsigned)rng(); break;                  // random keys
                        case 1: v = (unsigned)rng() & 0x3fu; break;          // few distinct values: long runs of equal keys
                        case 2: v = (pos / 37u) * 2048u; break;              // runs of equal keys, ascending
                        case 3: v = 0x7fffffffu - pos * 2048u; break;        // reversed input
                        case 4: v = 0x7fffffffu - (pos / 23u) * 2048u; break;  // reversed runs of equal keys
                        default: v = 12345u; break;                          // every key equal
                    }
                    a.k[l][i] = l < lanes_used ? v & 0x7fffffffu : 0x80000000u + pos;  // pads beyond lanes_used
                }
            sort_front(a, lanes_used);
            b = a;
            run_list(a, s4);
            if (lanes_used > 16) run_list(a, s5);
            if (lanes_used > 32) run_list(a, s6);
            for (int L = 4; L <= 6; ++L)
                if (lanes_used > (1 << (L - 1))) serial_level(b, L);
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < K; ++i) bad += a.k[l][i] != b.k[l][i];
            for (int p = 1; p < lanes_used * K; ++p) bad += a.k[(p - 1) / K][(p - 1) % K] > a.k[p / K][p % K];
            ++waves;
        }
    }
    std::printf("policy %d: lists of %d + %d + %d ops, %d requests to the LDS pipe, %d DPP moves, %d counted waits (at most %d outstanding), %d waves: %s\n",
                P, s4.n, s5.n, s6.n, lds, dpp, waits, most, waves, bad ? "FAILED" : "ok");
    return bad;
}

int main() {
    static_assert(sdws::kRoutePolicies == 4, "a policy without a check");
    std::vector<std::vector<Event>> ref[3], got[3];
    int bad = check_policy<0>(ref, ref);  // (compares policy 0 with itself; fills ref)
    bad += check_policy<1>(ref, got);
    bad += check_policy<2>(ref, got);
    bad += check_policy<3>(ref, got);
    return bad ? 1 : 0;
}
