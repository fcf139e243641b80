// Wave-level sort of 32-bit keys held in registers: 64 lanes x K keys, no LDS storage at all.
//
// Layout: blocked -- lane l holds K keys; afterwards lane l owns sorted positions K*l .. K*l + K-1 (ascending in
// k[0..K)).  The network is a bitonic sort over 64 *blocks*:
//
//   * every lane sorts its K keys with a comparator network (Batcher's odd-even merge sort pruned to K inputs);
//   * level L = 1..6 merges pairs of sorted runs of m = 2^(L-1) lanes.  Step 1 compares element i of lane l with
//     element K-1-i of lane l ^ (2m-1) (the partner run read backwards): the lower run keeps the minima and the upper
//     run the maxima, both as bitonic sequences.  Steps 2.. are half-cleaners between lanes l and l ^ h, h = m/2 .. 1
//     (same element index); they leave every lane with a bitonic sequence of K keys, which a local bitonic merger
//     sorts.  21 cross-lane stages and 6 local mergers in all.
//   * a cross-lane stage costs two vector instructions per key: fetch the partner's key (DPP move for lane ^ 1, 2, 3, 7,
//     8, 15; ds_swizzle -- the LDS crossbar, no LDS memory -- for lane ^ 4, 16, 31; ds_bpermute for lane ^ 63) and
//     v_med3_u32(own, partner, sel) with sel = 0 in the lanes that keep the minimum and 0xffffffff in those that keep
//     the maximum: median(a, b, 0) = min(a, b), median(a, b, ~0) = max(a, b).  No lane-dependent sign conventions, no
//     divergence; all keys stay in true ascending order.  Which route a stage takes is one function, via_lds(policy, L, x):
//     the policies 1 .. 3 move DPP stages of the levels 4 .. 6 to the LDS pipe (one vector instruction per key less each);
//     measured inside bcsd_fd_kernel every step of them is slower (profiles/fd_valu/README.md), so every kernel uses policy 0.
//   * the local merger sorts cyclic-bitonic sequences: even lengths are half-cleaned and split; the odd lengths 3 and 5
//     (K = 12, 24; K = 20) end in 3-sorters (v_min3 / v_med3 / v_max3_u32), other odd lengths in a full sorter.
//
//   * schedule of the levels 4..6, whose stages lane ^ 4, 16, 31, 63 go through the LDS pipe (a round trip of a hundred cycles and
//     more against none for a DPP move): in the stages after the first every key register is a dependency chain of its own, so a
//     level runs as two half-batches of K/2 keys (LevelSched below).  One half issues its ds_swizzle requests and the other half
//     then runs its own DPP moves and v_med3 until it has requests of its own in flight; only then are the first half's results
//     consumed, behind one counted s_waitcnt lgkmcnt per half-batch.  The comparators and their order per register are those of
//     the stage-by-stage form, so the result is bit-identical; -DSD_WSORT_SERIAL keeps that form for A/B runs
//     (microbench/wsort_occ.hip, wsort_test.hip), and K = 24 always uses it (registers).  Not the default, -DSD_WSORT_PREFETCH: the
//     first stage of the levels 5 and 6 reads registers the local merger of the level before has finished sub-block by sub-block
//     (K = 20: 5|5|5|5), so its requests can go out under the merging of the other sub-blocks -- at K more live registers, which
//     bcsd_fd_kernel does not have.  tests/wsort_sched_check.cpp runs a host model of the op lists; profiles/wsort_pipe/ has
//     the measurements (-3.6 % per sort with two resident waves per SIMD, -0.8 % on the BCSD headline).
//
// K = 20: 202 + 6 * 80 + 21 * 20 * 2 = ~1 520 32-bit instructions per 1 280 keys, against ~2 800 mostly double-rate instructions and 410 LDS instructions of the f64 merge sort of
// sd_wave.h.  tools/dev/nets.py checks the networks (0-1 principle), tools/dev/sim_wave_bitonic.py the lane scheme.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace sdws {

constexpr int kMaxCmp = 400;

// a list of operations on registers: compare-exchange (a, b) -- min to a, max to b -- or, when c != kNone, a 3-sorter
// (a, b, c) -- min to a, median to b, max to c: v_min3_u32, v_med3_u32, v_max3_u32, three instructions for what three
// compare-exchanges (six instructions) do
constexpr unsigned char kNone = 0xff;
struct CmpList {
    int n = 0;
    unsigned char a[kMaxCmp] = {}, b[kMaxCmp] = {}, c[kMaxCmp] = {};
    constexpr void add(int lo, int hi) {
        a[n] = (unsigned char)lo;
        b[n] = (unsigned char)hi;
        c[n] = kNone;
        ++n;
    }
    constexpr void add3(int lo, int mid, int hi) {
        a[n] = (unsigned char)lo;
        b[n] = (unsigned char)mid;
        c[n] = (unsigned char)hi;
        ++n;
    }
};

// Batcher's odd-even merge sort for the inputs base .. base + K-1 (comparators that would touch the +inf padding up
// to the next power of two are no-ops and dropped)
constexpr void batcher_into(CmpList& out, int K, int base) {
    int N = 1;
    while (N < K) N <<= 1;
    for (int p = 1; p < N; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j + k < N; j += 2 * k)
                for (int i = 0; i < k; ++i) {
                    const int lo = i + j, hi = i + j + k;
                    if (hi < N && lo / (2 * p) == hi / (2 * p) && hi < K) out.add(base + lo, base + hi);
                }
}

template <int K>
struct SortNet {
    CmpList c;
    constexpr SortNet() { batcher_into(c, K, 0); }
};

// sorts every cyclic-bitonic sequence of K keys
template <int K>
struct BitonicNet {
    CmpList c;
    constexpr BitonicNet() {
        int sb[64] = {}, sl[64] = {};
        int sp = 0;
        sb[sp] = 0;
        sl[sp] = K;
        ++sp;
        while (sp > 0) {
            --sp;
            const int base = sb[sp], len = sl[sp];
            if (len <= 1) continue;
            if (len % 2 == 0) {
                const int h = len / 2;
                for (int i = 0; i < h; ++i) c.add(base + i, base + i + h);
                sb[sp] = base + h;
                sl[sp] = h;
                ++sp;
                sb[sp] = base;
                sl[sp] = h;
                ++sp;
            } else if (len == 3) {
                c.add3(base, base + 1, base + 2);
            } else if (len == 5) {
                // found by exhaustive search over the cyclic-bitonic 0-1 inputs (tools/dev/nets.py checks it): 10 instructions
                c.add(base, base + 2);
                c.add(base + 1, base + 3);
                c.add3(base, base + 1, base + 4);
                c.add3(base + 2, base + 3, base + 4);
            } else {
                batcher_into(c, len, base);
            }
        }
    }
};


// ---- issue order of one merge level (levels 4 .. 6), as a list of operations on the key registers k[0..K) and the partner
// temporaries t[0..2K): the kernels execute the list as straight-line code, the host check (tests/wsort_sched_check.cpp) runs it
// on a model of the 64 lanes.
//   kOpFetch      t[b] = k[a] of lane ^ c
//   kOpFetchNext  the same for the first stage of the NEXT level; executed only when that level runs
//   kOpMed        k[a] = med3(k[a], t[b], lanes with bit c set keep the maximum)
//   kOpNet        operation a of BitonicNet<K>
//   kOpFence      the instruction scheduler moves nothing across
//   kOpWait       s_waitcnt lgkmcnt(a): at most a requests to the LDS pipe still out
constexpr unsigned char kOpFetch = 0, kOpFetchNext = 1, kOpMed = 2, kOpNet = 3, kOpFence = 4, kOpWait = 5;
constexpr int kMaxLgkm = 15;  // the counter has four bits
struct SchedOp {
    unsigned char kind, a, b, c;
};
constexpr int kMaxSched = 768;
// Route of a cross-lane stage: the partner lane ^ x of merge level L comes through the LDS pipe (ds_swizzle / ds_bpermute: no
// vector instruction) or by a DPP move (one vector instruction per key).  lane ^ 4, 16, 31, 63 have no DPP form.  The others have
// both, and saturated the two cost the same (profiles/r06/microbench_permlane_swap.log), so which is cheaper depends on how busy
// the kernel keeps either pipe: a policy moves stages of the levels 4 .. 6 -- where LevelSched hides the round trip behind the
// other half-batch -- to the LDS pipe.  The levels 1 .. 3 hide nothing and stay DPP under every policy.
//   0  DPP wherever it exists
//   1  + lane ^ 15 in level 4 and lane ^ 8 in the levels 5 and 6     (-60 vector instructions per sort at K = 20)
//   2  + lane ^ 2 in the levels 4 .. 6                                (-120)
//   3  + lane ^ 1 in the levels 4 .. 6                                (-180)
// LevelSched and lane_xor both read this one function.  A kernel names its policy in wave_sort<K, POLICY>; the default is 0.
constexpr int kRoutePolicies = 4;
constexpr bool via_lds(int policy, int L, int x) {
    if (x == 4 || x == 16 || x == 31 || x == 63) return true;
    if (L < 4) return false;
    if (policy >= 1 && ((L == 4 && x == 15) || (L >= 5 && x == 8))) return true;
    if (policy >= 2 && x == 2) return true;
    if (policy >= 3 && x == 1) return true;
    return false;
}

// A/B: -DSD_WSORT_PREFETCH chains the levels 4 -> 5 -> 6 through PRE / NEXT below.  Not the default: up to K more temporaries are
// live across a merger, and bcsd_fd_kernel<20> then spills (128 VGPRs, 14 to scratch).
#ifdef SD_WSORT_PREFETCH
constexpr bool kPrefetch = true;
#else
constexpr bool kPrefetch = false;
#endif

// Level L (runs of M = 2^(L-1) lanes).  Stage 0 pairs element i with element K-1-i of lane ^ (2M-1) and writes its partners to
// t[K + i]; the stages h = M/2 .. 1 pair element i with element i of lane ^ h through t[i].
//   PRE   the fetches of stage 0 were issued by the level before (its NEXT)
//   NEXT  issue the fetches of the next level's stage 0 inside the local merger, each register once no later operation of the
//         merger touches it
// The halves A = [0, K/2) and B = [K/2, K) each walk stage by stage; a half that has just issued fetches through the LDS pipe
// hands over to the other one, which runs until it has issued such fetches itself (or is done).  Every med3 of stage 0 comes after
// all fetches of stage 0: it overwrites a register the partner lane reads.
template <int K, int L, bool PRE, bool NEXT, int POLICY = 0>
struct LevelSched {
    static constexpr bool via_lds(int x) { return sdws::via_lds(POLICY, L, x); }
    int n = 0;
    SchedOp op[kMaxSched] = {};
    constexpr void put(unsigned char kind, int a, int b, int c) {
        op[n].kind = kind;
        op[n].a = (unsigned char)a;
        op[n].b = (unsigned char)b;
        op[n].c = (unsigned char)c;
        ++n;
    }
    constexpr void fence() {
        if (n > 0 && op[n - 1].kind != kOpFence) put(kOpFence, 0, 0, 0);
    }
    BitonicNet<K> net{};
    // the merger's last operation on register r
    constexpr int last_use(int r) const {
        int last = -1;
        for (int c = 0; c < net.c.n; ++c)
            if (net.c.a[c] == r || net.c.b[c] == r || (net.c.c[c] != kNone && net.c.c[c] == r)) last = c;
        return last;
    }
    constexpr LevelSched() {
        constexpr int M = 1 << (L - 1), H = K / 2;
        int xs[6] = {}, bits[6] = {}, S = 0;
        xs[S] = 2 * M - 1;
        bits[S] = L - 1;
        ++S;
        for (int h = 16, b = 4; h >= 1; h >>= 1, --b)
            if (M >= 2 * h) {
                xs[S] = h;
                bits[S] = b;
                ++S;
            }
        // sequence numbers of the requests to the LDS pipe, which answers in order: a group of med3 that reads answers up to
        // number q waits for lgkmcnt(issued - 1 - q) once, and the compiler's own per-use waits behind it fall away
        int seq[2 * K] = {}, issued = 0;
        for (int i = 0; i < 2 * K; ++i) seq[i] = -1;
        // the half that goes first consumes the other half's registers: after a prefetch those of A (final first in the merger)
        int h = PRE ? 1 : 0;
        if (PRE) {
            for (int c = 0; c < net.c.n; ++c)
                for (int r = 0; r < K; ++r)
                    if (last_use(r) == c) seq[K + r] = issued++;
        } else {
            for (int j = 0; j < K; ++j) {
                const int i = (j + H) % K;  // B's registers first: A consumes them
                put(kOpFetch, i, K + i, xs[0]);
                if (via_lds(xs[0])) seq[K + i] = issued++;
            }
        }
        int st[2] = {0, 0};  // per half: the stage whose fetches are issued and whose med3 are due
        while (st[0] < S || st[1] < S) {
            if (st[h] >= S) {
                h = 1 - h;
                continue;
            }
            const int lo = h ? H : 0, hi = h ? K : H, s = st[h];
            if (via_lds(xs[s])) {
                int q = -1;
                for (int i = lo; i < hi; ++i) q = seq[s == 0 ? K + (K - 1 - i) : i] > q ? seq[s == 0 ? K + (K - 1 - i) : i] : q;
                fence();
                if (issued - 1 - q <= kMaxLgkm) {
                    put(kOpWait, issued - 1 - q, 0, 0);
                    fence();  // or the med3 below are scheduled in front of the wait and get waits of their own
                }
            }
            for (int i = lo; i < hi; ++i) put(kOpMed, i, s == 0 ? K + (K - 1 - i) : i, bits[s]);
            ++st[h];
            if (st[h] < S) {
                const int x = xs[st[h]];
                if (via_lds(x)) fence();
                for (int i = lo; i < hi; ++i) {
                    put(kOpFetch, i, i, x);
                    if (via_lds(x)) seq[i] = issued++;
                }
                if (via_lds(x)) {
                    fence();
                    h = 1 - h;
                }
            }
        }
        fence();
        for (int c = 0; c < net.c.n; ++c) {
            put(kOpNet, c, 0, 0);
            if (!NEXT) continue;
            bool any = false;
            for (int r = 0; r < K; ++r)
                if (last_use(r) == c) {
                    put(kOpFetchNext, r, K + r, 4 * M - 1);
                    any = true;
                }
            if (any) fence();
        }
        fence();
    }
};

#ifdef __HIPCC__
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
// median of three; the compiler matches max(min(a, b), min(max(a, b), c)) to v_med3_u32
__device__ __forceinline__ unsigned med3(unsigned a, unsigned b, unsigned c) { return umax(umin(a, b), umin(umax(a, b), c)); }

// the value lane (l ^ X) holds in v; LDS: through the LDS pipe (via_lds of the stage's level and policy)
template <int X, bool LDS>
__device__ __forceinline__ unsigned lane_xor(unsigned v, int addr63) {
    static_assert(LDS || !via_lds(0, 6, X), "lane ^ 4, 16, 31, 63 have no DPP form");
    if constexpr (X == 63) return (unsigned)__builtin_amdgcn_ds_bpermute(addr63, (int)v);
    else if constexpr (LDS) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F);  // and 0x1f, xor X (X < 32)
    else if constexpr (X == 1) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    else if constexpr (X == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (X == 3) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x1B, 0xF, 0xF, true);   // quad_perm [3,2,1,0]
    else if constexpr (X == 7) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    else if constexpr (X == 15) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    else {
        static_assert(X == 8, "unsupported lane permutation");
        return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);   // row_ror:8
    }
}

template <int K, typename Net>
__device__ __forceinline__ void apply_net(unsigned (&k)[K], const Net& net) {
#pragma unroll
    for (int c = 0; c < net.c.n; ++c) {
        if (net.c.c[c] == kNone) {
            const unsigned lo = umin(k[net.c.a[c]], k[net.c.b[c]]);
            const unsigned hi = umax(k[net.c.a[c]], k[net.c.b[c]]);
            k[net.c.a[c]] = lo;
            k[net.c.b[c]] = hi;
        } else {
            // written out: the compiler re-associates min(min(x, z), y) to share min(x, y) with its v_med3 pattern and then
            // emits five instructions instead of three
            const unsigned x = k[net.c.a[c]], y = k[net.c.b[c]], z = k[net.c.c[c]];
            unsigned lo, mid, hi;
            asm("v_min3_u32 %0, %3, %4, %5\n\tv_med3_u32 %1, %3, %4, %5\n\tv_max3_u32 %2, %3, %4, %5"
                : "=&v"(lo), "=&v"(mid), "=&v"(hi)
                : "v"(x), "v"(y), "v"(z));
            k[net.c.a[c]] = lo;
            k[net.c.b[c]] = mid;
            k[net.c.c[c]] = hi;
        }
    }
}

// Registers written by the inline assembly above may be read by a DPP move right away, and the compiler's hazard
// recognizer does not look inside inline assembly (a VALU write needs two wait states before a DPP read of the same
// register): every key passes through one "s_nop 1" after a network that uses 3-sorters.
constexpr bool uses_sort3(const CmpList& c) {
    for (int i = 0; i < c.n; ++i)
        if (c.c[i] != kNone) return true;
    return false;
}
template <int K>
__device__ __forceinline__ void dpp_fence(unsigned (&k)[K]) {
    if constexpr (!uses_sort3(BitonicNet<K>{}.c)) {
        return;
    } else if constexpr (K == 20) {
        asm volatile("s_nop 1"
                     : "+v"(k[0]), "+v"(k[1]), "+v"(k[2]), "+v"(k[3]), "+v"(k[4]), "+v"(k[5]), "+v"(k[6]), "+v"(k[7]), "+v"(k[8]), "+v"(k[9]),
                       "+v"(k[10]), "+v"(k[11]), "+v"(k[12]), "+v"(k[13]), "+v"(k[14]), "+v"(k[15]), "+v"(k[16]), "+v"(k[17]), "+v"(k[18]),
                       "+v"(k[19]));
    } else if constexpr (K == 12) {
        asm volatile("s_nop 1"
                     : "+v"(k[0]), "+v"(k[1]), "+v"(k[2]), "+v"(k[3]), "+v"(k[4]), "+v"(k[5]), "+v"(k[6]), "+v"(k[7]), "+v"(k[8]), "+v"(k[9]),
                       "+v"(k[10]), "+v"(k[11]));
    } else {
        static_assert(K == 24, "add the operand list for this K");
        asm volatile("s_nop 1"
                     : "+v"(k[0]), "+v"(k[1]), "+v"(k[2]), "+v"(k[3]), "+v"(k[4]), "+v"(k[5]), "+v"(k[6]), "+v"(k[7]), "+v"(k[8]), "+v"(k[9]),
                       "+v"(k[10]), "+v"(k[11]), "+v"(k[12]), "+v"(k[13]), "+v"(k[14]), "+v"(k[15]), "+v"(k[16]), "+v"(k[17]), "+v"(k[18]),
                       "+v"(k[19]), "+v"(k[20]), "+v"(k[21]), "+v"(k[22]), "+v"(k[23]));
    }
}

// one cross-lane stage: partner = lane ^ X; the lane with bit BIT of its id clear keeps the minima.  REV: element i
// meets element K-1-i of the partner (the first stage of a level), otherwise element i.
template <int K, int X, int BIT, bool REV>
__device__ __forceinline__ void cross_stage(unsigned (&k)[K], int lane, int addr63) {
    const unsigned sel = (unsigned)(-((lane >> BIT) & 1));
    unsigned t[K];
#pragma unroll
    for (int i = 0; i < K; ++i) t[i] = lane_xor<X, via_lds(0, BIT + 1, X)>(k[i], addr63);  // (stage by stage: nothing hides a round trip)
#pragma unroll
    for (int i = 0; i < K; ++i) k[i] = med3(k[i], t[REV ? K - 1 - i : i], sel);
}

// One level in the issue order of LevelSched.  t: the partner temporaries, kept by the caller because a level's NEXT fetches are
// consumed by the level after it; `next` (wave-uniform): that level runs.  The compiler places the s_waitcnt lgkmcnt itself (the
// LDS pipe returns in order, so they are counted); the fences keep the requests and their consumers where the list puts them.
template <int K, int L, bool PRE, bool NEXT, int POLICY>
struct LevelTables {
    static constexpr LevelSched<K, L, PRE, NEXT, POLICY> s{};
    static constexpr BitonicNet<K> bnet{};
};

template <int K, int L, bool PRE, bool NEXT, int POLICY, int O>
__device__ __forceinline__ void sched_step(unsigned (&k)[K], unsigned (&t)[2 * K], int lane, int addr63, bool next) {
    using T = LevelTables<K, L, PRE, NEXT, POLICY>;
    constexpr int kind = T::s.op[O].kind, a = T::s.op[O].a, b = T::s.op[O].b, c = T::s.op[O].c;
    if constexpr (kind == kOpFetch) {
        t[b] = lane_xor<c, via_lds(POLICY, L, c)>(k[a], addr63);
    } else if constexpr (kind == kOpFetchNext) {
        if (next) t[b] = lane_xor<c, via_lds(POLICY, L + 1, c)>(k[a], addr63);
    } else if constexpr (kind == kOpMed) {
        k[a] = med3(k[a], t[b], (unsigned)(-((lane >> c) & 1)));
    } else if constexpr (kind == kOpNet) {
        constexpr int ra = T::bnet.c.a[a], rb = T::bnet.c.b[a], rc = T::bnet.c.c[a];
        if constexpr (rc == kNone) {
            const unsigned lo = umin(k[ra], k[rb]);
            const unsigned hi = umax(k[ra], k[rb]);
            k[ra] = lo;
            k[rb] = hi;
        } else {
            // see apply_net
            const unsigned x = k[ra], y = k[rb], z = k[rc];
            unsigned lo, mid, hi;
            asm("v_min3_u32 %0, %3, %4, %5\n\tv_med3_u32 %1, %3, %4, %5\n\tv_max3_u32 %2, %3, %4, %5"
                : "=&v"(lo), "=&v"(mid), "=&v"(hi)
                : "v"(x), "v"(y), "v"(z));
            k[ra] = lo;
            k[rb] = mid;
            k[rc] = hi;
        }
    } else if constexpr (kind == kOpWait) {
        __builtin_amdgcn_s_waitcnt(0xC07F | (a << 8));  // lgkmcnt(a); vmcnt and expcnt at their maxima: no wait
    } else {
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int K, int L, bool PRE, bool NEXT, int POLICY, int... O>
__device__ __forceinline__ void sched_steps(unsigned (&k)[K], unsigned (&t)[2 * K], int lane, int addr63, bool next, std::integer_sequence<int, O...>) {
    (sched_step<K, L, PRE, NEXT, POLICY, O>(k, t, lane, addr63, next), ...);
}

template <int K, int L, bool PRE, bool NEXT, int POLICY>
__device__ __forceinline__ void merge_level_piped(unsigned (&k)[K], unsigned (&t)[2 * K], int lane, int addr63, bool next) {
    sched_steps<K, L, PRE, NEXT, POLICY>(k, t, lane, addr63, next, std::make_integer_sequence<int, LevelTables<K, L, PRE, NEXT, POLICY>::s.n>{});
}

template <int K, int L>
__device__ __forceinline__ void merge_level(unsigned (&k)[K], int lane, int addr63) {
    constexpr int M = 1 << (L - 1);
    constexpr BitonicNet<K> bnet{};
    cross_stage<K, 2 * M - 1, L - 1, true>(k, lane, addr63);
    if constexpr (M >= 32) cross_stage<K, 16, 4, false>(k, lane, addr63);
    if constexpr (M >= 16) cross_stage<K, 8, 3, false>(k, lane, addr63);
    if constexpr (M >= 8) cross_stage<K, 4, 2, false>(k, lane, addr63);
    if constexpr (M >= 4) cross_stage<K, 2, 1, false>(k, lane, addr63);
    if constexpr (M >= 2) cross_stage<K, 1, 0, false>(k, lane, addr63);
    apply_net<K>(k, bnet);
    dpp_fence<K>(k);
}

// Sorts the wave's 64 * K keys; `lanes_used` (wave-uniform) = number of leading lanes that hold data: lanes beyond
// must hold keys >= every key of the lanes in use (pads), and merge levels that could only move pads are skipped.
// POLICY: route of the cross-lane stages of the levels 4 .. 6 (via_lds)
template <int K, int POLICY = 0>
__device__ __forceinline__ void wave_sort(unsigned (&k)[K], int lane, int lanes_used = 64) {
    static_assert(POLICY >= 0 && POLICY < kRoutePolicies, "route policy");
    constexpr SortNet<K> snet{};
    const int addr63 = (lane ^ 63) << 2;
    apply_net<K>(k, snet);
    if (lanes_used > 1) merge_level<K, 1>(k, lane, addr63);
    if (lanes_used > 2) merge_level<K, 2>(k, lane, addr63);
    if (lanes_used > 4) merge_level<K, 3>(k, lane, addr63);
#ifndef SD_WSORT_SERIAL
    // the levels with stages on the LDS pipe, in the issue order of LevelSched.  No "s_nop 1" between them: the stage behind a
    // merger reads through the LDS pipe there; the one fence at the end is for a DPP read by the caller.  K = 24 stays stage by
    // stage: bcsd_fx_kernel<24>, which spills already, spills more with the fences in its way.
    if constexpr (K > 20) {
        if (lanes_used > 8) merge_level<K, 4>(k, lane, addr63);
        if (lanes_used > 16) merge_level<K, 5>(k, lane, addr63);
        if (lanes_used > 32) merge_level<K, 6>(k, lane, addr63);
    } else if (lanes_used > 8) {
        unsigned t[2 * K];
        const bool l5 = lanes_used > 16, l6 = lanes_used > 32;
        merge_level_piped<K, 4, false, kPrefetch, POLICY>(k, t, lane, addr63, l5);
        if (l5) {
            merge_level_piped<K, 5, kPrefetch, kPrefetch, POLICY>(k, t, lane, addr63, l6);
            if (l6) merge_level_piped<K, 6, kPrefetch, false, POLICY>(k, t, lane, addr63, false);
        }
        dpp_fence<K>(k);
    }
#else
    // A/B: stage by stage over all K keys
    if (lanes_used > 8) merge_level<K, 4>(k, lane, addr63);
    if (lanes_used > 16) merge_level<K, 5>(k, lane, addr63);
    if (lanes_used > 32) merge_level<K, 6>(k, lane, addr63);
#endif
}
#endif  // __HIPCC__

}  // namespace sdws
