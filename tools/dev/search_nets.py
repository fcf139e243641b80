"""Search for the K = 20 networks of csrc/sd_wsort.h under the instruction cost of the ISA: a compare-exchange is two vector
instructions (v_min_u32, v_max_u32), a 3-sorter three (v_min3 / v_med3 / v_max3_u32) -- the work of three compare-exchanges.

Two problems, both by the 0-1 principle:
  sorter   sort all 2^20 0-1 inputs of 20 keys                      (SortNet<20>;    Batcher pruned to 20 inputs: 103 comparators, 206)
  merger   sort all 382 cyclic-bitonic 0-1 inputs of length 20      (BitonicNet<20>; half-cleaners + four 5-nets:     80)

Method, in two steps per problem.

1. A beam search over the SET of reachable 0-1 states.  A state is a 20-bit word (bit i = key i); an operation maps the set
   onto a smaller one, and the network sorts exactly when K + 1 states are left (the sorted word of every number of ones: the
   operations put the minimum on the lower index, so a sorted word never moves and is always reachable).  Candidates live on
   cost levels (instructions spent so far); on every level the `beam` candidates with the fewest reachable states are extended
   by every compare-exchange (a, b) and every 3-sorter (a, b, c), a < b < c, that shrinks the set, onto the levels cost + 2 and
   cost + 3.  Equal state sets on a level are kept once.  Ties in the set size go to the smaller dependency depth (instructions
   along the longest chain: either operation is one instruction deep), then to a seeded random number.  The first level with a
   sorting network ends the search.  (Sorter: 145 instructions; the plain greedy choice, beam 1, gives 153.)
2. A local search on that network: random edits -- delete an operation, narrow a 3-sorter to a compare-exchange, change one
   register, swap neighbours, move an operation, widen a compare-exchange to a 3-sorter while deleting another operation --
   kept when the network still sorts (bit-sliced 0-1 check) and costs no more.  Steps at equal cost let it drift off a local
   minimum.  The cheapest network seen wins, the shallowest among equals.  (Sorter: 145 -> 138.)
A last pass drops operations that turned out redundant, narrows 3-sorters where that still sorts, and orders the operations
layer by layer (every register's operations stay in their own order).

The sorter's first layer is fixed: six 3-sorters and one compare-exchange (20 instructions) sort the triples
(0 1 2) .. (15 16 17) and the pair (18 19), which leaves 4^6 * 3 = 12 288 states of the 2^20.  The merger's problem is tiny and
the merger runs six times per sort, so it gets 24 independent searches (seeds SEED + 1 ..), side by side on the CPU cores; the
best one is kept (73 instructions at depth 6; most seeds end at 74).

Live temporaries: a 3-sorter needs its three results beside its three inputs for the length of three instructions; no
operation keeps anything else alive, and the kernels' register counts did not move (profiles/wsort_nets/README.md).

    python tools/dev/search_nets.py            # search, verify, report, write csrc/sd_wsort_nets20.h
    python tools/dev/search_nets.py --check    # verify and report the committed header against today's constructions

numpy only; fixed seed; about three minutes on eight CPU cores.
"""
import argparse
import multiprocessing
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "scikit-downscale_amd", "csrc", "sd_wsort_nets20.h")
K = 20
SEED = 20
CHUNK = 1 << 22  # elements of one vectorised batch of operations


# ---- operations on sets of 0-1 states ------------------------------------------------------------------------------------
def ce(x, a, b):
    """compare-exchange on words: minimum (and) to bit a, maximum (or) to bit b; a, b scalars or columns of operations"""
    swap = (x >> a) & ~(x >> b) & 1
    return x ^ (swap << a) ^ (swap << b)


def apply_op(x, op):
    if len(op) == 2:
        return ce(x, op[0], op[1])
    a, b, c = op
    return ce(ce(ce(x, a, b), b, c), a, b)


def run(ops, x):
    for op in ops:
        x = np.unique(apply_op(x, op))
    return x


def cost(ops):
    return sum(2 if len(op) == 2 else 3 for op in ops)


def depth(ops, k=K):
    d = [0] * k
    for op in ops:
        t = max(d[r] for r in op) + 1
        for r in op:
            d[r] = t
    return max(d)


def all_states(k):
    return np.arange(1 << k, dtype=np.uint32)


def cyclic_bitonic_states(k):
    cols = nets.cyclic_bitonic01(k)
    x = np.zeros(len(cols[0]), dtype=np.uint32)
    for i, c in enumerate(cols):
        x |= c.astype(np.uint32) << np.uint32(i)
    return np.unique(x)


def sorts(ops, start, k=K):
    return len(run(ops, start)) == k + 1


# ---- beam search ---------------------------------------------------------------------------------------------------------
def op_table(k):
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    triples = [(a, b, c) for a in range(k) for b in range(a + 1, k) for c in range(b + 1, k)]
    return pairs, triples


def expand(x, ops):
    """sizes of the state sets every operation of `ops` leaves, and those sets as rows of sorted words"""
    width = len(ops[0])
    cols = [np.array([op[i] for op in ops], dtype=np.uint32)[:, None] for i in range(width)]
    step = max(1, CHUNK // len(x))
    sizes, rows = [], []
    for lo in range(0, len(ops), step):
        sl = slice(lo, lo + step)
        y = x[None, :]
        if width == 2:
            y = ce(y, cols[0][sl], cols[1][sl])
        else:
            y = ce(ce(ce(y, cols[0][sl], cols[1][sl]), cols[1][sl], cols[2][sl]), cols[0][sl], cols[1][sl])
        y.sort(axis=1)
        sizes.append((np.diff(y, axis=1) != 0).sum(axis=1) + 1)
        rows.append(y)
    return np.concatenate(sizes), rows, step


def beam_search(start, prefix, beam, rng, k=K, log=None):
    pairs, triples = op_table(k)
    x0 = run(prefix, np.unique(start))
    d0 = [0] * k
    for op in prefix:
        t = max(d0[r] for r in op) + 1
        for r in op:
            d0[r] = t
    # a candidate: (states left, depth, random tie-break, operations, state set, depth per register)
    levels = {cost(prefix): [(len(x0), max(d0), 0.0, list(prefix), x0, d0)]}
    c = cost(prefix)
    while True:
        if c not in levels:
            c += 1
            continue
        cands = sorted(levels.pop(c), key=lambda t: t[:3])
        done = [t for t in cands if t[0] == k + 1]
        if done:
            return done[0][3]
        seen, kept = set(), []
        for t in cands:
            h = t[4].tobytes()
            if h not in seen:
                seen.add(h)
                kept.append(t)
            if len(kept) == beam:
                break
        if log:
            log(f"  cost {c:3d}: {len(cands):5d} candidates, best {kept[0][0]:6d} states, depth {kept[0][1]}")
        for n, _, _, ops, x, dreg in kept:
            for table, w in ((pairs, 2), (triples, 3)):
                sizes, rows, step = expand(x, table)
                # only the best few extensions of one candidate can enter the next beam
                order = np.argsort(sizes, kind="stable")[: 2 * beam]
                for j in order:
                    if sizes[j] >= n:
                        break
                    op = table[j]
                    t = max(dreg[r] for r in op) + 1
                    d = list(dreg)
                    for r in op:
                        d[r] = t
                    y = rows[j // step][j % step]
                    y = y[np.concatenate(([True], np.diff(y) != 0))]
                    levels.setdefault(c + w, []).append((int(sizes[j]), max(d), float(rng.random()), ops + [op], y, d))
        c += 1


def tighten(ops, start, n_fixed, k=K):
    """drop redundant operations, narrow 3-sorters to one compare-exchange; the first n_fixed operations stay"""
    ops = list(ops)
    changed = True
    while changed:
        changed = False
        for i in range(len(ops) - 1, n_fixed - 1, -1):
            trial = ops[:i] + ops[i + 1:]
            if sorts(trial, start, k):
                ops, changed = trial, True
                continue
            if len(ops[i]) == 3:
                a, b, c = ops[i]
                for sub in ((a, b), (b, c), (a, c)):
                    trial = ops[:i] + [sub] + ops[i + 1:]
                    if sorts(trial, start, k):
                        ops, changed = trial, True
                        break
    return ops


# ---- local search on a sorting network: random edits, kept when the network still sorts at no higher cost ---------------------
def bit_slices(x, k=K):
    """the states as k rows of bits (64 states per word): min = and, max = or"""
    n = -(-len(x) // 64) * 64
    rows = []
    for i in range(k):
        bits = np.zeros(n, dtype=np.uint8)
        bits[: len(x)] = (x >> np.uint32(i)) & 1
        rows.append(np.packbits(bits).view(np.uint64))
    return np.array(rows)


def sorts_sliced(ops, rows):
    c = rows.copy()
    for op in ops:
        if len(op) == 2:
            a, b = op
            x, y = c[a], c[b]
            c[a], c[b] = x & y, x | y
        else:
            x, y, z = c[op[0]], c[op[1]], c[op[2]]
            lo, hi = x & y, x | y
            c[op[0]], c[op[1]], c[op[2]] = lo & z, lo | (hi & z), hi | z
    return not (c[:-1] & ~c[1:]).any()


def local_search(ops, start, n_fixed, iters, rng, k=K, log=None):
    """edits: delete an operation, narrow a 3-sorter to a compare-exchange, change one register of an operation, swap
    neighbours, move an operation, widen a compare-exchange to a 3-sorter while deleting another operation.  An edit is kept
    when the network still sorts and costs no more (equal cost: a neutral step, which is what lets the search drift off a
    local minimum).  Returns the cheapest network seen, the shallowest among equals."""
    rows = bit_slices(run(ops[:n_fixed], np.unique(start)), k)
    fixed, cur = list(ops[:n_fixed]), list(ops[n_fixed:])
    best, best_key = list(cur), (cost(cur), depth(fixed + cur, k))
    for it in range(iters):
        new = list(cur)
        i = int(rng.integers(len(new)))
        r = rng.random()
        if r < 0.25:
            del new[i]
        elif r < 0.40:
            if len(new[i]) == 2:
                continue
            j = int(rng.integers(3))
            new[i] = tuple(v for t, v in enumerate(new[i]) if t != j)
        elif r < 0.65:
            regs = list(new[i])
            regs[int(rng.integers(len(regs)))] = int(rng.integers(k))
            if len(set(regs)) != len(regs):
                continue
            new[i] = tuple(sorted(regs))
        elif r < 0.80:
            if i + 1 >= len(new):
                continue
            new[i], new[i + 1] = new[i + 1], new[i]
        elif r < 0.90:
            op = new.pop(i)
            new.insert(int(rng.integers(len(new) + 1)), op)
        else:
            j = int(rng.integers(len(new)))
            c = int(rng.integers(k))
            if len(new[i]) != 2 or j == i or c in new[i]:
                continue
            new[i] = tuple(sorted(new[i] + (c,)))
            del new[j]
        if cost(new) > cost(cur) or not sorts_sliced(new, rows):
            continue
        cur = new
        key = (cost(cur), depth(fixed + cur, k))
        if key < best_key:
            best, best_key = list(cur), key
            if log:
                log(f"  edit {it:7d}: {cost(fixed) + key[0]} instructions, depth {key[1]}")
    return fixed + best


def merger_job(job):
    seed, beam, iters = job
    rng = np.random.default_rng(seed)
    cyc = cyclic_bitonic_states(K)
    net = tighten(beam_search(cyc, [], beam, rng), cyc, 0)
    net = local_search(net, cyc, 0, iters, rng)
    return layered(tighten(net, cyc, 0))


def layered(ops, k=K):
    """the same operations, stably reordered layer by layer (an operation's layer = its depth): independent operations
    next to each other, every register's operations in their own order"""
    d = [0] * k
    keyed = []
    for i, op in enumerate(ops):
        t = max(d[r] for r in op) + 1
        for r in op:
            d[r] = t
        keyed.append((t, i, op))
    return [op for _, _, op in sorted(keyed)]


# ---- today's constructions, for the report ---------------------------------------------------------------------------------
def old_sorter(k=K):
    return [tuple(p) for p in nets.batcher(k)]


def old_merger(k=K, base=0):
    if k <= 1:
        return []
    if k % 2 == 0:
        h = k // 2
        return [(base + i, base + i + h) for i in range(h)] + old_merger(h, base) + old_merger(h, base + h)
    if k == 3:
        return [(base, base + 1, base + 2)]
    if k == 5:
        return [(base, base + 2), (base + 1, base + 3), (base, base + 1, base + 4), (base + 2, base + 3, base + 4)]
    return [(base + a, base + b) for a, b in nets.batcher(k)]


# ---- the generated header ------------------------------------------------------------------------------------------------
def emit(name, ops):
    out, line = [], "   "
    for op in ops:
        s = f" c.add({op[0]}, {op[1]});" if len(op) == 2 else f" c.add3({op[0]}, {op[1]}, {op[2]});"
        if len(line) + len(s) > 120:
            out.append(line)
            line = "   "
        line += s
    out.append(line)
    return f"constexpr void {name}(CmpList& c) {{\n" + "\n".join(out) + "\n}\n"


def write_header(sorter, merger, beams, path=HEADER):
    text = f"""// GENERATED by tools/dev/search_nets.py (seed {SEED}, beams {beams[0]} / {beams[1]}); do not edit -- run the tool again.
// The K = 20 networks of sd_wsort.h under the cost model of the ISA: compare-exchange 2 instructions, 3-sorter 3.
//   sorter of 20 keys:                              {cost(sorter):3d} instructions in {len(sorter)} operations, depth {depth(sorter)}   (Batcher pruned: {cost(old_sorter())}, depth {depth(old_sorter())})
//   sorter of the cyclic-bitonic sequences of 20:   {cost(merger):3d} instructions in {len(merger)} operations, depth {depth(merger)}   (half-cleaners + 5-nets: {cost(old_merger())}, depth {depth(old_merger())})
// Included by sd_wsort.h behind the definition of CmpList; tests/wsort_nets20_check.cpp proves both by the 0-1 principle.
#pragma once

namespace sdws {{

constexpr int kSortNet20Cost = {cost(sorter)}, kBitonicNet20Cost = {cost(merger)};

{emit("sort_net20_into", sorter)}
{emit("bitonic_net20_into", merger)}
}}  // namespace sdws
"""
    with open(path, "w") as f:
        f.write(text)


def read_header():
    text = open(HEADER).read()
    res = []
    for name in ("sort_net20_into", "bitonic_net20_into"):
        body = text.split(f"void {name}(CmpList& c) {{")[1].split("}")[0]
        res.append([tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"c\.add3?\(([^)]*)\)", body)])
    return res


def report(sorter, merger):
    full, cyc = all_states(K), cyclic_bitonic_states(K)
    assert len(cyc) == 382
    for what, old, new, start in (("sorter", old_sorter(), sorter, full), ("merger", old_merger(), merger, cyc)):
        for tag, ops in (("today", old), ("searched", new)):
            ok = sorts(ops, start)
            n3 = sum(len(op) == 3 for op in ops)
            print(f"{what:7s} {tag:9s}: {cost(ops):3d} instructions, {len(ops) - n3:3d} compare-exchanges + {n3:2d} 3-sorters, depth {depth(ops):2d}, "
                  f"{'sorts all ' + str(len(start)) + ' inputs' if ok else 'DOES NOT SORT'}")
            assert ok
    per_sort = lambda s, m: cost(s) + 6 * cost(m)
    print(f"local part of one sort: {per_sort(old_sorter(), old_merger())} -> {per_sort(sorter, merger)} instructions")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="verify and report the committed header, search nothing")
    ap.add_argument("--beam-sorter", type=int, default=4)
    ap.add_argument("--beam-merger", type=int, default=48)
    ap.add_argument("--iters-sorter", type=int, default=150000, help="edits of the local search behind the beam search")
    ap.add_argument("--iters-merger", type=int, default=300000)
    ap.add_argument("--restarts-merger", type=int, default=24, help="independent merger searches, the best one is kept")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--out", default=HEADER, help="the header to write")
    args = ap.parse_args()
    if args.check:
        report(*read_header())
        return
    log = None if args.quiet else print
    rng = np.random.default_rng(SEED)
    t0 = time.time()
    first = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(6)] + [(18, 19)]
    print(f"sorter: beam {args.beam_sorter}")
    sorter = beam_search(all_states(K), first, args.beam_sorter, rng, log=log)
    sorter = tighten(sorter, all_states(K), len(first))
    print(f"  beam: {cost(sorter)} instructions, depth {depth(sorter)}, {time.time() - t0:.0f} s")
    sorter = local_search(sorter, all_states(K), len(first), args.iters_sorter, rng, log=log)
    sorter = layered(tighten(sorter, all_states(K), len(first)))
    print(f"  -> {cost(sorter)} instructions, depth {depth(sorter)}, {time.time() - t0:.0f} s")
    print(f"merger: {args.restarts_merger} x (beam {args.beam_merger} + local search)")
    # the merger runs six times per sort and its problem is tiny: several independent searches, each with a seed of its own,
    # side by side; the cheapest wins, the shallowest among equals, the lowest seed among those
    jobs = [(SEED + 1 + r, args.beam_merger, args.iters_merger) for r in range(args.restarts_merger)]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        found = pool.map(merger_job, jobs)
    for (seed, _, _), cand in zip(jobs, found):
        print(f"  seed {seed}: {cost(cand)} instructions, depth {depth(cand)}")
    merger = min(found, key=lambda m: (cost(m), depth(m)))
    print(f"  -> {cost(merger)} instructions, depth {depth(merger)}, {time.time() - t0:.0f} s")
    report(sorter, merger)
    write_header(sorter, merger, (args.beam_sorter, args.beam_merger), args.out)
    print("wrote", os.path.relpath(args.out, ROOT))


if __name__ == "__main__":
    main()
