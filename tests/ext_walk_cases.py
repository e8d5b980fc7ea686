"""Planted k1-mer graphs and a sequential reference for the walks of the contig extension (csrc/extend.hip: the thread walker and its
hand-over after 16 steps, the wavefront walker with its 64-step memo chunks, the claim logs, the rank blocks, the marks, the audit;
csrc/ext_results.hip: the readers).

Plain numpy: nothing here loads the library.  walk_reference is the seed loop of oracle/extension.py:python_walks restated on the
oriented ids of ext_setup_cases.reference: seeds in ref.order; a seed that an earlier walk owns makes its walk void (n_right =
0xFFFFFFFF, n_left = 0, tot_weight = 0: what ext_walk_kernel leaves of a void walk); else right over rows[o][0:4], then left over
rows[o][4:8], each step to the heaviest candidate that exists and is unowned, ties in the order A, G, C, T with a strict >, and
every step claims its k1-mer.

The tables are made from strings: plant() puts every k1-window of a sequence into a dict with a weight (canonicalised for a
canonical table; a later plant overwrites an earlier one), so that the path of every walk is known before it is run --

  lengths_<k>_<fwd|canon>   a sequence per (a, b): the walk seeded b windows in runs a steps right and b steps left -- around the
                            hand-over (15, 16, 17), the memo chunk (63, 64, 65), two chunks and a walk of 1000
  chain_<fwd|canon>         walk i takes its detour, and claims the tip of walk i + 1, only because walk i - 1 claimed its own tip: a
                            dependency chain of depth 40
  loops_<fwd|canon>         a circle, a tail into a circle, a hairpin (through a palindrome on a canonical table), a 2-cycle
  dense_<k>_<fwd|canon>     every k1-mer at k = 6, 7: four candidates at every step, most decisions and seed ranks are ties
  heavy                     every count 2^32 - 1, a palindrome among them: totals beyond 2^35
  seeds_<n>, empty, no_seed seed counts around a 64-lane block and the first rank block of 4,096

-- each made on demand from a seed of its own and cached.  Shared by tests/test_ext_walk_cases.py (CPU: the reference against the
oracle, the cases hold what they are for), tests/test_ext_walks_gpu.py and its child tests/ext_walks_poison_worker.py."""
from collections import namedtuple
from functools import lru_cache
import numpy as np
import ext_setup_cases as ec
from ext_setup_cases import ALPHA, NONE32, Table, _rng, _table, mask_of

Walks = namedtuple("Walks", "n_right n_left tot_weight paths contigs depth owner")
TIE_ORDER = (0, 2, 1, 3)                                              # A, G, C, T as codes of ACGT (extension_correction.py:10)


def walk_reference(ref, k):
    """the walks of a table whose set-up is `ref` (ext_setup_cases.reference), rank by rank: n_right, n_left (uint32), tot_weight
    (uint64), the path of oriented ids (seed, right steps, left steps; empty for a void walk), the contig (None for a void walk), the
    dependency depth (0: the walk met no claim of another walk; else 1 + the largest depth among the walks whose claims it met, at its
    seed or as a candidate) and, per oriented id, the rank that owns it or -1"""
    rows = ref.rows.tolist()
    w = np.repeat(ref.weight, 2).tolist()
    strings = ref.strings.tolist()
    owner = [-1] * len(rows)
    ns = len(ref.order)
    n_right, n_left, tot = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32), np.zeros(ns, np.uint64)
    paths, contigs, depth = [], [], []
    for rank, seed in enumerate(ref.order.tolist()):
        if owner[seed] >= 0:
            n_right[rank] = NONE32
            paths.append([]), contigs.append(None), depth.append(1 + depth[owner[seed]])
            continue
        owner[seed] = rank
        met, total, sides = set(), w[seed], ([], [])
        for side, first in zip(sides, (0, 4)):
            cur = seed
            while True:
                best, best_w = -1, -1
                for b in TIE_ORDER:
                    c = rows[cur][first + b]
                    if c < 0:
                        continue
                    if owner[c] >= 0:
                        if owner[c] != rank:
                            met.add(owner[c])
                    elif w[c] > best_w:
                        best, best_w = c, w[c]
                if best < 0:
                    break
                owner[best] = rank
                side.append(best)
                total += best_w
                cur = best
        right, left = sides
        n_right[rank], n_left[rank], tot[rank] = len(right), len(left), total
        paths.append([seed] + right + left)
        contigs.append("".join(ALPHA[strings[o] >> (2 * (k - 1))] for o in reversed(left)) + ec.str_of(strings[seed], k) +
                       "".join(ALPHA[strings[o] & 3] for o in right))
        depth.append(1 + max(depth[r] for r in met) if met else 0)
    return Walks(n_right, n_left, tot, paths, contigs, depth, np.array(owner, dtype=np.int64))


def live_of(walks):
    """ranks of the walks that are not void"""
    return np.flatnonzero(walks.n_right != NONE32)


# ---------------------------------------------------------------- tables from strings
def rc_str(s):
    return "".join(ALPHA[3 - ALPHA.index(c)] for c in reversed(s))


def rnd(rng, n):
    return "".join(ALPHA[c] for c in rng.integers(0, 4, n).tolist())


def windows(seq, k):
    """the packed keys of all k-windows of a string, in order"""
    out, v, m = [], 0, mask_of(k)
    for i, c in enumerate(seq):
        v = ((v << 2) | ALPHA.index(c)) & m
        if i >= k - 1:
            out.append(v)
    return out


def _canon(v, k):
    r, x = 0, v
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return min(v, r)


def plant(d, seq, k, canonical, weight):
    """every k-window of seq into d with this count (the canonical key for a canonical table); overwrites"""
    for v in windows(seq, k):
        d[_canon(v, k) if canonical else v] = weight


def _table_of(d, k, canonical, rng):
    keys = np.array(list(d.keys()), dtype=np.uint64)
    counts = np.array(list(d.values()), dtype=np.uint64)
    p = rng.permutation(len(keys))
    return _table(keys[p], counts[p], k, canonical)


A_STEPS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000)
B_STEPS = (0, 1, 15, 16, 17, 64, 129)
LENGTH_PAIRS = tuple((a, b) for a in A_STEPS for b in B_STEPS)
LENGTH_KMERS = sum(a + b + 1 for a, b in LENGTH_PAIRS)              # 15,278
LENGTHS = tuple("lengths_%d_%s" % (k, c) for k in (26, 32, 31, 20) for c in ("fwd", "canon"))
CHAINS = ("chain_fwd", "chain_canon")
CHAIN_D = 40
LOOPS = ("loops_fwd", "loops_canon")
DENSE = ("dense_6_fwd", "dense_6_canon", "dense_7_fwd", "dense_7_canon", "dense_6_canon_one_count")
HEAVY = "heavy"
SEED_COUNTS = (1, 63, 64, 65, 4095, 4096, 4097)
SEEDS = tuple("seeds_%d" % n for n in SEED_COUNTS) + ("empty", "no_seed")
# (name, min_weight) of every run; chain_* also with only the planted seeds as seeds
CASES = tuple((n, 3) for n in LENGTHS + CHAINS + LOOPS + DENSE + (HEAVY,) + SEEDS) + (("chain_fwd", 100), ("chain_canon", 100))


def _kind(name):
    return name.endswith("canon") or "_canon_" in name


def _lengths(name):
    """a random sequence of k + a + b bases per (a, b), every window of count 5, the one at offset b of count 100000 - i: walk i is
    seeded there, runs a steps to the right and b to the left; on a canonical table the other strand gives the mirror (b, a)"""
    k, canonical = int(name.split("_")[1]), _kind(name)
    rng = _rng("walk:" + name)
    d = {}
    for i, (a, b) in enumerate(LENGTH_PAIRS):
        seq = rnd(rng, k + a + b)
        plant(d, seq, k, canonical, 5)
        plant(d, seq[b:b + k], k, canonical, 100000 - i)
    return _table_of(d, k, canonical, rng)


def chain_parts(name):
    """(tips T_0 .. T_D, starts A_i, detours R_i) of a chain table"""
    k = 26
    rng = _rng("walk:" + name)
    tips = [rnd(rng, k) for _ in range(CHAIN_D + 1)]
    starts, detours = [], []
    for i in range(CHAIN_D):
        a = rnd(rng, 9) + ALPHA[i % 4] + tips[i][:-1]
        other = ALPHA[(ALPHA.index(tips[i][-1]) + 1 + int(rng.integers(0, 3))) & 3]
        starts.append(a)
        detours.append(a[-k:][1:] + other + rnd(rng, 12) + ALPHA[(i + 2) % 4] + tips[i + 1])
    return tips, starts, detours


def _chain(name):
    """walk i (seeded at the first window of A_i, count 1000 - i) comes after 9 steps to the predecessor of its tip T_i (count 9) and
    of its detour R_i (count 4, 40 k1-mers, the last of them T_(i + 1)): it takes the tip unless walk i - 1 has claimed it.  T_0 is
    not in the table, so walk 0 takes its detour, and so does every walk after it, each only because of the one before"""
    k, canonical = 26, _kind(name)
    tips, starts, detours = chain_parts(name)
    d = {}
    for i in range(CHAIN_D):
        plant(d, detours[i], k, canonical, 4)
    for i in range(CHAIN_D):
        plant(d, starts[i], k, canonical, 5)
        plant(d, starts[i][:k], k, canonical, 1000 - i)
    for i in range(1, CHAIN_D + 1):
        plant(d, tips[i], k, canonical, 9)
    return _table_of(d, k, canonical, _rng("walk:order:" + name))


LoopParts = namedtuple("LoopParts", "circle rho hairpin two_cycle")
CIRCLE, RHO_TAIL, RHO_CIRCLE, HAIRPIN_HALF = 300, 99, 200, 150


def loop_parts(name):
    """the four sequences of a loops table: a circle of 300 k1-mers (c + c[:k - 1]); a tail of 99 k1-mers (the seed among them) into a
    circle of 200, 299 k1-mers and so 298 steps; the hairpin h + rc(h), |h| = 150, of 275 k1-mers, the middle one a palindrome; an
    entry path of 20 k1-mers into the 2-cycle ACAC... / CACA..."""
    k = 26
    rng = _rng("walk:" + name)
    c = rnd(rng, CIRCLE)
    t, c2 = rnd(rng, RHO_TAIL), rnd(rng, RHO_CIRCLE)
    h = rnd(rng, HAIRPIN_HALF)
    return LoopParts(c + c[:k - 1], t + c2 + c2[:k - 1], h + rc_str(h), rnd(rng, 19) + "G" + ("AC" * k)[:k + 1])


def _loops(name):
    k, canonical = 26, _kind(name)
    d = {}
    for seq, seed_count in zip(loop_parts(name), (900, 800, 700, 5)):
        plant(d, seq, k, canonical, 5)
        plant(d, seq[:k], k, canonical, seed_count)
    return _table_of(d, k, canonical, _rng("walk:order:" + name))


def _dense(name):
    """every k1-mer (the canonical ones for `canon`) in a random order, counts 1 .. 6 (all 6 for one_count)"""
    k, canonical = int(name.split("_")[1]), _kind(name)
    rng = _rng("walk:" + name)
    keys = np.arange(1 << (2 * k), dtype=np.uint64)
    if canonical:
        keys = keys[keys == ec.canonical_of(keys, k)]
    keys = rng.permutation(keys)
    counts = np.full(len(keys), 6) if name.endswith("one_count") else rng.integers(1, 7, size=len(keys))
    return _table(keys, counts, k, canonical)


HEAVY_PATH = 12


def heavy_parts():
    """three sequences of 12 k1-mers each; the window at offset 5 of the first is a palindrome"""
    k = 26
    rng = _rng("walk:heavy")
    half = rnd(rng, k // 2)
    return (rnd(rng, 5) + half + rc_str(half) + rnd(rng, HEAVY_PATH - 6), rnd(rng, k + HEAVY_PATH - 1), rnd(rng, k + HEAVY_PATH - 1))


def _heavy():
    d = {}
    for seq in heavy_parts():
        plant(d, seq, 26, True, NONE32)
    return _table_of(d, 26, True, _rng("walk:order:heavy"))


def _seeds(name):
    """a forward table with exactly n seeds at min_weight 3: every third starts a private path of three k1-mers of count 1 (walked,
    but no seeds), the others are isolated k1-mers (walks of no step); no_seed: 50 k1-mers of counts 1 and 2"""
    k = 26
    rng = _rng("walk:" + name)
    d = {}
    if name == "no_seed":
        for i in range(50):
            plant(d, rnd(rng, k), k, False, 1 + i % 2)
    elif name != "empty":
        for i in range(int(name.split("_")[1])):
            seq = rnd(rng, k + (3 if i % 3 == 0 else 0))
            plant(d, seq, k, False, 1)
            plant(d, seq[:k], k, False, int(rng.integers(3, 9)))
    return _table_of(d, k, False, rng)


@lru_cache(maxsize=None)
def table(name):
    if name in LENGTHS:
        return _lengths(name)
    if name in CHAINS:
        return _chain(name)
    if name in LOOPS:
        return _loops(name)
    if name in DENSE:
        return _dense(name)
    if name == HEAVY:
        return _heavy()
    if name in SEEDS:
        return _seeds(name)
    raise KeyError(name)


@lru_cache(maxsize=None)
def expected(name, min_weight=3):
    """(Ref, Walks) of a case's table in the order it was made in -- the CPU tests' view; the GPU tests compute both again from the
    downloaded table, whose order is the library's"""
    t = table(name)
    ref = ec.reference(t.keys, t.counts, t.k, t.canonical, min_weight)
    return ref, walk_reference(ref, t.k)
