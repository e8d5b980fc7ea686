"""Tables and a brute-force reference for the set-up of the contig extension (csrc/k1dict.hip, csrc/extend.hip: ext_prepare_kernel,
fd_build_kernel / fd_match, ext_records_kernel, ext_seed_kernel, the two seed sorts, ext_seed_rank_kernel).

Plain numpy: nothing here loads the library.  The reference is written from the definition (extension_correction.py:202-245, 334 of
the project this one follows; oracle/extension.py restates it): a k1-mer table (keys, counts, k, canonical) stands for the strings of
a strand-doubled input --

  flags       bit 0: the table is canonical and the key is its own reverse complement; bit 1: the most frequent base occurs >= k - 2
              times (low complexity: load_kmers drops the k1-mer)
  weight      the count, twice that for a palindrome (both strands give the same string), clamped to 2^32 - 1
  oriented id o = 2 i + s: the string of key i (s = 0) or its reverse complement (s = 1); orientation 1 exists on canonical tables
              only, and only for k1-mers that are neither palindromes nor low-complexity
  rows        R[o][b] / L[o][b]: the oriented id of string(o)[1:] + b / b + string(o)[:-1] -- 2 j if key j is that string, 2 j + 1 if
              key j is its reverse complement, -1 if there is no such key or it is low-complexity; all -1 for a low-complexity
              k1-mer and for an orientation that does not exist
  seeds       the orientations that exist, are not low-complexity and weigh >= min_weight, ordered by (weight descending, string
              ascending); seed_rank is the inverse of that order, 0xFFFFFFFF elsewhere

-- each looked up with np.searchsorted over the sorted keys.  The cases are the tables at which the set-up takes another way: sizes
around a group of eight lanes, a wavefront and a block of 1024; a grid that strides; every k1-mer at small k; k1 = 32, 31, 20 with
planted palindromes, low-complexity boundaries, full rows, a self-loop and a 2-cycle; weights around 2^31 and 2^32; a dictionary with
lines that overflow four times in a row.  Every case is made on demand from a seed of its own and cached.

Shared by tests/test_ext_setup_cases.py (CPU: the reference against the oracle, the cases hold what they are for) and
tests/test_ext_setup_gpu.py."""
import zlib
from collections import namedtuple
from functools import lru_cache
import numpy as np
from primitives_cases import fmix64, bucket_of, start_bits

U64 = np.uint64
NONE32 = 0xFFFFFFFF
FD_SLOTS, FD_PER_LINE, FD_HOPS, FD_PAL = 10, 4, 4, 0x80000000        # csrc/k1dict.h
ALPHA = "ACGT"

Table = namedtuple("Table", "keys counts k canonical")
Ref = namedtuple("Ref", "flags weight strings exists alive rows order seed_rank")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _frozen(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def mask_of(k):
    return (1 << (2 * k)) - 1


def key_of(s):
    v = 0
    for c in s:
        v = (v << 2) | ALPHA.index(c)
    return v


def str_of(key, k):
    key = int(key)
    return "".join(ALPHA[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp(keys, k):
    """reverse complements of packed k-mers (2 bits a base, the first base in the high bits)"""
    keys = np.array(keys, dtype=np.uint64, copy=True)
    out = np.zeros(keys.shape, dtype=np.uint64)
    for _ in range(k):
        out = (out << U64(2)) | (U64(3) - (keys & U64(3)))
        keys >>= U64(2)
    return out


def canonical_of(keys, k):
    keys = np.asarray(keys, dtype=np.uint64)
    return np.minimum(keys, revcomp(keys, k))


def max_base_count(keys, k):
    """how often the most frequent base of each k-mer occurs"""
    keys = np.asarray(keys, dtype=np.uint64)
    cnt = np.zeros((4,) + keys.shape, dtype=np.int64)
    for j in range(k):
        b = (keys >> U64(2 * j)) & U64(3)
        for v in range(4):
            cnt[v] += b == U64(v)
    return cnt.max(axis=0)


def low_complexity(keys, k):
    return max_base_count(keys, k) >= k - 2


# ---------------------------------------------------------------- the reference
def reference(keys, counts, k, canonical, min_weight):
    """everything the set-up makes of a table whose keys stand in this order (the order of shn_table_download: i is an index into it)"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    n = len(keys)
    assert len(np.unique(keys)) == n, "the keys of a table are distinct"
    rc = revcomp(keys, k)
    pal = (rc == keys) if canonical else np.zeros(n, bool)
    lc = low_complexity(keys, k)
    flags = (pal.astype(np.uint8) | (lc.astype(np.uint8) << 1)).astype(np.uint8)
    weight = np.minimum(counts.astype(np.uint64) * np.where(pal, U64(2), U64(1)), U64(NONE32)).astype(np.uint32)
    strings = np.empty(2 * n, dtype=np.uint64)
    strings[0::2], strings[1::2] = keys, rc
    exists = np.zeros(2 * n, bool)
    exists[0::2] = True
    exists[1::2] = (~pal & ~lc) if canonical else False
    alive = exists & ~np.repeat(lc, 2)

    by_key = np.argsort(keys)
    sorted_keys = keys[by_key]

    def oriented_id(x):
        """of the strings x: 2 j (key j is the string), 2 j + 1 (key j is its reverse complement), -1 (neither, or low complexity)"""
        if n == 0:
            return np.full(x.shape, -1, np.int64)
        if canonical:
            r = revcomp(x, k)
            c, strand = np.minimum(x, r), (r < x).astype(np.int64)
        else:
            c, strand = x, np.zeros(x.shape, np.int64)
        pos = np.minimum(np.searchsorted(sorted_keys, c), n - 1)
        j = by_key[pos]
        return np.where((sorted_keys[pos] == c) & ~lc[j], 2 * j + strand, -1)

    rows = np.full((2 * n, 8), -1, dtype=np.int32)
    m = U64(mask_of(k))
    for b in range(4):
        rows[:, b] = oriented_id(((strings << U64(2)) | U64(b)) & m)
        rows[:, 4 + b] = oriented_id((strings >> U64(2)) | U64(b << (2 * (k - 1))))
    rows[~alive] = -1

    w2 = np.repeat(weight, 2)
    seeds = np.flatnonzero(alive & (w2 >= min_weight))
    order = seeds[np.lexsort((strings[seeds], U64(NONE32) - w2[seeds].astype(np.uint64)))].astype(np.uint32)
    seed_rank = np.full(2 * n, NONE32, dtype=np.uint32)
    seed_rank[order] = np.arange(len(order), dtype=np.uint32)
    return Ref(flags, weight, strings, exists, alive, rows, order, seed_rank)


def dumped_items(table):
    """what the oracle's load_kmers reads of a table: (string, count) of the strand-doubled input -- a canonical key and its reverse
    complement with the key's count, a palindrome once with twice the count; in descending string order (the order the extension tests
    feed the oracle in: its stable sort by weight, popped from the end, then walks ties in ascending string order)"""
    items = {}
    for key, c in zip(table.keys.tolist(), table.counts.tolist()):
        s = str_of(key, table.k)
        if table.canonical:
            r = str_of(int(revcomp(np.array([key], np.uint64), table.k)[0]), table.k)
            items[s] = items.get(s, 0) + c
            items[r] = items.get(r, 0) + c
        else:
            items[s] = c
    return [(s, items[s]) for s in sorted(items, reverse=True)]


# ---------------------------------------------------------------- tables
def _random_keys(rng, n, k, canonical, avoid=()):
    """n distinct random k-mers that are not low-complexity (canonical ones on request), none of them in `avoid`"""
    out, seen = [], set(int(a) for a in avoid)
    while len(out) < n:
        x = rng.integers(0, 1 << 64, size=2 * (n - len(out)) + 16, dtype=np.uint64) & U64(mask_of(k))
        if canonical:
            x = canonical_of(x, k)
        x = x[~low_complexity(x, k)]
        for v in x.tolist():
            if v not in seen:
                seen.add(v)
                out.append(v)
                if len(out) == n:
                    break
    return np.array(out, dtype=np.uint64)


def _table(keys, counts, k, canonical):
    keys = np.asarray(keys, dtype=np.uint64)
    assert len(np.unique(keys)) == len(keys)
    if canonical:
        assert np.array_equal(keys, canonical_of(keys, k))
    return Table(_frozen(keys, np.uint64), _frozen(counts, np.uint32), k, canonical)


SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 5000)
SIZE_RUNS = tuple(("size_%d" % n, 3) for n in SIZES) + (("size_5000", 1), ("size_5000", 7))
TAIL_N = 70001
TAIL_BLOCKS = (1, 3, 64)
SMALL_K = ("all_4_fwd", "all_5_fwd", "half_4", "half_5", "half_6")
EDGE_K = tuple("edge_%d_%s" % (k, c) for k in (32, 31, 20) for c in ("canon", "fwd"))
WEIGHTS = ("weights_extreme", "weights_one_count", "weights_bit31")
COLLIDE = "collide"
LAYOUT1 = ((20, True), (21, True), (26, True), (31, True), (32, True), (26, False), (31, False))


def _sized(name, n):
    rng = _rng("ext:" + name)
    keys = _random_keys(rng, n, 26, True)
    return _table(keys, rng.integers(1, 7, size=n), 26, True)


def _small_k(name):
    kind, k = name.split("_")[:2]
    k = int(k)
    keys = np.arange(1 << (2 * k), dtype=np.uint64)
    canonical = kind == "half"
    if canonical:
        keys = keys[keys == canonical_of(keys, k)]
    keys = _rng("ext:" + name).permutation(keys)
    return _table(keys, 1 + (keys % U64(6)), k, canonical)


def _with_bases(k, base, others):
    """the homopolymer of `base` with len(others) bases replaced, spread over the string (its ends included)"""
    s = [ALPHA[base]] * k
    where = [0, k - 1, k // 2][:len(others)]
    for p, o in zip(where, others):
        s[p] = ALPHA[o]
    return key_of("".join(s))


def edge_plants(k, canonical):
    """{name: [string keys]}: what an edge table holds on purpose (canonicalised for a canonical table where the table stores them)"""
    rng = _rng("ext:plants:%d" % k)
    plants = {"homopolymers": [0, mask_of(k)]}
    for b in range(4):
        o = [(b + 1) & 3, (b + 2) & 3, (b + 3) & 3]
        plants["k-3 of %s" % ALPHA[b]] = [_with_bases(k, b, o)]
        plants["k-2 of %s" % ALPHA[b]] = [_with_bases(k, b, o[:2])]
    if k % 2 == 0:
        half = rng.integers(0, 1 << 64, size=10, dtype=np.uint64) & U64(mask_of(k // 2))
        plants["palindromes"] = [(int(h) << k) | int(r) for h, r in zip(half, revcomp(half, k // 2))]
    else:
        # k odd: C + a palindrome of k - 1 bases: its successor by G is its own reverse complement
        h = int(rng.integers(0, 1 << 62, dtype=np.uint64)) & mask_of((k - 1) // 2)
        pal = (h << (k - 1)) | int(revcomp(np.array([h], np.uint64), (k - 1) // 2)[0])
        plants["turns into its reverse complement"] = [(1 << (2 * (k - 1))) | pal]
    ac = key_of(("AC" * k)[:k])
    plants["2-cycle"] = [ac, key_of(("CA" * k)[:k])]
    return plants


def _edge(name):
    _, k, kind = name.split("_")
    k, canonical = int(k), kind == "canon"
    rng = _rng("ext:" + name)
    m = mask_of(k)
    base = _random_keys(rng, 3000, k, canonical)
    strings = [int(v) for v in base]
    for v in base[::10].tolist():                                     # a tenth of the keys: all four successors, all four predecessors
        for b in range(4):
            strings.append(((v << 2) | b) & m)
            strings.append((v >> 2) | (b << (2 * (k - 1))))
    for group in edge_plants(k, canonical).values():
        strings += group
    keys = np.array(strings, dtype=np.uint64)
    if canonical:
        keys = canonical_of(keys, k)
    keys = rng.permutation(np.unique(keys))
    return _table(keys, rng.integers(1, 7, size=len(keys)), k, canonical)


def _palindromes(rng, n, k):
    half = np.unique(rng.integers(0, 1 << 62, size=2 * n, dtype=np.uint64) & U64(mask_of(k // 2)))[:n]
    assert len(half) == n
    return (half << U64(k)) | revcomp(half, k // 2)


EXTREME_COUNTS = (1, 2, 3, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF)


def _weights(name):
    rng = _rng("ext:" + name)
    k = 26
    if name == "weights_extreme":
        # every count on three palindromes and on three other k1-mers
        reps = 3 * len(EXTREME_COUNTS)
        pal = _palindromes(rng, reps, k)
        other = _random_keys(rng, reps, k, True, avoid=pal)
        keys = np.concatenate([pal, other])
        counts = np.tile(np.repeat(np.array(EXTREME_COUNTS, dtype=np.uint64), 3), 2)
    elif name == "weights_one_count":
        keys = _random_keys(rng, 2000, k, True)
        counts = np.full(2000, 6)
    else:
        # counts that differ in bit 31 alone: as sort keys over 31 bits they tie
        keys = _random_keys(rng, 600, k, True)
        low = rng.integers(3, 9, size=600).astype(np.uint64)
        counts = low | (rng.integers(0, 2, size=600).astype(np.uint64) << U64(31))
    p = rng.permutation(len(keys))
    return _table(keys[p], counts[p], k, True)


@lru_cache(maxsize=None)
def table(name):
    if name.startswith("size_"):
        return _sized(name, int(name[5:]))
    if name == "tail":
        return _sized(name, TAIL_N)
    if name in SMALL_K:
        return _small_k(name)
    if name in EDGE_K:
        return _edge(name)
    if name in WEIGHTS:
        return _weights(name)
    if name == COLLIDE:
        return collision_case().table
    raise KeyError(name)


def default_adj_blocks(n):
    """the grid ext_records_kernel gets without SHN_EXT_ADJ_BLOCKS: eight lanes per k1-mer, 256 threads a block, 2^22 blocks at the most"""
    return min((8 * n + 255) // 256, 1 << 22)


# ---------------------------------------------------------------- the dictionary
def mulhi(a, b):
    """(a * b) >> 64 of a uint64 array and a number below 2^32"""
    a = np.asarray(a, dtype=np.uint64)
    assert 0 <= b < (1 << 32)
    return ((a >> U64(32)) * U64(b) + (((a & U64(NONE32)) * U64(b)) >> U64(32))) >> U64(32)


def hashed_lines(n):
    """lines the look-ups of a hashed table (layout 0) of n k1-mers start at; FD_HOPS spare lines follow them"""
    return n // FD_PER_LINE + 1


def home_lines(keys, n_lines):
    """fd_bucket for a hashed table: (mix64(key) * n_lines) >> 64"""
    return mulhi(fmix64(keys), n_lines).astype(np.int64)


def host_table_order(keys):
    """the order shn_table_create lays up to 2^22 distinct keys out in: by bucket (the top bits of mix64), ascending inside a bucket"""
    keys = np.asarray(keys, dtype=np.uint64)
    return np.lexsort((keys, bucket_of(keys, start_bits(len(keys)))))


def simulate_dictionary(keys, lc, n_lines):
    """one order the build may run in (table order, one k1-mer after the other): (count word of every line, line every k1-mer is stored
    in or -1).  The count words depend on that order only where a line overflows; what the tests take from here are lower bounds."""
    count = np.zeros(n_lines + FD_HOPS, dtype=np.int64)
    stored = np.full(len(keys), -1, dtype=np.int64)
    for i, home in enumerate(home_lines(keys, n_lines).tolist()):
        if lc[i]:
            continue
        for line in range(home, home + FD_HOPS):
            count[line] += 1
            if count[line] <= FD_SLOTS:
                stored[i] = line
                break
    return count, stored


Collision = namedtuple("Collision", "table lines L M last M2 M3 picked absent low_complexity")
COLLIDE_N = 4096
COLLIDE_HOMED = (("L", 0, 45), ("L", 1, 8), ("L", 3, 8), ("M", 0, 15), ("last", 0, 12), ("M2", 0, 20), ("M3", 0, 20))


@lru_cache(maxsize=None)
def collision_case():
    """4096 canonical 26-mers, 1025 hashed lines: 45 homed at one line L, 8 at L + 1 and at L + 3 (four full lines in a row: some key is
    stored nowhere), 15 at a line M (one hop), 12 at the last hashed line (hops into the spare lines); a predecessor and a successor of
    every such key, so that the records kernel looks each of them up from two rows; four low-complexity keys and three palindromes.
    And 20 keys each at two more lines M2 and M3.  A wavefront of the build makes its first attempts together, so the keys homed at
    L + 1 and L + 3 have their slots before a key of L hops there: of the first five groups 21 keys are stored away from home in
    the worst order and 23 on an MI355X, not the 30 the test asks for.  Ten of the 20 keys of M2 and of M3 hop in any order."""
    rng = _rng("ext:collide")
    k, n, lines = 26, COLLIDE_N, hashed_lines(COLLIDE_N)
    pool = _random_keys(rng, 150000, k, True)
    home = home_lines(pool, lines)
    where = {"L": 300, "M": 700, "last": lines - 1, "M2": 500, "M3": 900}
    picked, used = [], np.zeros(len(pool), bool)
    for name, d, cnt in COLLIDE_HOMED:
        idx = np.flatnonzero(home == where[name] + d)
        assert len(idx) >= cnt + 40, "the pool is too small for line %d" % (where[name] + d)
        picked += pool[idx[:cnt]].tolist()
        used[idx[:cnt]] = True
    m = mask_of(k)
    around = []
    for v in picked:
        b = int(rng.integers(0, 4))
        around += [((v << 2) | b) & m, (v >> 2) | (b << (2 * (k - 1)))]
    planted = [_with_bases(k, 0, [1, 2]), _with_bases(k, 1, [0, 2]), _with_bases(k, 0, [1]), 0]           # low complexity
    planted += _palindromes(rng, 3, k).tolist()
    fixed = np.unique(canonical_of(np.array(picked + around + planted, dtype=np.uint64), k))
    crowded = [where["L"] + d for d in range(4)] + [where["M"], where["last"]]
    absent = np.concatenate([pool[np.flatnonzero((home == l) & ~used)][:34] for l in crowded])[:200]
    pad = _random_keys(rng, n - len(fixed), k, True, avoid=np.concatenate([fixed, pool]))
    keys = rng.permutation(np.concatenate([fixed, pad]))
    assert len(keys) == n and len(absent) == 200 and not np.isin(absent, keys).any()
    t = _table(keys, rng.integers(1, 7, size=n), k, True)
    lc = keys[low_complexity(keys, k)]
    return Collision(t, lines, where["L"], where["M"], where["last"], where["M2"], where["M3"], _frozen(picked, np.uint64), _frozen(absent, np.uint64), _frozen(lc, np.uint64))


def expected_ids(table_keys, flags, queries):
    """the id word of every query: index | palindrome << 31 of the key that equals it, 0xFFFFFFFF if there is none or it is
    low-complexity (a Python dict over the downloaded keys)"""
    where = {key: i for i, key in enumerate(np.asarray(table_keys, dtype=np.uint64).tolist())}
    out = np.full(len(queries), NONE32, dtype=np.uint32)
    for qi, q in enumerate(np.asarray(queries, dtype=np.uint64).tolist()):
        i = where.get(q, -1)
        if i >= 0 and not (flags[i] & 2):
            out[qi] = i | (FD_PAL if flags[i] & 1 else 0)
    return out


# ---------------------------------------------------------------- reads for tables of the super-k-mer layout
def layout1_palindrome(k1):
    """a palindrome of k1 bases (k1 even) that is not low-complexity"""
    half = ("ACGGTCATTGCAAGTC" * 2)[:k1 // 2]
    return half + "".join(ALPHA[3 - ALPHA.index(c)] for c in reversed(half))


@lru_cache(maxsize=None)
def layout1_reads(k1):
    """~3,000 reads of 100 bases from a random sequence of 4,000, 1 % errors, with poly-A and poly-T reads and, at even k1, a palindrome
    of k1 bases in five reads (codes 0..3, uint8[reads, 100])"""
    rng = _rng("ext:layout1:%d" % k1)
    base = rng.integers(0, 4, 4000, dtype=np.uint8)
    starts = rng.integers(0, len(base) - 100, 3000)
    reads = base[starts[:, None] + np.arange(100)]
    err = rng.random(reads.shape) < 0.01
    reads = np.where(err, (reads + rng.integers(1, 4, reads.shape)) & 3, reads).astype(np.uint8)
    reads[:40] = 3
    reads[40:70] = 0
    if k1 % 2 == 0:
        pal = np.array([ALPHA.index(c) for c in layout1_palindrome(k1)], dtype=np.uint8)
        reads[70:75, 30:30 + k1] = pal
    return _frozen(reads, np.uint8)
