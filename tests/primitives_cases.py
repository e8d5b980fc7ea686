"""Inputs and checkers for the shared device primitives: the radix sort (csrc/sort.hip), the scan (shn_device_scan_u32, csrc/count.hip),
the runs of a sorted array (shn_sorted_runs, csrc/runs.hip), the three bucket searches of csrc/common.h and the table builds
(shn_table_create, shn_table_from_pairs).

Plain numpy: nothing here loads the library.  The references are np.argsort(kind="stable"), np.cumsum in uint64, np.flatnonzero of
the neighbours that differ, a Python dict and np.unique / np.add.at.  The inputs are the smallest at which each primitive takes another way: a wavefront's share of a sort tile
(1024), a tile (4096), a histogram longer than one scan block (5 tiles), more than 1024 scan block sums (2^20 elements), a final
bucket past the 950 distinct keys its LDS table takes.  Every case is made on demand from a seed of its own and cached.

Shared by tests/test_primitives_cases.py (CPU: the checkers reject wrong answers, the inputs are what they claim to be) and
tests/test_primitives_gpu.py."""
import zlib
from collections import namedtuple
from functools import lru_cache
import numpy as np

U64 = np.uint64
ALL64 = (1 << 64) - 1
TILE = 4096                      # items of a sort tile (STILE, csrc/sort.hip)
CAP_LIMIT = 950                  # distinct keys a final bucket's LDS table takes before the build tries again (csrc/count.hip)
PER_BUCKET = 96                  # shn_table_from_pairs / shn_table_create: bits = the first with (n >> bits) <= 96

SortCase = namedtuple("SortCase", "keys vals lo hi")
RunCase = namedtuple("RunCase", "keys shift")
TableCase = namedtuple("TableCase", "keys counts k canonical")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _u64(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def fmix64(x):
    """murmur3's 64-bit finaliser (shn_mix64, csrc/common.h) over a uint64 array"""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xff51afd7ed558ccd)
        x ^= x >> U64(33)
        x *= U64(0xc4ceb9fe1a85ec53)
        x ^= x >> U64(33)
    return x


def bucket_of(keys, bits):
    """shn_bucket_of: the top `bits` bits of fmix64(key)"""
    keys = np.asarray(keys, dtype=np.uint64)
    return (fmix64(keys) >> U64(64 - bits)).astype(np.int64) if bits else np.zeros(len(keys), np.int64)


def start_bits(n):
    """the bucket bits the table builds start with at n pairs"""
    bits = 0
    while bits < 23 and (n >> bits) > PER_BUCKET:
        bits += 1
    return bits


# ---------------------------------------------------------------- checkers
def range_mask(lo, hi):
    """the ones of a range of hi - lo bits (0 for an empty range)"""
    return ALL64 if hi - lo >= 64 else (1 << max(hi - lo, 0)) - 1


def masked(keys, lo, hi):
    """(key >> lo) & ((1 << (hi - lo)) - 1): what the sort orders by"""
    keys = np.asarray(keys, dtype=np.uint64)
    if hi <= lo:
        return np.zeros(len(keys), np.uint64)
    return (keys >> U64(lo)) & U64(range_mask(lo, hi))


def stable_order(keys, lo, hi):
    return np.argsort(masked(keys, lo, hi), kind="stable")


def rounded_hi(lo, hi):
    """where the passes of 8 bits end that cover [lo, hi)"""
    return lo + (hi - lo + 7) // 8 * 8 if hi > lo else hi


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %d elements, %d expected" % (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %d (%r, expected %r)" % (
        what, bad.size, want.size, int(bad[0]), got[bad[0]], want[bad[0]])


def check_sorted_pairs(keys_in, vals_in, keys_out, vals_out, lo, hi):
    """the output is exactly the stable sort of the input by the key bits [lo, hi): whole keys (bits outside the range untouched)
    and values in the order of np.argsort(kind="stable"); hi <= lo: the input"""
    keys_in, vals_in = np.asarray(keys_in, dtype=np.uint64), np.asarray(vals_in, dtype=np.uint32)
    order = stable_order(keys_in, lo, hi)
    _same("keys", np.asarray(keys_out, dtype=np.uint64), keys_in[order])
    _same("values", np.asarray(vals_out, dtype=np.uint32), vals_in[order])


def check_sorted_keys(keys_in, keys_out, lo, hi):
    """the same for the words alone"""
    keys_in = np.asarray(keys_in, dtype=np.uint64)
    _same("words", np.asarray(keys_out, dtype=np.uint64), keys_in[stable_order(keys_in, lo, hi)])


def check_scan(values, out, total):
    """out = the exclusive sums of the 32-bit values in 64 bits, n + 1 of them: out[0] = 0, out[n] = total"""
    values = np.asarray(values, dtype=np.uint32)
    want = np.zeros(len(values) + 1, dtype=np.uint64)
    np.cumsum(values.astype(np.uint64), out=want[1:])
    out = np.asarray(out)
    assert out.dtype == np.uint64, "the scan's output is 64 bits wide, not %s" % out.dtype
    _same("sums", out, want)
    assert int(total) == int(want[-1]), "total %d, expected %d" % (int(total), int(want[-1]))


def run_starts(keys, shift):
    """where the runs of equal (key >> shift) begin"""
    k = np.asarray(keys, dtype=np.uint64) >> U64(shift)
    if not len(k):
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero(np.r_[True, k[1:] != k[:-1]])


def check_runs(keys, shift, n_runs, run_keys, start, length, pos):
    """everything shn_sorted_runs gives: n_runs runs; run_keys[r] = the whole first key of run r; start[r] = its first element, with
    the sentinel start[n_runs] = n; length[r] = its elements; pos = the n + 1 exclusive sums of the head flags"""
    keys = np.asarray(keys, dtype=np.uint64)
    n, want = len(keys), run_starts(keys, shift)
    assert int(n_runs) == len(want), "%d runs, expected %d" % (int(n_runs), len(want))
    start, length, pos = np.asarray(start), np.asarray(length), np.asarray(pos)
    assert start.dtype == np.uint32 and length.dtype == np.uint32 and pos.dtype == np.uint64, (start.dtype, length.dtype, pos.dtype)
    _same("starts and the sentinel", start, np.r_[want, n].astype(np.uint32))
    _same("lengths", length, np.diff(np.r_[want, n]).astype(np.uint32))
    _same("run keys", np.asarray(run_keys, dtype=np.uint64), keys[want])
    head = np.zeros(n, dtype=np.uint64)
    head[want] = 1
    _same("positions", pos, np.r_[0, np.cumsum(head)].astype(np.uint64))


def expected_find(table_keys, queries):
    """for every query the one index of the downloaded keys that holds it, or -1 (a Python dict over the downloaded keys)"""
    tk = np.asarray(table_keys, dtype=np.uint64).tolist()
    where = {}
    for i, key in enumerate(tk):
        assert key not in where, "key %#x is stored twice, at %d and %d" % (key, where[key], i)
        where[key] = i
    get = where.get
    return np.fromiter((get(q, -1) for q in np.asarray(queries, dtype=np.uint64).tolist()), dtype=np.int64, count=len(queries))


def check_find(table_keys, queries, idx, want=None):
    """a hit gives the one index holding that key, a miss -1 (want: expected_find of the same arrays, made once for several checks)"""
    idx = np.asarray(idx)
    assert idx.dtype == np.int64, "indices are int64, not %s" % idx.dtype
    _same("indices", idx, expected_find(table_keys, queries) if want is None else want)


def reduce_by_key(keys, counts):
    """(distinct keys ascending, their summed counts in uint64)"""
    keys = np.asarray(keys, dtype=np.uint64)
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), dtype=np.uint64)
    np.add.at(sums, inv, np.asarray(counts).astype(np.uint64))
    return uk, sums


def check_table_content(keys_in, counts_in, table_keys, table_counts):
    """a downloaded table, regrouped by key, is the input reduced by key: every distinct key once, with the sum of its counts"""
    uk, sums = reduce_by_key(keys_in, counts_in)
    table_keys = np.asarray(table_keys, dtype=np.uint64)
    order = np.argsort(table_keys, kind="stable")
    _same("distinct keys", table_keys[order], uk)
    _same("counts", np.asarray(table_counts).astype(np.uint64)[order], sums)


# ---------------------------------------------------------------- sort cases
SORT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 2 * TILE + 1, 5 * TILE + 77, 70001)
SHAPE_SIZES = (4097, 70001)
SHAPES = ("all_equal", "zeros", "two_digits", "ascending", "descending", "digits256", "lane_digit", "random", "distinct3", "distinct17",
          "distinct1000")
TIE_SHAPES = ("all_equal", "zeros", "two_digits", "digits256", "lane_digit", "distinct3", "distinct17", "distinct1000")
RANGES = ((0, 8), (0, 16), (0, 24), (0, 26), (0, 32), (0, 33), (0, 50), (0, 62), (0, 64), (32, 62), (32, 64), (3, 19), (5, 5), (8, 0))
RANGE_N = 5 * TILE + 77          # the first size whose histogram (256 a tile) needs more than one scan block


def _sort_names():
    names = []
    for n in SORT_SIZES:
        names += ["size_%d_b0_64" % n, "size_%d_b0_24" % n]          # 8 passes (result in place), 3 passes (copied back)
    for n in SHAPE_SIZES:
        names += ["%s_%d" % (s, n) for s in SHAPES]
    for lo, hi in RANGES:
        names += ["range_%d_%d_zero_outside" % (lo, hi), "range_%d_%d_random_outside" % (lo, hi)]
    return tuple(names)


SORT_CASES = _sort_names()
TIE_CASES = tuple("%s_%d" % (s, n) for n in SHAPE_SIZES for s in TIE_SHAPES)
RANDOM_OUTSIDE_CASES = tuple(n for n in SORT_CASES if n.endswith("_random_outside"))
ZERO_OUTSIDE_CASES = tuple(n for n in SORT_CASES if n.endswith("_zero_outside"))


def _shape_keys(shape, n, rng):
    i = np.arange(n, dtype=np.uint64)
    if shape == "all_equal":
        return np.full(n, 0xC3A5C85C97CB3127, dtype=np.uint64), 0, 64
    if shape == "zeros":                                               # the padding lanes of the last tile hold k = 0 too
        return np.zeros(n, dtype=np.uint64), 0, 64
    if shape == "two_digits":
        return np.where(i & U64(1), U64(0x00FF00FF00FF00FF), U64(0xFF00FF00FF00FF00)), 0, 64
    if shape == "ascending":
        return i, 0, 24
    if shape == "descending":
        return U64(n - 1) - i, 0, 24
    if shape == "digits256":                                           # every digit equally often (to within one), in random order
        return rng.permutation(i % U64(256)).astype(np.uint64), 0, 8
    if shape == "lane_digit":                                          # digit = lane: no two lanes of a row of 64 share a digit
        return i % U64(64), 0, 8
    if shape == "random":
        return _u64(rng, n), 0, 64
    pool = _u64(rng, int(shape[len("distinct"):]))
    return pool[rng.integers(0, len(pool), size=n)], 0, 64


@lru_cache(maxsize=None)
def sort_case(name):
    rng = _rng("sort:" + name)
    parts = name.split("_")
    if parts[0] == "size":
        n, lo, hi = int(parts[1]), int(parts[2][1:]), int(parts[3])
        keys = _u64(rng, n)
    elif parts[0] == "range":
        lo, hi, n = int(parts[1]), int(parts[2]), RANGE_N
        # inside the range: half as many values as elements, so most elements tie with another one
        pool = _u64(rng, n // 2)
        inside = masked(pool[rng.integers(0, len(pool), size=n)], lo, hi) << U64(lo if hi > lo else 0)
        keep = U64((range_mask(lo, hi) << lo) & ALL64) if hi > lo else U64(0)
        keys = inside & keep
        if parts[3] == "random":
            keys = keys | (_u64(rng, n) & ~keep)
    else:
        n = int(parts[-1])
        keys, lo, hi = _shape_keys("_".join(parts[:-1]), n, rng)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys.setflags(write=False)
    vals = np.arange(len(keys), dtype=np.uint32)
    vals.setflags(write=False)
    return SortCase(keys, vals, lo, hi)


# ---------------------------------------------------------------- scan cases
SCAN_SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 21) + 5, 3 * (1 << 20) + 17)
SCAN_VALUES = ("ones32", "zeros", "final_one", "random", "flags97")
SCAN_CASES = tuple("%s_%d" % (v, n) for n in SCAN_SIZES for v in SCAN_VALUES)


@lru_cache(maxsize=4)                                                   # (the largest is 12 MB)
def scan_case(name):
    kind, n = name.rsplit("_", 1)
    n = int(n)
    rng = _rng("scan:" + name)
    if kind == "ones32":                                               # the running sum passes 2^32 inside one thread's four elements
        v = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    elif kind == "zeros":
        v = np.zeros(n, dtype=np.uint32)
    elif kind == "final_one":
        v = np.zeros(n, dtype=np.uint32)
        v[-1:] = 1
    elif kind == "random":
        v = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    else:                                                              # keep flags as the compactions scan them
        v = (rng.integers(0, 97, size=n) == 0).astype(np.uint32)
    v.setflags(write=False)
    return v


# ---------------------------------------------------------------- run cases
# sizes: nothing, one, two; around one workgroup (256); around one scan block (1024); several scan blocks with an odd tail
RUN_SIZES = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 70001)
RUN_PATTERNS = ("all_equal", "all_distinct", "random_runs", "edge_runs", "shift20", "bit63", "all_ones")
RUN_CASES = tuple("%s_%d" % (p, n) for n in RUN_SIZES for p in RUN_PATTERNS)


def _random_lengths(rng, n):
    """run lengths 1 .. 9 that sum to n"""
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(1, 10)))
    if lens:
        lens[-1] -= sum(lens) - n
    return lens


@lru_cache(maxsize=None)
def run_case(name):
    """keys sorted by (key >> shift):
    all_equal / all_distinct   one run / n runs
    random_runs                runs of 1 .. 9 elements
    edge_runs                  the first and the last run hold one element (n >= 3: longer ones between them)
    shift20                    random_runs by the bits from 20 up, random bits below the shift inside a run
    bit63                      two runs (n >= 2) whose keys differ in bit 63 alone, shift 0
    all_ones                   random_runs, the last run's key 0xFFFFFFFFFFFFFFFF"""
    pattern, n = name.rsplit("_", 1)
    n = int(n)
    rng = _rng("runs:" + name)
    shift = 20 if pattern == "shift20" else 0
    if pattern == "all_equal":
        lens = [n] if n else []
    elif pattern == "all_distinct":
        lens = [1] * n
    elif pattern == "edge_runs":
        lens = [1] * n if n < 3 else [1] + _random_lengths(rng, n - 2) + [1]
    elif pattern == "bit63":
        lens = [n // 2, n - n // 2] if n >= 2 else [1] * n
    else:
        lens = _random_lengths(rng, n)
    if pattern == "bit63":
        low = int(rng.integers(0, 1 << 63))
        values = np.array([low, low | (1 << 63)][2 - len(lens):], dtype=np.uint64)
    else:
        values = np.zeros(0, dtype=np.uint64)
        while len(values) < len(lens):                                  # distinct, ascending, below 2^(64 - shift) - 1
            values = np.unique(rng.integers(0, (1 << (64 - shift)) - 1, size=len(lens) + 8, dtype=np.uint64))
        values = values[np.sort(rng.choice(len(values), size=len(lens), replace=False))]
        if pattern == "all_ones" and len(values):
            values[-1] = U64(ALL64)
    keys = np.repeat(values, lens) << U64(shift)
    if shift:
        keys |= rng.integers(0, 1 << shift, size=n, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert len(keys) == n
    keys.setflags(write=False)
    return RunCase(keys, shift)


# ---------------------------------------------------------------- table cases
TABLE_CASES = ("n0", "n1", "n2", "n3", "n96", "n97", "uniform_k2", "uniform_k8", "uniform_k13", "uniform_k25", "uniform_k32", "clustered",
               "top16_ones", "top16_zeros", "one_key", "dups", "retry")
RETRY_N, RETRY_K, RETRY_HEAVY = 100000, 25, 1200


def _key_mask(k):
    return ALL64 if k == 32 else (1 << (2 * k)) - 1


def _retry_keys(rng):
    """100,000 distinct 50-bit keys; 1,200 of them fall into ONE bucket of the 11 bits the build starts with and, 300 each, into its
    four sub-buckets at 13 bits"""
    bits0 = start_bits(RETRY_N)
    want = None
    picked = []
    have = [0, 0, 0, 0]
    while min(have) < RETRY_HEAVY // 4:
        cand = np.unique(rng.integers(0, 1 << (2 * RETRY_K), size=1 << 20, dtype=np.uint64))
        h = fmix64(cand)
        if want is None:
            want = int(h[0] >> U64(64 - bits0))
        cand = cand[(h >> U64(64 - bits0)) == U64(want)]
        sub = (fmix64(cand) >> U64(64 - bits0 - 2)).astype(np.int64) & 3
        for s in range(4):
            take = cand[sub == s][:RETRY_HEAVY // 4 - have[s]]
            picked.append(take)
            have[s] += len(take)
    heavy = np.unique(np.concatenate(picked))
    assert len(heavy) == RETRY_HEAVY
    rest = np.unique(rng.integers(0, 1 << (2 * RETRY_K), size=2 * RETRY_N, dtype=np.uint64))
    rest = rng.permutation(rest[~np.isin(rest, heavy)])[:RETRY_N - RETRY_HEAVY]
    return rng.permutation(np.concatenate([heavy, rest]))


@lru_cache(maxsize=None)
def table_case(name):
    rng = _rng("table:" + name)
    canonical = 0
    if name[0] == "n" and name[1:].isdigit():
        k, n = 25, int(name[1:])
        keys = rng.permutation(np.unique(_u64(rng, 4 * n + 4) & U64(_key_mask(k))))[:n]
    elif name.startswith("uniform_k"):
        k = int(name[len("uniform_k"):])
        keys = _u64(rng, 5000) & U64(_key_mask(k))
        if k == 32:
            keys[rng.choice(5000, size=7, replace=False)] = U64(ALL64)     # EMPTY_KEY of the bucket kernel, which carries it apart
            canonical = 1
    elif name == "clustered":                                          # one run of integers: the top 16 of the 62 bits are the same everywhere
        k = 31
        base = int(rng.integers(1 << 40, 1 << 61))
        keys = rng.permutation(U64(base) + np.arange(50000, dtype=np.uint64))
    elif name in ("top16_ones", "top16_zeros"):
        k = 25
        keys = _u64(rng, 20000) & U64((1 << 34) - 1)
        if name == "top16_ones":
            keys |= U64(0xFFFF << 34)
    elif name == "one_key":
        k = 25
        keys = np.full(100000, 0x2B7E151628AED & _key_mask(k), dtype=np.uint64)
    elif name == "dups":
        k = 25
        pool = np.unique(_u64(rng, 21000) & U64(_key_mask(k)))[:20000]
        keys = rng.permutation(np.concatenate([pool, pool[rng.integers(0, 20000, size=40000)]]))
    elif name == "retry":
        k = RETRY_K
        keys = _retry_keys(rng)
    else:
        raise KeyError(name)
    if name == "one_key":
        counts = np.full(len(keys), 3, dtype=np.uint32)
    else:
        counts = rng.integers(1, 1001, size=len(keys)).astype(np.uint32)   # (sums stay far below 2^32)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys.setflags(write=False)
    counts.setflags(write=False)
    return TableCase(keys, counts, k, canonical)


@lru_cache(maxsize=None)
def table_queries(name):
    """every stored key, every stored key +-1 (held inside the 2k bits), 2,000 uniform keys, 0 and the largest key"""
    case = table_case(name)
    top = _key_mask(case.k)
    k = case.keys
    up = np.where(k == U64(top), k, k + U64(1))
    down = np.where(k == U64(0), k, k - U64(1))
    rnd = _u64(_rng("queries:" + name), 2000) & U64(top)
    q = np.concatenate([k, up, down, rnd, np.array([0, top], dtype=np.uint64)])
    q.setflags(write=False)
    return q


@lru_cache(maxsize=None)
def table_reference(name):
    """(distinct keys ascending, summed counts uint64) of a case"""
    case = table_case(name)
    return reduce_by_key(case.keys, case.counts)


def reference_counts(name, queries):
    """the count of every query in the case's table, 0 for a miss"""
    uk, sums = table_reference(name)
    queries = np.asarray(queries, dtype=np.uint64)
    if not len(uk):
        return np.zeros(len(queries), dtype=np.uint64)
    at = np.minimum(np.searchsorted(uk, queries), len(uk) - 1)
    return np.where(uk[at] == queries, sums[at], U64(0))
