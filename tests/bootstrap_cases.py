"""Rule 1 of DESIGN.md 3.14 (the bootstrap replicates' class counts) as a brute force, written from the rule's text; nothing here imports
shannon_amd.

  Replicate b of B makes N = sum n_c draws t = 0..N-1.  A draw is Philox4x32-10 with counter (t, b, 0, 0) and key (seed & 0xFFFFFFFF,
  seed >> 32), giving o0..o3.  One round: p0 = M0 * c0, p1 = M1 * c2, c = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)), then
  both key words are bumped (k0 += W0, k1 += W1); ten rounds.  u = o0 | o1 << 32, r = (u * N) >> 64; the draw lands in the class c with
  cum[c] <= r < cum[c + 1], cum the exclusive prefix sum of n_c.  counts[b][c] = the draws of replicate b that land in c.

`philox`, `draw` and `brute_counts` are that text in Python integers.  `brute_counts_np` is the same arithmetic on numpy uint64 arrays
(the 128-bit product split into 32-bit halves) for the sizes the GPU tests use; tests/test_bootstrap.py holds it equal to the integers.
"""
import bisect
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter / key -> output
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw(t, b, seed, N):
    """r of draw t of replicate b"""
    o = philox((t, b, 0, 0), (seed & MASK, seed >> 32))
    return ((o[0] | o[1] << 32) * N) >> 64


def cum_of(n_c):
    cum = [0]
    for n in n_c:
        cum.append(cum[-1] + int(n))
    return cum


def class_of(cum, r):
    """the c with cum[c] <= r < cum[c + 1]"""
    return bisect.bisect_right(cum, r) - 1


def brute_counts(n_c, B, seed):
    """counts[B][classes] in Python integers"""
    cum = cum_of(n_c)
    N = cum[-1]
    out = [[0] * len(n_c) for _ in range(B)]
    for b in range(B):
        for t in range(N):
            out[b][class_of(cum, draw(t, b, seed, N))] += 1
    return out


def brute_counts_np(n_c, B, seed):
    """brute_counts on uint64 arrays: uint64[B][classes]"""
    cum = np.array(cum_of(n_c), dtype=np.uint64)
    N, n_classes = int(cum[-1]), len(n_c)
    assert N < 1 << 32 and B < 1 << 32
    out = np.zeros((B, n_classes), dtype=np.uint64)
    if N == 0:
        return out
    m32, s32 = np.uint64(MASK), np.uint64(32)
    t = np.arange(N, dtype=np.uint64)
    for b in range(B):
        c0, c1, c2, c3 = t.copy(), np.full(N, b, np.uint64), np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        k0, k1 = seed & MASK, seed >> 32
        for _ in range(10):
            p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                      # (32-bit words: the products fit 64 bits)
            c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        # u = c1 << 32 | c0; (u * N) >> 64 = (c1 * N + ((c0 * N) >> 32)) >> 32, and c1 * N + 2^32 - 1 < 2^64
        r = (c1 * np.uint64(N) + ((c0 * np.uint64(N)) >> s32)) >> s32
        cls = np.searchsorted(cum, r, side="right") - 1
        out[b] = np.bincount(cls, minlength=n_classes).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def resample_cases():
    """the class counts the GPU test draws from: {name: n_c}"""
    rng = np.random.Generator(np.random.PCG64(91))
    out = {"one fragment": [1], "an empty class between two": [5, 0, 3], "64 draws": [40, 24], "65 draws": [40, 25],
           "all draws to one class": [100000, 1, 1], "no fragments": [0, 0, 0]}
    cuts = np.sort(rng.integers(0, 10001, 999))
    out["1,000 random classes, N = 10,000"] = [int(x) for x in np.diff(np.concatenate([[0], cuts, [10000]]))]
    few = np.zeros(5000, dtype=np.int64)
    np.add.at(few, rng.integers(0, 5000, 200), 1)
    out["5,000 classes, N = 200"] = [int(x) for x in few]
    # the most classes a block counts in LDS, and one more (a wave then combines its equal destinations): a dominant class, a few
    # hundred classes drawn a few times each, the last class among them
    for n in (8192, 8193):
        many = np.zeros(n, dtype=np.int64)
        np.add.at(many, rng.integers(0, n, 700), 1)
        many[17] += 6000
        many[n - 1] += 3
        out["%s classes, N = 6,703" % format(n, ",")] = [int(x) for x in many]
    return out
