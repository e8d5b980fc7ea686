"""The --kallisto_cutoff rule as a brute force, and the inputs the GPU tests hold the library against.

Written from the rule's text, with numpy and plain loops; nothing here imports shannon_amd.abundance.  The
placement of a mate on the transcripts and the sequence helpers are those of tests/filter_fp_cases.py (rules 2-5 of DESIGN.md 3.8).

The rule, for final transcripts T_0..T_{m-1} and N read pairs:
  1. all transcripts are ONE partition; fragment i gives the oriented pair (a, RC(b)) and, not strand-specific, (b, RC(a)); a mate
     of L >= 15 bases is placed without gaps with at most L // 30 mismatches (N = mismatch); (x at u, y at v) on one transcript is
     concordant iff u <= v, u + |x| <= v + |y|, v + |y| - u <= 500.  C_i = the transcripts that hold a placement of fragment i's
     minimum cost; empty: unmapped.  A transcript shorter than 15 bases or with a base outside ACGT is in no C_i.
  2. h[s] = fragments with exactly one minimum-cost placement, s = its span v + |y| - u.  mu_l = mean of s over h restricted to
     s <= l; eff_j = len_j - mu_{len_j} + 1, or len_j when that is < 1 or the restricted histogram is empty.
  3. fragments with equal C_i form a class with n_c members.
  4. EM in float64 from alpha_j = 1 / m: d_c = sum_{j in c} alpha_j / eff_j, alpha'_j = sum_{c with j} n_c (alpha_j / eff_j) / d_c;
     a class with d_c == 0 gives nothing; tested after rounds 50, 100, ...: stop unless some j has alpha'_j > 1e-2 and
     |alpha'_j - alpha_j| > 1e-2 alpha'_j; stop after 10,000 rounds; alpha_j < 1e-8 -> 0.
  5. cov_j = alpha_j / eff_j * L, L = (bases of reads_1 + bases of reads_2) / N; kept iff cov_j >= cutoff.
"""
import functools
import numpy as np
import filter_fp_cases as fc

MAX_SPAN = 500
MIN_LEN = 15


def eligible(t):
    return len(t) >= MIN_LEN and set(t) <= set("ACGTacgt")


def brute_fragments(transcripts, r1, r2, ss, max_span=MAX_SPAN):
    """per fragment (C_i as a sorted tuple, number of minimum-cost placements, span of the last of them) by rule 1"""
    P = fc._Partition(transcripts, [j for j, t in enumerate(transcripts) if eligible(t)])
    out = []
    for a, b in zip(r1, r2):
        pairs = [(a, fc.rc(b))] + ([] if ss else [(b, fc.rc(a))])
        found = []
        for x, y in pairs:
            py = {}
            for j, v, cy in P.placements(y):
                py.setdefault(j, []).append((v, cy))
            for j, u, cx in P.placements(x):
                for v, cy in py.get(j, ()):
                    if u <= v and u + len(x) <= v + len(y) and v + len(y) - u <= max_span:
                        found.append((cx + cy, j, v + len(y) - u))
        if not found:
            out.append(((), 0, None))
            continue
        best = min(f[0] for f in found)
        at = [f for f in found if f[0] == best]
        out.append((tuple(sorted(set(f[1] for f in at))), len(at), at[-1][2]))
    return out


def brute_classes(frags, max_span=MAX_SPAN):
    """({C: n_c} over the mapped fragments, h as a list of max_span + 1 integers, mapped fragments) by rules 2-3"""
    classes, hist, mapped = {}, [0] * (max_span + 1), 0
    for C, n, span in frags:
        if not C:
            continue
        mapped += 1
        classes[C] = classes.get(C, 0) + 1
        if n == 1:
            hist[span] += 1
    return classes, hist, mapped


def brute_eff(lens, hist):
    out = []
    for n in lens:
        cnt = sum(hist[s] for s in range(min(n, len(hist) - 1) + 1))
        tot = sum(s * hist[s] for s in range(min(n, len(hist) - 1) + 1))
        eff = float(n)
        if cnt:
            e = float(n) - tot / cnt + 1.0
            if e >= 1.0:
                eff = e
        out.append(eff)
    return np.array(out, dtype=np.float64)


def brute_em(class_lists, n_c, eff, m):
    """rule 4 -> (alpha, rounds, [largest relative change over alpha' > 1e-2 at every tested round]); class_lists[c] = the members of
    class c (distinct), two classes may hold the same members"""
    eff = np.asarray(eff, dtype=np.float64)
    alpha = np.full(m, 1.0 / m, dtype=np.float64)
    lists = [np.asarray(M, dtype=np.int64) for M in class_lists]
    tested, rounds = [], 0
    while True:
        w = alpha / eff
        new = np.zeros(m, dtype=np.float64)
        for M, n in zip(lists, n_c):
            d = float(w[M].sum())
            if d != 0.0:
                new[M] += float(n) * w[M] / d
        rounds += 1
        if rounds % 50 == 0:
            big = new > 1e-2
            rel = float((np.abs(new - alpha)[big] / new[big]).max()) if big.any() else 0.0
            tested.append(rel)
            moved = bool((big & (np.abs(new - alpha) > 1e-2 * new)).any())
            alpha = new
            if not moved or rounds >= 10000:
                break
        else:
            alpha = new
    alpha = np.where(alpha < 1e-8, 0.0, alpha)
    return alpha, rounds, tested


def csr(class_lists):
    off = np.zeros(len(class_lists) + 1, dtype=np.uint64)
    if class_lists:
        off[1:] = np.cumsum([len(M) for M in class_lists], dtype=np.uint64)
    mem = np.array([j for M in class_lists for j in M], dtype=np.uint32)
    return off, mem


def brute_table(transcripts, r1, r2, ss, max_span=MAX_SPAN):
    """rules 1-5 -> {"eff", "alpha", "cov", "rounds", "tested", "mapped", "classes", "hist", "L"}"""
    frags = brute_fragments(transcripts, r1, r2, ss, max_span)
    classes, hist, mapped = brute_classes(frags, max_span)
    eff = brute_eff([len(t) for t in transcripts], hist)
    keys = sorted(classes)
    alpha, rounds, tested = brute_em([list(k) for k in keys], [classes[k] for k in keys], eff, len(transcripts))
    L = (sum(len(r) for r in r1) + sum(len(r) for r in r2)) / len(r1)
    return {"eff": eff, "alpha": alpha, "cov": alpha / eff * L, "rounds": rounds, "tested": tested, "mapped": mapped, "classes": classes,
            "hist": hist, "L": L}


# ---------------------------------------------------------------------------------------------------------------- inputs
def shared_exon_case(seed=31):
    """65 transcripts: every one holds exon X65, the first 64 also X64, the first two X2, and each a stretch of its own; pairs from
    inside X65 / X64 / X2 / transcript 0's own stretch have compatibility sets of 65, 64, 2 and 1 transcripts, several pairs each;
    one pair that matches nothing: (transcripts, r1, r2, expected {set size: pairs})"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X65, X64, X2 = (fc.rand_seq(rng, 300) for _ in range(3))
    T = []
    for j in range(65):
        T.append(fc.rand_seq(rng, 40) + X65 + (X64 if j < 64 else "") + (X2 if j < 2 else "") + fc.rand_seq(rng, 260))
    own = T[0][-260:]
    r1, r2, want = [], [], {}
    for src, size, n in ((X65, 65, 5), (X64, 64, 4), (X2, 2, 3), (own, 1, 6)):
        for k in range(n):
            u = int(rng.integers(0, len(src) - 220))
            x, y = fc.pair_from(src, u, 100, u + 100 + int(rng.integers(0, 20)), 100)
            r1.append(x)
            r2.append(y)
        want[size] = n
    r1.append(fc.rand_seq(rng, 100))
    r2.append(fc.rand_seq(rng, 100))
    return T, r1, r2, want


def interleaved_case(n_tr, seed=37):
    """n_tr transcripts around one exon E: the even ones differ from E at base 105 of it, the odd ones at base 120; pairs drawn from E
    whose first mate starts at base 100 cost one mismatch on every transcript, the odd ones found through the mate's first seed
    (bases 0-14, in text order), the even ones through its second (bases 15-29): every pair's placements arrive as the odd
    transcripts ascending, then the even ones ascending -- a list that has to be sorted: (transcripts, r1, r2)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    E = fc.rand_seq(rng, 400)
    T = [fc.rand_seq(rng, 30 + j % 3) + fc.mutate(E, [120 if j % 2 else 105]) + fc.rand_seq(rng, 40) for j in range(n_tr)]
    r1, r2 = [], []
    for k in range(3):
        x, y = fc.pair_from(E, 100, 100, 210 + 7 * k, 100)
        r1.append(x)
        r2.append(y)
    return T, r1, r2


def random_classes(seed, m, n_classes, max_size, max_count=400, eff_range=(50.0, 3000.0)):
    """random classes for the EM: (class lists, n_c, eff)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lists = []
    for _ in range(n_classes):
        k = int(rng.integers(1, max_size + 1))
        lists.append(sorted(int(j) for j in rng.choice(m, size=min(k, m), replace=False)))
    n_c = [int(x) for x in rng.integers(1, max_count, n_classes)]
    eff = rng.uniform(eff_range[0], eff_range[1], m)
    return lists, n_c, eff


def spurious_case(seed=7, n_pairs=3000):
    """planted_case's true isoforms and pairs + one spurious transcript of 700 random bases that 14 pairs cover about four deep (the
    pairs appended behind the true ones): (true transcripts, spurious, r1, r2)"""
    T, _names, r1, r2 = fc.planted_case(seed=seed, n_pairs=n_pairs)
    n_true = len(T) - 3                                       # (planted_case appends two tailed copies and a 40-base transcript)
    rng = np.random.Generator(np.random.PCG64(seed + 200))
    S = fc.rand_seq(rng, 700)
    for k in range(14):
        u = min(k * 31, len(S) - 300)
        x, y = fc.pair_from(S, u, 100, u + 200, 100)
        r1.append(x)
        r2.append(y)
    return T[:n_true], S, r1, r2


def em_cases():
    """the hand-made inputs of the EM tests: {name: (class lists, n_c, eff, m)}"""
    out = {}
    # one shared class beside unique counts
    out["shared pair"] = ([[0], [1], [0, 1]], [30, 10, 20], [200.0, 200.0], 2)
    # transcript 2 in no class, transcript 3 only in a class of its own
    out["a transcript in no class"] = ([[0, 1], [0], [3]], [50, 5, 7], [100.0, 150.0, 80.0, 60.0], 4)
    # a class of 65 members (crosses a wave) beside unique evidence for a few of them
    lists, n_c, eff = random_classes(41, 70, 30, 4)
    out["a class of 65"] = ([list(range(65))] + lists, [900] + n_c, eff, 70)
    # transcript 0 in 130 classes {0, k}: the strided loop over its entries runs three times
    rng = np.random.Generator(np.random.PCG64(43))
    out["a transcript in 130 classes"] = ([[0, k] for k in range(1, 131)] + [[k] for k in range(1, 131, 3)],
                                          [int(x) for x in rng.integers(1, 60, 130)] + [int(x) for x in rng.integers(1, 30, 44)],
                                          rng.uniform(100.0, 2000.0, 131), 131)
    # effective lengths a factor 100 apart inside the classes
    lists, n_c, eff = random_classes(47, 40, 80, 5)
    eff[::2] = eff[::2] / 100.0
    out["eff a factor 100 apart"] = (lists, n_c, eff, 40)
    lists, n_c, eff = random_classes(51, 40, 60, 5)
    out["random, 40 transcripts"] = (lists, n_c, eff, 40)
    # ... and larger ones in which every transcript also has evidence of its own (the EM then settles within the first 50 rounds;
    # without it the changes of dying transcripts linger near 1e-2 for hundreds of rounds, which the stated condition excludes)
    for seed, m, nc, size in ((60, 300, 500, 6), (62, 1000, 1500, 8)):
        lists, n_c, eff = random_classes(seed, m, nc, size)
        rng = np.random.Generator(np.random.PCG64(seed + 1000))
        out["random, %d transcripts" % m] = (lists + [[j] for j in range(m)], n_c + [int(x) for x in rng.integers(20, 400, m)], eff, m)
    return out


def union_case():
    """"shared pair", "a class of 65" and "random, 40 transcripts" side by side on 2 + 70 + 40 transcripts; rows: the counts of the first
    alone, of the second alone, of the third alone, of all three, and none at all"""
    cases = em_cases()
    lists, eff, blocks, base = [], [], [], 0
    for name in ("shared pair", "a class of 65", "random, 40 transcripts"):
        L, n_c, e, m = cases[name]
        lists += [[j + base for j in M] for M in L]
        eff += [float(x) for x in e]
        blocks.append([int(x) for x in n_c])
        base += m
    z = [[0] * len(b) for b in blocks]
    rows = [blocks[0] + z[1] + z[2], z[0] + blocks[1] + z[2], z[0] + z[1] + blocks[2], blocks[0] + blocks[1] + blocks[2], z[0] + z[1] + z[2]]
    return lists, np.array(rows, dtype=np.uint64), np.array(eff), base


@functools.lru_cache(maxsize=None)
def em_golden_case(name):
    """the rows tests/golden/abundance_em_bits.json records for `name` (an em_cases() name, or "union"): (class lists, count matrix, eff,
    labels) -- the case's own n_c ("n_c") and the 65 bootstrap rows of bootstrap_cases.brute_counts_np(n_c, 65, 7) ("b0" ..); "union":
    union_case()'s five rows ("u0" ..)"""
    import bootstrap_cases as bc
    if name == "union":
        lists, matrix, eff, _m = union_case()
        return lists, matrix, eff, ["u%d" % k for k in range(len(matrix))]
    lists, n_c, eff, _m = em_cases()[name]
    matrix = np.concatenate([np.array([n_c], dtype=np.uint64), bc.brute_counts_np(n_c, 65, 7)])
    return lists, matrix, np.asarray(eff, dtype=np.float64), ["n_c"] + ["b%d" % b for b in range(65)]


def em_golden_names():
    return sorted(em_cases()) + ["union"]
