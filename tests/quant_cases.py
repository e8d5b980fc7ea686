"""The single-end rule of `python -m shannon_amd.quant` as a brute force, and the inputs the tests hold the library against.

Written from the rule's text, with numpy and plain loops, WITHOUT seeds: every start u of every transcript is
scanned.  Nothing here imports shannon_amd.abundance or shannon_amd.quant.  Sequence helpers: tests/filter_fp_cases.py; the EM:
tests/abundance_cases.py (rule 4 of DESIGN.md 3.10, unchanged).

The rule, for transcripts T_0..T_{m-1} and N single reads:
  1. read x is tried as itself and, unless strand-specific, as RC(x).  An orientation y is placed at u on T_j iff u + |y| <= len_j and
     Hamming(y, T_j[u:u+|y|]) <= |y| // 30 (ungapped, forward strand of the text; a base of the read outside ACGT is a mismatch);
     a read shorter than 15 bases is never placed.  C_i = the transcripts that hold at least one placement of the read's minimum
     cost over its orientations; empty: unmapped.  A transcript shorter than 15 bases or with a base outside ACGT is in no C_i.
  2. g[s] = exp(-0.5 * ((s - MEAN) / SD)^2), s = 0..999; mu_l = (sum of s g[s]) / (sum of g[s]) over s <= min(l, 999), both sums in
     ascending s in double; eff_j = len_j - mu_{len_j} + 1, or len_j when that is < 1.
  3. reads with equal C_i form a class; EM, tpm and decision as rules 3-5 of DESIGN.md 3.10, L = bases of the reads / N.
"""
import math
import numpy as np
import abundance_cases as ac
import filter_fp_cases as fc

MIN_LEN = 15
MEAN, SD, BINS = 200.0, 20.0, 1000


def _codes(s, other):
    t = np.full(256, other, np.uint8)
    for i, c in enumerate(b"ACGT"):
        t[c] = i
    return t[np.frombuffer(s.encode(), dtype=np.uint8)]


class Transcripts(object):
    """the eligible transcripts as code arrays; placements(y) scans every start of every one of them (memoised per sequence)"""

    def __init__(self, transcripts):
        self.codes = [(j, _codes(t, 5)) for j, t in enumerate(transcripts) if ac.eligible(t)]
        self.memo = {}

    def placements(self, y):
        """[(transcript, u, mismatches)] of the oriented read y, by rule 1"""
        if y in self.memo:
            return self.memo[y]
        L, out = len(y), []
        if L >= MIN_LEN:
            yc = _codes(y, 4)                                    # (4: a read's base outside ACGT equals nothing)
            for j, tc in self.codes:
                if len(tc) < L:
                    continue
                mm = (np.lib.stride_tricks.sliding_window_view(tc, L) != yc[None, :]).sum(axis=1)      # every u with u + L <= len_j
                for u in np.nonzero(mm <= L // 30)[0].tolist():
                    out.append((j, u, int(mm[u])))
        self.memo[y] = out
        return out


def brute_sets(transcripts, reads, ss, T=None):
    """C_i per read as a sorted tuple (empty: unmapped), by rule 1"""
    T = T if T is not None else Transcripts(transcripts)
    out = []
    for x in reads:
        found = []
        for y in [x] + ([] if ss else [fc.rc(x)]):
            found += [(c, j) for j, _u, c in T.placements(y)]
        if not found:
            out.append(())
            continue
        best = min(c for c, _j in found)
        out.append(tuple(sorted(set(j for c, j in found if c == best))))
    return out


def brute_classes(sets):
    """({C: reads} over the mapped reads, mapped reads)"""
    classes = {}
    for C in sets:
        if C:
            classes[C] = classes.get(C, 0) + 1
    return classes, sum(classes.values())


def brute_eff_model(lens, mean=MEAN, sd=SD):
    """rule 2, every mu_l summed from scratch"""
    out = []
    for n in lens:
        cnt, tot = 0.0, 0.0
        for s in range(min(n, BINS - 1) + 1):
            z = (s - mean) / sd
            g = math.exp(-0.5 * (z * z))
            cnt = cnt + g
            tot = tot + s * g
        eff = float(n)
        if cnt > 0.0:
            e = float(n) - tot / cnt + 1.0
            if e >= 1.0:
                eff = e
        out.append(eff)
    return np.array(out, dtype=np.float64)


def brute_table(transcripts, reads, ss, mean=MEAN, sd=SD):
    """rules 1-3 -> {"sets", "classes", "mapped", "eff", "alpha", "rounds", "tested", "L", "cov"}"""
    sets = brute_sets(transcripts, reads, ss)
    classes, mapped = brute_classes(sets)
    eff = brute_eff_model([len(t) for t in transcripts], mean, sd)
    keys = sorted(classes)
    alpha, rounds, tested = ac.brute_em([list(k) for k in keys], [classes[k] for k in keys], eff, len(transcripts))
    L = sum(len(r) for r in reads) / len(reads)
    return {"sets": sets, "classes": classes, "mapped": mapped, "eff": eff, "alpha": alpha, "rounds": rounds, "tested": tested, "L": L,
            "cov": alpha / eff * L}


# ---------------------------------------------------------------------------------------------------------------- inputs
LENGTHS = [14, 15, 29, 30, 31, 32, 33, 64, 65, 100, 270]         # the seed count steps and the 32-base word edges


def with_n(s, pos):
    s = list(s)
    for p in pos:
        s[p] = "N"
    return "".join(s)


def length_case(lens, n_reads, seed=3, err=0.005):
    """n_reads reads of the lengths `lens` in turn from three random transcripts, every second one reverse-complemented, 0.5 %
    substitutions, every seventh a random sequence: (transcripts, reads)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [fc.rand_seq(rng, n) for n in (400, 330, 500)]
    reads = []
    for k in range(n_reads):
        L = lens[k % len(lens)]
        t = T[int(rng.integers(0, 3))]
        u = int(rng.integers(0, len(t) - L + 1))
        x = t[u:u + L] if k % 7 != 6 else fc.rand_seq(rng, L)
        x = fc.mutate(x, np.nonzero(rng.random(L) < err)[0])
        reads.append(fc.rc(x) if k % 2 else x)
    return T, reads


def end_case(seed=5):
    """reads flush with a transcript's first and last base, and hanging over either end by one base -- over the end with the first
    base of the transcript that follows in memory, over the start with the last base of the one before: (transcripts, reads, the
    indices of the reads that must stay unmapped)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [fc.rand_seq(rng, n) for n in (300, 260, 280)]
    reads, unmapped = [], []
    for L in (15, 33, 100):
        reads += [T[1][:L], T[1][-L:]]                           # flush with the start, ends exactly at the last base
        unmapped += [len(reads), len(reads) + 1]
        reads += [T[1][-(L - 1):] + T[2][0], T[0][-1] + T[1][:L - 1]]        # one over the end, one over the start
    reads.append(T[0] + "ACGT")                                  # a read longer than every transcript ...
    unmapped.append(len(reads) - 1)
    reads.append(T[1])                                           # ... and one exactly as long as its transcript
    return T, reads, unmapped


def budget_case(seed=7):
    """per read length L (thr = L // 30 mismatches allowed, thr + 1 seeds at 0, 15, ...) and per seed `clean`: a mismatch inside
    every OTHER seed -- thr of them: placed, found through the clean seed alone; those and one inside the clean seed too (thr + 1,
    every seed hit): never; those and one behind the seeds (thr + 1, the clean seed still finds the start): refused by the count.
    (transcripts, reads, expected mapped flags)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [fc.rand_seq(rng, 700), fc.rand_seq(rng, 650)]
    reads, mapped = [], []
    for L in (30, 31, 64, 65, 100, 270):
        ns = L // 30 + 1
        for clean in range(ns):
            t = T[clean % 2]
            u = int(rng.integers(0, len(t) - L + 1))
            x = t[u:u + L]
            others = [15 * s + 7 for s in range(ns) if s != clean]
            reads.append(fc.mutate(x, others))
            mapped.append(True)
            reads.append(fc.mutate(x, others + [15 * clean + 3]))
            mapped.append(False)
            if L > 15 * ns:
                reads.append(fc.mutate(x, others + [L - 1]))
                mapped.append(False)
            reads.append(fc.rc(fc.mutate(x, others)))            # the same budget on the other orientation
            mapped.append(None)                                  # (mapped iff not strand-specific)
    return T, reads, mapped


def n_case(seed=9):
    """reads with N (an N is a mismatch): inside a seed, outside every seed, at and over the budget, in reads of one seed:
    (transcripts, reads, expected mapped flags)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [fc.rand_seq(rng, 500)]
    t = T[0]
    reads, mapped = [], []
    for L, npos, sub, ok in ((100, [5], [], True),               # inside seed 0: found through seed 1
                             (100, [70], [], True),              # outside every seed (the seeds cover bases 0..59)
                             (100, [5, 20, 35], [], True),       # three seeds hold an N, the fourth finds it: cost 3 = thr
                             (100, [5, 20, 35, 50], [], False),  # every seed holds an N
                             (100, [5, 20, 35, 70], [], False),  # found, 4 > thr
                             (100, [5, 70], [22], True), (100, [99, 98], [0, 50], False),
                             (15, [7], [], False), (29, [20], [], False),       # one seed, thr 0: an N anywhere is one too many
                             (30, [3], [], True), (30, [3, 20], [], False),     # thr 1
                             (64, [63], [0], True), (65, [64, 32], [31], False), (33, [32], [], True)):
        u = int(rng.integers(0, len(t) - L + 1))
        x = with_n(fc.mutate(t[u:u + L], sub), npos)
        reads += [x, fc.rc(x)]
        mapped += [ok, ok and None]                              # (the reverse complement: mapped iff not strand-specific)
    return T, reads, mapped


def orientation_case(seed=11):
    """transcript 0 holds X and, further on, RC(X): read X lands on it in both orientations -- listed once.  Transcript 1 holds a
    palindrome P = RC(P): both orientations are the same placement.  Transcript 2 holds Y with one base changed, transcript 3
    RC(Y) exactly: read Y costs 1 forward on 2 and 0 reverse on 3 -- {3}, but {2} when strand-specific.  Transcript 4 is 12 bases,
    transcript 5 holds an N (and a copy of X): neither takes part.  (transcripts, reads, {ss: expected sets})"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X, Y = fc.rand_seq(rng, 100), fc.rand_seq(rng, 100)
    half = fc.rand_seq(rng, 16)
    P = half + fc.rc(half)
    assert fc.rc(P) == P
    T = [fc.rand_seq(rng, 40) + X + fc.rand_seq(rng, 30) + fc.rc(X) + fc.rand_seq(rng, 25),
         fc.rand_seq(rng, 50) + P + fc.rand_seq(rng, 50),
         fc.rand_seq(rng, 20) + fc.mutate(Y, [50]) + fc.rand_seq(rng, 20),
         fc.rand_seq(rng, 33) + fc.rc(Y) + fc.rand_seq(rng, 10),
         fc.rand_seq(rng, 12),
         fc.rand_seq(rng, 10) + "N" + X + fc.rand_seq(rng, 10)]
    reads = [X, P, Y, fc.rc(Y)]
    want = {False: [(0,), (1,), (3,), (3,)], True: [(0,), (1,), (2,), (3,)]}
    return T, reads, want


def count_case(seed=13):
    """257 reads of 30 bases drawn from three transcripts of which two are handed over, every seventh a random sequence:
    (transcripts, reads)"""
    T, reads = length_case([30], 257, seed=seed)
    return T[:2], reads


def unsorted_case(n_tr):
    """abundance_cases.interleaved_case's transcripts with its first mates as single reads: every read costs one mismatch on every
    transcript, the odd ones found through seed 0, the even ones through seed 1 -- the list arrives as the odd transcripts
    ascending, then the even ones"""
    T, r1, _r2 = ac.interleaved_case(n_tr)
    return T, r1


def isoform_case(seed=17, n_reads=1500, L=75):
    """three genes of two isoforms each (a shared exon and a stretch of their own) + a barely expressed transcript of 500 random
    bases that 6 reads cover once; reads forward and reverse in turn, 0.3 % substitutions: (names, transcripts, reads, the name of
    the barely expressed one)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    names, T, weight = [], [], []
    for g in range(3):
        E = fc.rand_seq(rng, 400)
        for k in range(2):
            names.append("g%d_i%d" % (g, k))
            T.append(fc.rand_seq(rng, 250 + 60 * k) + E + fc.rand_seq(rng, 200))
            weight.append(1.0 + 2.0 * k + g)
    p = np.array(weight) * np.array([len(t) for t in T], dtype=np.float64)
    p /= p.sum()
    reads = []
    for k in range(n_reads):
        t = T[int(rng.choice(len(T), p=p))]
        u = int(rng.integers(0, len(t) - L + 1))
        x = fc.mutate(t[u:u + L], np.nonzero(rng.random(L) < 0.003)[0])
        reads.append(fc.rc(x) if k % 2 else x)
    S = fc.rand_seq(rng, 500)
    names.append("rare")
    T.append(S)
    for k in range(6):
        reads.append(S[k * 80:k * 80 + L])
    return names, T, reads, "rare"


def stranded_case(seed=19, n_each=150, L=60):
    """two unrelated transcripts; the reads from A are given on A's strand, the reads from B as their reverse complements: not
    strand-specific all of them map, strand-specific only A's -- B's est_counts are 0.  (names, transcripts, reads)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B = fc.rand_seq(rng, 700), fc.rand_seq(rng, 640)
    reads = []
    for _ in range(n_each):
        u = int(rng.integers(0, len(A) - L + 1))
        reads.append(A[u:u + L])
        u = int(rng.integers(0, len(B) - L + 1))
        reads.append(fc.rc(B[u:u + L]))
    return ["A", "B"], [A, B], reads
