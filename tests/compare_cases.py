"""The --compare rule as a brute force, and the inputs the tests hold the library against.

Written from the rule's text with plain loops and numpy prefix sums; nothing here imports shannon_amd.compare.

The rule, for reference transcripts R_0..R_{n-1} (queries) and reconstructed transcripts X_0..X_{m-1} (targets), upper-cased:
  1. every target is taken as it is ('+') and -- unless strand-specific -- as its reverse complement ('-').
  2. a 16-mer of ACGT that R_i holds at a and the oriented target holds at b names the diagonal d = b - a of (i, j, o).
  3. on a named diagonal, over the positions where both sequences exist, a position matches iff both bases are one of ACGT and
     equal; the best segment is the contiguous one of greatest S = matches - 2 mismatches, then the longest, then the one with the
     smallest query start.
  4. per (i, j) the best diagonal: greatest S, then most matches, then '+' before '-', then the smallest d.
  5. a pair whose best holds 30 matches or more gives a row (i, j, o, matches, mismatches, qStart, qEnd, tStart); tStart is counted
     on the target's forward strand.  Rows are ordered by i, then j.
"""
import numpy as np

SEED = 16
MIN_MATCHES = 30

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def _seeds(s):
    """{16-mer of ACGT: [positions]}"""
    out = {}
    for p in range(len(s) - SEED + 1):
        w = s[p:p + SEED]
        if not w.strip("ACGT"):
            out.setdefault(w, []).append(p)
    return out


def best_segment(q, t, d):
    """(S, length, query start) of rule 3 on diagonal d: every start, and from it every end through one prefix-sum pass"""
    a0, a1 = max(0, -d), min(len(q), len(t) - d)
    sc = np.array([1 if (q[a] == t[a + d] and q[a] in "ACGT") else -2 for a in range(a0, a1)], dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(sc)])
    best = None
    for s in range(len(sc)):
        v = P[s + 1:] - P[s]
        m = int(v.max())
        e = len(v) - 1 - int(np.argmax(v[::-1]))          # the last end of that score: the longest
        key = (m, e + 1, -s)
        if best is None or key > best:
            best = key
    return best[0], best[1], a0 - best[2]


def brute_rows(ref, rec, ss, min_matches=MIN_MATCHES):
    """the rows of rules 1-5 as a list of 8-tuples; ref / rec: [(name, sequence)]"""
    rows = []
    qs = [s.upper() for _n, s in ref]
    ts = [s.upper() for _n, s in rec]
    t_seeds = [[_seeds(x)] + ([] if ss else [_seeds(rc(x))]) for x in ts]
    for i, q in enumerate(qs):
        q_seeds = _seeds(q)
        for j, x in enumerate(ts):
            best = None
            for o, idx in enumerate(t_seeds[j]):
                t = rc(x) if o else x
                diags = set()
                for w, pa in q_seeds.items():
                    for b in idx.get(w, ()):
                        diags.update(b - a for a in pa)
                for d in sorted(diags):
                    S, ln, a = best_segment(q, t, d)
                    mm = (ln - S) // 3
                    if best is None or (S, ln - mm) > best[0]:
                        b0 = a + d
                        best = ((S, ln - mm), (i, j, o, ln - mm, mm, a, a + ln, len(t) - (b0 + ln) if o else b0))
            if best is not None and best[1][3] >= min_matches:
                rows.append(best[1])
    return rows


def as_tuples(r):
    """a shannon_amd.compare.Rows as brute_rows' list"""
    return list(zip(*(a.tolist() for a in r)))


# ---------------------------------------------------------------------------------------------------------------- inputs
def rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def other(s, step=1):
    """every base replaced by another one: equals s nowhere"""
    return "".join("ACGT"[("ACGT".index(c) + step) % 4] for c in s)


def mutate(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def with_n(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "N"
    return "".join(s)


def named(prefix, seqs):
    return [("%s%d" % (prefix, k), s) for k, s in enumerate(seqs)]


def island(q, start, length):
    """a target as long as q that equals it on [start, start + length) and nowhere else"""
    return other(q[:start]) + q[start:start + length] + other(q[start + length:])


def segment_end_cases(seed=3):
    """one shared segment of 31 .. 65 bases, starting at query base 0, 1 and 31 (the word boundaries move), on diagonal 0 and 5"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref, rec = [], []
    for L in (31, 32, 33, 63, 64, 65):
        for start in (0, 1, 31):
            q = rand_seq(rng, 140)
            ref.append(q)
            rec.append(island(q, start, L))
            ref.append(q)
            rec.append(rand_seq(rng, 5) + island(q, start, L))
    # every query meets every target: the segments of the others are random and name nothing
    return named("r", ref), named("x", rec)


def long_diagonal_cases(seed=5):
    """diagonals of 2,049 and 2,100 positions (a second pass of the wave), substitutions on both sides of position 2,048, a best
    segment that crosses it and one that ends right in front of it"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q1 = rand_seq(rng, 2049)
    q2 = rand_seq(rng, 2100)
    q3 = rand_seq(rng, 2100)
    ref = [q1, q2, q3, q1]
    rec = [mutate(q1, [100, 1000, 2040]), mutate(q2, [5, 2047, 2048, 2049, 2050, 2060]), mutate(q3, list(range(2048, 2100, 2)) + [700]),
           mutate(q1, [2030, 2031, 2032, 2033])]
    return named("r", ref), named("x", rec)


def diagonal_cases(seed=7):
    """positive and negative diagonals, a target shorter than its query and a query shorter than its target"""
    rng = np.random.Generator(np.random.PCG64(seed))
    core = rand_seq(rng, 90)
    ref = [rand_seq(rng, 50) + core + rand_seq(rng, 20), core[10:70], rand_seq(rng, 300) + core]
    rec = [core, rand_seq(rng, 200) + core + rand_seq(rng, 7), core[20:60]]
    return named("r", ref), named("x", rec)


def strand_cases(seed=9):
    """targets that hold a query on the other strand; an insert that is its own reverse complement, which both orientations score
    alike ('+' stays); a target that holds the query on both strands, the '-' copy the better one"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rand_seq(rng, 120)
    h = rand_seq(rng, 24)
    pal = h + rc(h)
    qp = rand_seq(rng, 30) + pal + rand_seq(rng, 25)
    q2 = rand_seq(rng, 100)
    ref = [q, qp, q2]
    rec = [rand_seq(rng, 12) + rc(q) + rand_seq(rng, 31), rand_seq(rng, 40) + pal + rand_seq(rng, 33),
           mutate(q2, [50]) + rand_seq(rng, 9) + rc(q2)]
    return named("r", ref), named("x", rec)


def n_cases(seed=11):
    """an N inside every seed of a 31-base island (no row); an N inside a 60-base island (a mismatch the segment runs over); an N
    in the target; an N at the same place in both (matches nothing); lower-case letters"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref, rec = [], []
    q = rand_seq(rng, 100)
    ref.append(with_n(q, [35]))
    rec.append(island(q, 20, 31))
    q = rand_seq(rng, 100)
    ref.append(with_n(q, [40]))
    rec.append(island(q, 20, 60))
    q = rand_seq(rng, 100)
    ref.append(q)
    rec.append(with_n(island(q, 20, 60), [41, 42]))
    q = rand_seq(rng, 100)
    ref.append(with_n(q, [50]))
    rec.append(with_n(island(q, 10, 80), [50]))
    q = rand_seq(rng, 80)
    ref.append(q.lower())
    rec.append(island(q, 5, 50))
    return named("r", ref), named("x", rec)


def threshold_cases(seed=13):
    """a mismatch at every 16th base (runs of 15: no seed, no row); islands of exactly 29 and exactly 30 matches; 30 matches around
    one mismatch (S = 28)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref, rec = [], []
    q = rand_seq(rng, 160)
    ref.append(q)
    rec.append(mutate(q, range(15, 160, 16)))
    for L in (29, 30):
        q = rand_seq(rng, 90)
        ref.append(q)
        rec.append(island(q, 33, L))
    q = rand_seq(rng, 90)
    ref.append(q)
    rec.append(mutate(island(q, 20, 31), [37]))
    return named("r", ref), named("x", rec)


def tie_cases(seed=15):
    """rule 3's ties: a tail of mismatch + two matches (score 0: the longer segment wins), on both ends; two equal islands on one
    diagonal (the first wins).  Rule 4's: two diagonals of one score (the smaller d wins)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref, rec = [], []
    q = rand_seq(rng, 100)
    t = list(other(q))
    t[30:70] = q[30:70]
    t[71:73] = q[71:73]
    t[27:29] = q[27:29]
    ref.append(q)
    rec.append("".join(t))
    q = rand_seq(rng, 150)
    t = list(other(q))
    t[10:50] = q[10:50]
    t[90:130] = q[90:130]
    ref.append(q)
    rec.append("".join(t))
    s, f1, f2 = rand_seq(rng, 45), rand_seq(rng, 10), rand_seq(rng, 10)
    ref.append(f1 + s + f2)                              # (the bases next to both copies differ from the query's: 45 matches each)
    rec.append(rand_seq(rng, 19) + other(f1[-1]) + s + other(f2[0]) + rand_seq(rng, 29) + other(f1[-1]) + s + other(f2[0]) + rand_seq(rng, 3))
    return named("r", ref), named("x", rec)


def repeat_cases(seed=17):
    """a query that holds a segment twice against a target that holds it once, twice, and three times (several diagonals of one
    pair); a low-complexity run (every 16-mer of it hits every other)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = rand_seq(rng, 50)
    q = rand_seq(rng, 20) + s + rand_seq(rng, 35) + s + rand_seq(rng, 15)
    ref = [q, rand_seq(rng, 10) + "A" * 40 + rand_seq(rng, 10)]
    rec = [rand_seq(rng, 9) + s + rand_seq(rng, 9), rand_seq(rng, 5) + s + rand_seq(rng, 35) + mutate(s, [25]) + rand_seq(rng, 5),
           s + rand_seq(rng, 3) + s + rand_seq(rng, 4) + s, rand_seq(rng, 6) + "A" * 33 + rand_seq(rng, 6) + "T" * 36]
    return named("r", ref), named("x", rec)


def isoform_cases(seed=19):
    """two isoforms that share an exon against one target that holds the exon between the first one's front and the second one's
    back, and against a target that is the exon alone"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B, Cc, D, E = (rand_seq(rng, n) for n in (70, 60, 50, 80, 120))
    ref = [A + E + B, Cc + E + D]
    rec = [A + E + D, E, rc(Cc + E)]
    return named("iso", ref), named("x", rec)


def short_cases(seed=21):
    """sequences shorter than a seed, of exactly 16 bases and empty ones, between ordinary ones"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rand_seq(rng, 64)
    ref = [q[:15], "", q, q[:16], "ACGT"]
    rec = ["", q[:15], q[3:19], q, rand_seq(rng, 8), q[10:50]]
    return named("r", ref), named("x", rec)


def random_cases(n_cases=40, seed=101):
    """small random inputs: 1-4 queries and 1-5 targets of 20-400 bases with planted shared segments of 16-200 bases on either
    strand, 0-3 % substitutions and a few N"""
    out = []
    for c in range(n_cases):
        rng = np.random.Generator(np.random.PCG64(seed + c))
        ref = [rand_seq(rng, int(rng.integers(20, 400))) for _ in range(int(rng.integers(1, 5)))]
        rec = []
        for _ in range(int(rng.integers(1, 6))):
            t = rand_seq(rng, int(rng.integers(20, 400)))
            for _p in range(int(rng.integers(0, 4))):
                q = ref[int(rng.integers(0, len(ref)))]
                L = int(rng.integers(16, min(200, len(q)) + 1))
                u = int(rng.integers(0, len(q) - L + 1))
                seg = q[u:u + L]
                seg = mutate(seg, np.nonzero(rng.random(L) < rng.choice([0.0, 0.01, 0.03]))[0])
                if rng.random() < 0.5:
                    seg = rc(seg)
                v = int(rng.integers(0, len(t) + 1))
                t = t[:v] + seg + t[v + (L if rng.random() < 0.5 else 0):]
            if rng.random() < 0.2 and len(t):
                t = with_n(t, rng.integers(0, len(t), 2))
            rec.append(t)
        if rng.random() < 0.2:
            k = int(rng.integers(0, len(ref)))
            ref[k] = with_n(ref[k], rng.integers(0, len(ref[k]), 2))
        out.append((named("r", ref), named("x", rec)))
    return out


NAMED_CASES = (("segment ends", segment_end_cases), ("long diagonals", long_diagonal_cases), ("diagonals", diagonal_cases), ("strands", strand_cases),
               ("N", n_cases), ("thresholds", threshold_cases), ("ties", tie_cases), ("repeats", repeat_cases), ("isoforms", isoform_cases),
               ("short", short_cases))


def fasta_text(recs, width=0):
    """a FASTA text of the records; width > 0: the sequences over lines of that many bases"""
    out = []
    for name, s in recs:
        out.append(">%s\n" % name)
        if width:
            out += [s[k:k + width] + "\n" for k in range(0, len(s), width)]
        else:
            out.append(s + "\n")
    return "".join(out)
