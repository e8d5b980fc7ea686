"""The --filter_FP rule as a brute force, and the inputs the GPU tests hold the library against.

Written from the rule's text ("filter_FP"), with numpy and plain loops; nothing here imports shannon_amd.filter_fp.

The rule, per partition p with transcripts T_0..T_{m-1}:
  1. every route (p, d) names fragment i = d (strand-specific) or d mod N (strand-doubled numbering, N pairs); a set.
  2. fragment i with mates a = reads_1[i], b = reads_2[i] gives the oriented pair (a, RC(b)); not strand-specific: also
     (b, RC(a)).
  3. read x (L bases) is placed at u on T_j iff 0 <= u, u + L <= |T_j| and Hamming(x, T_j[u:u+L]) <= L // 30; a base of the
     read outside ACGT is a mismatch; a read shorter than 15 bases is never placed.
  4. (x at u, y at v) on the same T_j is concordant iff u <= v, u + |x| <= v + |y|, v + |y| - u <= 500; cost = mismatches.
  5. over both oriented pairs and all transcripts of p: every concordant placement of the fragment's minimum cost covers
     T_j[u:u+|x|) and T_j[v:v+|y|).
  6. hits_j = covered positions of T_j; keep iff hits_j >= len_j * 0.9 in double.
"""
import numpy as np

THRESH = 0.9
MAX_SPAN = 500
MIN_READ = 15

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s):
    return s[::-1].translate(_COMP)


def _codes(s, other):
    t = np.full(256, other, np.uint8)
    for i, c in enumerate(b"ACGT"):
        t[c] = i
    return t[np.frombuffer(s.encode(), dtype=np.uint8)]


class _Partition(object):
    """the transcripts of one partition side by side, so that one pass places a read on all of them"""

    def __init__(self, transcripts, members):
        self.members = members
        self.codes = [_codes(transcripts[j], 5) for j in members]           # (5: a transcript's base outside ACGT equals nothing)
        self.cat = np.concatenate(self.codes + [np.zeros(0, np.uint8)]) if members else np.zeros(0, np.uint8)
        self.start = np.concatenate([[0], np.cumsum([len(c) for c in self.codes])]).astype(np.int64)
        self.owner = np.repeat(np.arange(len(members)), [len(c) for c in self.codes])
        # every 4 bases from every position on as one number: a cheap NECESSARY condition below, nothing more
        n4 = max(len(self.cat) - 3, 0)
        c = self.cat.astype(np.uint32)
        self.quad = (c[0:n4] * 216 + c[1:n4 + 1] * 36 + c[2:n4 + 2] * 6 + c[3:n4 + 3]) if n4 else np.zeros(0, np.uint32)
        self.memo = {}

    def placements(self, x):
        """[(transcript, u, mismatches)] of read x (rule 3): every start of every transcript is looked at.  A window with at most
        L // 30 mismatches differs from x in at most L // 30 of any disjoint 4-base blocks: the starts that fail this on the first
        blocks are dropped before the base-by-base count (an exact shortcut: it only removes windows that rule 3 refuses)."""
        if x in self.memo:
            return self.memo[x]
        L, out = len(x), []
        n = len(self.cat) - L + 1
        if L >= MIN_READ and n > 0:
            xc = _codes(x, 4).astype(np.uint32)                              # (4: a read's base outside ACGT equals nothing)
            nb = min(8, L // 4)
            bad = np.zeros(n, np.int32)
            for b in range(nb):
                q = xc[4 * b] * 216 + xc[4 * b + 1] * 36 + xc[4 * b + 2] * 6 + xc[4 * b + 3]
                bad += self.quad[4 * b:4 * b + n] != q
            u = np.nonzero(bad <= L // 30)[0]
            u = u[self.owner[u] == self.owner[u + L - 1]]                    # inside one transcript
            if len(u):
                mm = (self.cat[u[:, None] + np.arange(L)[None, :]] != xc[None, :]).sum(axis=1)
                for g, m in zip(u.tolist(), mm.tolist()):
                    if m <= L // 30:
                        k = int(self.owner[g])
                        out.append((self.members[k], g - int(self.start[k]), int(m)))
        self.memo[x] = out
        return out


def brute_hits(case, max_span=MAX_SPAN, want_placed=False):
    """hits per transcript of a case (see make_case) by rules 1-5"""
    cover = [np.zeros(len(t), bool) for t in case["transcripts"]]
    n = len(case["r1"])
    by_part = {}
    for p, d in zip(case["routes"][0], case["routes"][1]):
        by_part.setdefault(int(p), set()).add(int(d) if case["ss"] else int(d) % n)
    placed = 0
    for p, frags in sorted(by_part.items()):
        P = _Partition(case["transcripts"], [j for j, q in enumerate(case["part_of"]) if q == p])
        for i in sorted(frags):
            a, b = case["r1"][i], case["r2"][i]
            pairs = [(a, rc(b))] + ([] if case["ss"] else [(b, rc(a))])
            found = []
            for x, y in pairs:
                py = {}
                for j, v, cy in P.placements(y):
                    py.setdefault(j, []).append((v, cy))
                for j, u, cx in P.placements(x):
                    for v, cy in py.get(j, ()):
                        if u <= v and u + len(x) <= v + len(y) and v + len(y) - u <= max_span:
                            found.append((cx + cy, j, u, len(x), v, len(y)))
            if found:
                placed += 1
                best = min(f[0] for f in found)
                for c, j, u, lx, v, ly in found:
                    if c == best:
                        cover[j][u:u + lx] = True
                        cover[j][v:v + ly] = True
    hits = [int(c.sum()) for c in cover]
    return (hits, placed) if want_placed else hits


def keep(hits, lens):
    return [h >= n * THRESH for h, n in zip(hits, lens)]


def make_case(transcripts, part_of, n_parts, r1, r2, routes, ss):
    return {"transcripts": list(transcripts), "part_of": list(part_of), "n_parts": n_parts, "r1": list(r1), "r2": list(r2),
            "routes": (np.asarray(routes[0], np.uint32), np.asarray(routes[1], np.uint32)), "ss": bool(ss)}


# ---------------------------------------------------------------------------------------------------------------- inputs
def rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def mutate(s, positions, rng=None):
    """s with the bases at `positions` replaced by a different base (the next one in ACGT)"""
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def pair_from(t, u, lx, v, ly):
    """mates as a sequencer gives them for x = t[u:u+lx] on the transcript's strand and y = t[v:v+ly]: (x, RC(y))"""
    return t[u:u + lx], rc(t[v:v + ly])


def synth_case(ss, n_pairs=300, read_len=100, seed=7):
    """synth's isoforms of 4 genes in two partitions (by gene), its pairs (0.5 % errors) routed to BOTH partitions; not strand-
    specific: the mates of every second fragment swapped (synth's first mate is always on the transcript's strand) and that
    fragment named by its index in the second half of the strand-doubled numbering"""
    from shannon_amd import synth
    iso, gene = synth.make_transcriptome(4, seed=seed)
    r1, r2 = synth.sample_pairs(iso, n_pairs, seed=seed, read_len=read_len, frag_len=max(300, read_len + 60), sigma=0.5)
    r1, r2 = synth.codes_to_strings(r1), synth.codes_to_strings(r2)
    idx = np.arange(n_pairs, dtype=np.uint32)
    if not ss:
        for i in range(1, n_pairs, 2):
            r1[i], r2[i] = r2[i], r1[i]
        idx[1::2] += n_pairs
    pid = np.concatenate([np.zeros(n_pairs, np.uint32), np.ones(n_pairs, np.uint32)])
    return make_case(synth.codes_to_strings(iso), [g // 2 for g in gene], 2, r1, r2, (pid, np.concatenate([idx, idx])), ss)


def length_case(lx, ly, n_pairs=40, seed=11, err=0.005):
    """pairs of mate lengths lx / ly (ints, or lists to draw from: a ragged set) on three random transcripts, 0.5 % errors"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [rand_seq(rng, n) for n in (900, 700, 1200)]
    r1, r2 = [], []
    for _ in range(n_pairs):
        a = int(rng.choice(lx)) if isinstance(lx, (list, tuple)) else lx
        b = int(rng.choice(ly)) if isinstance(ly, (list, tuple)) else ly
        t = T[int(rng.integers(0, 3))]
        frag = int(rng.integers(max(a, b), min(MAX_SPAN, len(t)) + 1))
        u = int(rng.integers(0, len(t) - frag + 1))
        x, y = pair_from(t, u, a, u + frag - b, b)
        x = mutate(x, np.nonzero(rng.random(len(x)) < err)[0])
        y = mutate(y, np.nonzero(rng.random(len(y)) < err)[0])
        r1.append(x)
        r2.append(y)
    return make_case(T, [0, 0, 0], 1, r1, r2, (np.zeros(n_pairs, np.uint32), np.arange(n_pairs)), True)


def _seed_positions(L, clean):
    """one position inside every 15-base seed of a read of L bases (seeds at 0, 15, ... : L // 30 + 1 of them) but seed `clean`"""
    return [15 * s + 7 for s in range(L // 30 + 1) if s != clean]


def mismatch_case(seed=13):
    """one transcript per fragment; first mate with exactly L // 30 mismatches (every seed but one hit -> placed) and with
    L // 30 + 1 (every seed but one hit + one base behind the seeds; every seed hit -> never placed), the clean seed first,
    in the middle and last; second mate exact.  L = 100 (4 seeds), 60 (3), 30 (2), 250 (9)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T, r1, r2 = [], [], []
    for L in (100, 60, 30, 250):
        ns = L // 30 + 1
        tail = 15 * ns + (L - 15 * ns) // 2 if L > 15 * ns else None          # a base behind the last seed, if there is one
        for clean in sorted({0, ns // 2, ns - 1}):
            variants = [_seed_positions(L, clean)]                             # L // 30 mismatches: placed
            if tail is not None:
                variants.append(_seed_positions(L, clean) + [tail])            # one more, a seed still clean: found, refused
            variants.append(_seed_positions(L, clean) + [15 * clean + 3])      # L // 30 + 1, every seed hit
            variants.append(_seed_positions(L, clean)[:-1])                    # one fewer
            for pos in variants:
                t = rand_seq(rng, 700)
                x, y = pair_from(t, 120, L, 300, L)
                T.append(t)
                r1.append(mutate(x, pos))
                r2.append(y)
        # ... and the same budget on the second mate
        t = rand_seq(rng, 700)
        x, y = pair_from(t, 120, L, 300, L)
        T += [t, t + "A"]
        r1 += [x, x]
        r2 += [rc(mutate(rc(y), _seed_positions(L, 0))), rc(mutate(rc(y), _seed_positions(L, 0) + [3]))]
    n = len(r1)
    # (the two last fragments of a length share their text: both transcripts hold both placements -- ties)
    return make_case(T, [0] * len(T), 1, r1, r2, (np.zeros(n, np.uint32), np.arange(n)), True)


def n_case(seed=17):
    """reads with N: an N is a mismatch -- inside a seed, behind the seeds, together with substitutions at and over the bound"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T, r1, r2 = [], [], []

    def with_n(s, pos):
        s = list(s)
        for p in pos:
            s[p] = "N"
        return "".join(s)
    for L, npos, sub in ((100, [5], []), (100, [70], []), (100, [5, 20, 35], []), (100, [5, 20, 35, 50], []), (100, [5, 20, 35, 70], []),
                         (100, [5, 70], [22]), (100, [99], [0, 50]), (100, [99, 98], [0, 50]), (64, [63], [0]), (64, [63, 20], [0]),
                         (29, [3], []), (20, [19], []), (150, [149, 0, 75, 76, 77], []), (150, [149, 0, 75, 76, 77, 30], [])):
        t = rand_seq(rng, 600)
        x, y = pair_from(t, 50, L, 300, L)
        T.append(t)
        r1.append(with_n(mutate(x, sub), npos))
        r2.append(y)
        t = rand_seq(rng, 600)
        x, y = pair_from(t, 50, L, 300, L)
        T.append(t)
        r1.append(x)
        r2.append(with_n(mutate(y, sub), npos))
    n = len(r1)
    return make_case(T, [0] * len(T), 1, r1, r2, (np.zeros(n, np.uint32), np.arange(n)), True)


def edge_case(seed=19):
    """mates hanging over either end of a transcript by one base, a mate that lies across the border of two transcripts that
    are neighbours in memory, pair geometry (u > v, first mate ending behind the second, span 500 / 501), reads of 14 / 15
    bases, a transcript shorter than the reads and one shorter than a seed"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = [rand_seq(rng, n) for n in (800, 650, 1200, 60, 10, 400)]
    t0, t1, t2 = T[0], T[1], T[2]
    P = []
    P.append(("A" if t0[0] != "A" else "C") + t0[:99])                                  # would start at -1
    P[-1] = (P[-1], rc(t0[300:400]))
    P.append((t0[400:500], rc(t0[701:800] + ("A" if t1[0] != "A" else "C"))))           # would end one behind the end
    P.append((t0[400:500], rc(t0[701:800] + t1[0])))                                    # ... with the neighbour's first base: still not
    P.append((t0[750:800] + t1[:50], rc(t1[200:300])))                                  # across the border
    P.append((t0[0:100], rc(t0[700:800])))                                              # flush with both ends, span 800: too long
    P.append((t0[0:100], rc(t0[400:500])))                                              # flush with the start, span 500
    P.append((t0[300:400], rc(t0[700:800])))                                            # flush with the end
    P.append(pair_from(t2, 300, 100, 250, 100))                                         # u > v
    P.append(pair_from(t2, 300, 100, 310, 60))                                          # u + |x| > v + |y|
    P.append(pair_from(t2, 300, 100, 340, 60))                                          # u + |x| == v + |y|
    P.append(pair_from(t2, 300, 60, 300, 100))                                          # u == v
    P.append(pair_from(t2, 600, 100, 1000, 100))                                        # span 500
    P.append(pair_from(t2, 600, 100, 1001, 100))                                        # span 501
    P.append(pair_from(t2, 100, 14, 200, 100))                                          # 14 bases: never
    P.append(pair_from(t2, 100, 15, 200, 100))                                          # 15 bases: one seed, no mismatch
    P.append((mutate(t2[100:115], [7]), rc(t2[200:300])))
    P.append(pair_from(t2, 100, 100, 200, 15))
    P.append(pair_from(t2, 100, 100, 200, 14))
    P.append(pair_from(t2, 120, 29, 130, 29))
    P.append(pair_from(T[3], 0, 60, 0, 60))                                             # a transcript exactly as long as the reads
    P.append(pair_from(T[5], 0, 100, 300, 100))
    P.append((T[3] + "ACGTACGTAC", rc(T[3] + "ACGTACGTAC")))                            # reads longer than the transcript
    n = len(P)
    return make_case(T, [0] * len(T), 1, [p[0] for p in P], [p[1] for p in P], (np.zeros(n, np.uint32), np.arange(n)), True)


def isoform_case(seed=23, ss=True):
    """six isoforms around one exon (ties: every best placement is marked), a seventh with one base of the exon changed (the
    fragments of either form mark only their own), a transcript that holds a 200-base segment twice"""
    rng = np.random.Generator(np.random.PCG64(seed))
    E = rand_seq(rng, 320)
    iso = [rand_seq(rng, int(rng.integers(60, 200))) + E + rand_seq(rng, int(rng.integers(60, 200))) for _ in range(6)]
    E2 = mutate(E, [160])
    iso.append(rand_seq(rng, 90) + E2 + rand_seq(rng, 90))
    S = rand_seq(rng, 200)
    rep = rand_seq(rng, 100) + S + rand_seq(rng, 50) + S + rand_seq(rng, 120)
    T = iso + [rep]
    P = []
    for u, v in ((0, 200), (10, 120), (100, 220)):
        P.append(pair_from(E, u, 100, v, 100))                 # inside the exon, away from base 160 or over it
        P.append(pair_from(E2, u, 100, v, 100))
    P.append(pair_from(iso[2], 20, 100, 250, 100))             # reaches into isoform 2's own flank
    x, y = pair_from(E, 100, 100, 220, 100)
    P.append((mutate(x, [10]), y))                             # cost 1 on the six, 2 on the seventh
    for u, v in ((0, 100), (20, 60), (50, 100)):
        P.append(pair_from(S, u, 100, v, 100))                 # inside the repeated segment
    P.append(pair_from(rep, 50, 100, 200, 100))                # from the first flank into the first copy
    if not ss:
        P = [(b, a) if i % 2 else (a, b) for i, (a, b) in enumerate(P)]
    n = len(P)
    idx = np.arange(n, dtype=np.uint32)
    if not ss:
        idx[::3] += n
    return make_case(T, [0] * len(T), 1, [p[0] for p in P], [p[1] for p in P], (np.zeros(n, np.uint32), idx), ss)


def partition_case(seed=29):
    """two partitions with the same transcript, fragments routed to one of them only; a partition without transcripts that has
    routes; a partition without routes; a fragment routed twice and to two partitions"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t, other = rand_seq(rng, 900), rand_seq(rng, 500)
    T, part_of = [t, other, t, rand_seq(rng, 300)], [0, 0, 2, 3]          # partition 1 holds nothing, partition 3 gets no routes
    P = [pair_from(t, int(u), 100, int(u) + 180, 100) for u in rng.integers(0, 600, 12)] + [pair_from(other, 20, 100, 300, 100)]
    n = len(P)
    pid = [0] * 6 + [1] * 6 + [0, 0, 2, 1]
    idx = list(range(6)) + list(range(6, 12)) + [12, 12, 12, 12]
    return make_case(T, part_of, 4, [p[0] for p in P], [p[1] for p in P], (pid, idx), True)


def planted_case(seed=7, n_pairs=3000):
    """true isoforms (synth, 4 genes) with their pairs + isoform 0 with a random tail of 8 % / 15 % of the new length + a
    40-base transcript: (transcripts, names, r1, r2)"""
    from shannon_amd import synth
    iso, _gene = synth.make_transcriptome(4, seed=seed)
    r1, r2 = synth.sample_pairs(iso, n_pairs, seed=seed, sigma=0.5)
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    T = synth.codes_to_strings(iso)
    names = ["iso%d" % i for i in range(len(T))]
    for frac, nm in ((0.08, "tail8"), (0.15, "tail15")):
        tail = int(round(frac * len(T[0]) / (1.0 - frac)))
        T.append(T[0] + rand_seq(rng, tail))
        names.append(nm)
    T.append(rand_seq(rng, 40))
    names.append("short40")
    return T, names, synth.codes_to_strings(r1), synth.codes_to_strings(r2)
