"""The chained form of the --compare rule ("Chained rows") as a brute force, and the inputs the tests hold the
library against.  Written from the rule's text; nothing here imports shannon_amd.compare.

Blocks.  For a query i and an oriented target (j, o) every seed-named diagonal d gives one block: its best segment by rule 3
(compare_cases.best_segment) -- d, qStart, qEnd, matches, mismatches; len = qEnd - qStart, S = matches - 2 mismatches, on the
oriented target tS = qStart + d, tE = qEnd + d.  Blocks are ordered by qEnd, then d; the position there is the block's index.
Join.  A -> B iff d_A != d_B and v < len_B, v = max(0, qEnd_A - qStart_B, tE_A - tS_B); B enters without its first v positions,
its matches and mismatches recounted over what is left.  A is never altered by what follows it.
Value of a chain: (sum S, sum matches, -blocks), greatest first; of equal values the chain whose block indices, read from the last
block backwards, are lexicographically smallest.  Per pair the greater value over both orientations, '+' of equals.  A row iff
sum matches >= 30; rows by i, then j.

A row here is a tuple: (i, j, o, matches, mismatches, qStart, qEnd, tStart, qNumInsert, qBaseInsert, tNumInsert, tBaseInsert,
blockCount, ((size, qStart, tStart), ..)) -- tStart of the row and of every block on the target's forward strand."""
import functools
import numpy as np
import compare_cases as cc

ENUMERATE_UP_TO = 10


def blocks_of(q, t):
    """the blocks of q against the oriented target t, in index order: [(d, qStart, qEnd, matches, mismatches)]"""
    qs, ts = cc._seeds(q), cc._seeds(t)
    diags = set()
    for w, pa in qs.items():
        for b in ts.get(w, ()):
            diags.update(b - a for a in pa)
    out = []
    for d in diags:
        S, ln, a = cc.best_segment(q, t, d)
        mm = (ln - S) // 3
        out.append((d, a, a + ln, ln - mm, mm))
    return sorted(out, key=lambda b: (b[2], b[0]))


def overlap(A, B):
    """v of the join rule, or None where B may not follow A"""
    if A[0] == B[0]:
        return None
    v = max(0, A[2] - B[1], (A[2] + A[0]) - (B[1] + B[0]))
    return v if v < B[2] - B[1] else None


def recount(q, t, B, v):
    """(matches, mismatches) of block B without its first v positions, on the strings"""
    d, a0, a1 = B[0], B[1] + v, B[2]
    m = sum(1 for a in range(a0, a1) if q[a] == t[a + d] and q[a] in "ACGT")
    return m, (a1 - a0) - m


def chain_of(q, t, blocks, idx):
    """the chain through the blocks idx, in that order: (value, [(block index, v, matches, mismatches)])"""
    S = M = 0
    parts = []
    for k, b in enumerate(idx):
        v = 0 if k == 0 else overlap(blocks[idx[k - 1]], blocks[b])
        m, mm = recount(q, t, blocks[b], v)
        S, M = S + m - 2 * mm, M + m
        parts.append((b, v, m, mm))
    return (S, M, -len(idx)), parts


def best_chain_enumerated(q, t, blocks):
    """every chain the join rule allows, each a sequence of block indices; the whole chains sorted"""
    found = []

    def extend(idx):
        found.append(tuple(idx))
        for b in range(len(blocks)):
            if b not in idx and overlap(blocks[idx[-1]], blocks[b]) is not None:
                extend(idx + [b])
    for b in range(len(blocks)):
        extend([b])
    ranked = sorted(found, key=lambda idx: (tuple(-x for x in chain_of(q, t, blocks, idx)[0]), idx[::-1]))
    return chain_of(q, t, blocks, ranked[0])


def best_chain_table(q, t, blocks):
    """the O(r^2) table: per block, in index order, the best value of a chain that ends in it and the smallest predecessor that
    attains it (the value is additive, so a prefix of an optimal chain is optimal for the block it ends in; and a chain's last
    block has the greatest index, because qEnd grows along a chain)"""
    best, pred = [], []
    for b, B in enumerate(blocks):
        m, mm = recount(q, t, B, 0)
        val, p = (m - 2 * mm, m, -1), None
        for a in range(b):
            v = overlap(blocks[a], B)
            if v is None:
                continue
            m, mm = recount(q, t, B, v)
            cand = (best[a][0] + m - 2 * mm, best[a][1] + m, best[a][2] - 1)
            if cand > val:
                val, p = cand, a
        best.append(val)
        pred.append(p)
    end = max(range(len(blocks)), key=lambda b: (best[b], -b))
    idx = [end]
    while pred[idx[-1]] is not None:
        idx.append(pred[idx[-1]])
    return chain_of(q, t, blocks, idx[::-1])


def best_chain(q, t, blocks):
    return best_chain_enumerated(q, t, blocks) if len(blocks) <= ENUMERATE_UP_TO else best_chain_table(q, t, blocks)


def row_of(i, j, o, t_len, blocks, parts):
    qn = qb = tn = tb = 0
    out = []
    for k, (b, v, m, mm) in enumerate(parts):
        d, a0, a1 = blocks[b][0], blocks[b][1] + v, blocks[b][2]
        if k:
            A = blocks[parts[k - 1][0]]
            if a0 - A[2] > 0:
                qn, qb = qn + 1, qb + a0 - A[2]
            if (a0 + d) - (A[2] + A[0]) > 0:
                tn, tb = tn + 1, tb + (a0 + d) - (A[2] + A[0])
        out.append((a1 - a0, a0, t_len - (a1 + d) if o else a0 + d))
    first, last = blocks[parts[0][0]], blocks[parts[-1][0]]
    t_start = t_len - (last[2] + last[0]) if o else first[1] + first[0]
    return (i, j, o, sum(p[2] for p in parts), sum(p[3] for p in parts), first[1], last[2], t_start, qn, qb, tn, tb, len(parts), tuple(out))


def brute_chain_rows(ref, rec, ss, min_matches=cc.MIN_MATCHES):
    rows = []
    qs = [s.upper() for _n, s in ref]
    ts = [s.upper() for _n, s in rec]
    for i, q in enumerate(qs):
        for j, x in enumerate(ts):
            best = None
            for o in ((0,) if ss else (0, 1)):
                t = cc.rc(x) if o else x
                blocks = blocks_of(q, t)
                if not blocks:
                    continue
                val, parts = best_chain(q, t, blocks)
                if best is None or val > best[0]:
                    best = (val, row_of(i, j, o, len(t), blocks, parts))
            if best is not None and best[1][3] >= min_matches:
                rows.append(best[1])
    return rows


@functools.lru_cache(maxsize=None)
def brute_of_case(name, ss, min_matches=cc.MIN_MATCHES):
    """the brute force's rows of a named case: computed once, shared by the tests, never changed (a tuple)"""
    ref, rec = CASES[name]()
    return tuple(brute_chain_rows(ref, rec, ss, min_matches))


def as_tuples(r):
    """a shannon_amd.compare.ChainRows as brute_chain_rows' list"""
    cols = [a.tolist() for a in r]
    off, size, bq, bt = cols[13], cols[14], cols[15], cols[16]
    return [tuple(row) + (tuple((size[x], bq[x], bt[x]) for x in range(off[k], off[k + 1])),) for k, row in enumerate(zip(*cols[:13]))]


def chain_rows_of(compare, rows):
    """brute_chain_rows' list as a shannon_amd.compare.ChainRows"""
    cols = [np.array([r[f] for r in rows], dtype=np.uint32) for f in range(13)]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r[13]) for r in rows])
    blocks = [np.array([b[f] for r in rows for b in r[13]], dtype=np.uint32) for f in range(3)]
    return compare.ChainRows(*(cols + [off] + blocks))


# ---------------------------------------------------------------------------------------------------------------- inputs
def differ(rng, s, *against):
    """s with base k replaced, where it equals one of against[.][k], by one that equals none (k over the shortest of them all)"""
    s = list(s)
    for k in range(min(len(x) for x in (s,) + against)):
        if any(s[k] == x[k] for x in against):
            free = [c for c in "ACGT" if all(c != x[k] for x in against)]
            s[k] = free[int(rng.integers(0, len(free)))]
    return "".join(s)


def pieces(rng, *lens):
    return [cc.rand_seq(rng, n) for n in lens]


def gapped(rng, la, lb, gq, gt):
    """(query, target) = A + X + B, A + Y + B: |X| = gq, |Y| = gt.  Four bases on either side of both seams are made to differ on
    the other block's diagonal, so the blocks are exactly A and B."""
    A, B, X, Y = pieces(rng, la, lb, gq, gt)
    # behind A on diagonal 0 stand (X + B)[k] and (Y + B)[k]; in front of B on its diagonal (A + X)[-1 - k] and (A + Y)[-1 - k].
    # One filler of 8 bases or more -- X if it has them, else Y -- is changed at its first and its last four bases.
    if gq >= 8:
        X = differ(rng, X[:4], (Y + B)[:4]) + X[4:-4] + differ(rng, X[-4:], (A + Y)[-4:])
    else:
        Y = differ(rng, Y[:4], (X + B)[:4]) + Y[4:-4] + differ(rng, Y[-4:], (A + X)[-4:])
    return A + X + B, A + Y + B


def gap_cases(seed=31):
    """two blocks around a gap in the target only (the target holds an exon the query skips), in the query only, in both (of
    different lengths); three exons of which the target lacks the middle one, and of which the query does"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = [gapped(rng, 40, 50, 0, 30), gapped(rng, 45, 35, 25, 0), gapped(rng, 40, 40, 30, 50)]
    A, B, Cc = pieces(rng, 50, 40, 60)
    B = differ(rng, B[:4], Cc[:4]) + B[4:-4] + differ(rng, B[-4:], A[-4:])
    pairs += [(A + B + Cc, A + Cc), (A + Cc, A + B + Cc)]
    return cc.named("r", [p[0] for p in pairs]), cc.named("x", [p[1] for p in pairs])


def tandem(rng, ll, v, lr, in_query=False):
    """(query, target) = L + M + R, L + M + M + R with |M| = v: block A = L + M on diagonal 0 and block B = M + R on diagonal v
    overlap by v in the query and by nothing in the target.  in_query: the duplication is the query's, the overlap the target's.
    The four bases behind A on its diagonal and in front of B on its diagonal are made to differ."""
    L, M, R = pieces(rng, ll, v, lr)
    for k in range(min(4, lr)):                                           # behind A: R[k] against (M + R)[k], left to right
        R = R[:k] + differ(rng, R[k], (M + R)[k]) + R[k + 1:]
    for k in range(1, 5):                                                 # in front of B: L[-k] against (L + M)[-k], right to left
        L = L[:ll - k] + differ(rng, L[-k], (L + M)[-k]) + L[ll - k + 1:]
    one, two = L + M + R, L + M + M + R
    return (two, one) if in_query else (one, two)


def trim_cases(seed=33):
    """an overlap v of 1, 31, 32, 33 and 70 with block B starting at query base 40, 41 and 71 of its sequence (and the sequences
    themselves at changing places of the packed texts)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = [tandem(rng, ll, v, 45) for v in (1, 31, 32, 33, 70) for ll in (40, 41, 71)]
    return cc.named("r", [p[0] for p in pairs]), cc.named("x", [p[1] for p in pairs])


def trim_edge_cases(seed=35):
    """v = len_B - 1: one base of B is left; v = len_B: the join is refused and the row is block A alone; a tandem duplication at
    the junction in the target (overlap in the query, none in the target) and in the query (the mirror)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = [tandem(rng, 30, 20, 1), tandem(rng, 30, 20, 0), tandem(rng, 50, 12, 60), tandem(rng, 50, 12, 60, in_query=True)]
    return cc.named("r", [p[0] for p in pairs]), cc.named("x", [p[1] for p in pairs])


def order_cases(seed=37):
    """two exons in swapped order (no join: the longer one is the row); crossing diagonals: A, B, C against A, C, B -- B and C
    cannot both stay, A -> B (the longer) wins over A -> C"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B = pieces(rng, 40, 60)
    A2, B2, C2 = pieces(rng, 40, 50, 30)
    B2 = differ(rng, B2[:4], C2[:4]) + B2[4:-4] + differ(rng, B2[-4:], A2[-4:])
    C2 = C2[:-4] + differ(rng, C2[-4:], A2[-4:])
    return cc.named("r", [A + B, A2 + B2 + C2]), cc.named("x", [B + A, A2 + C2 + B2])


def threshold_cases(seed=39):
    """two blocks of 20 matches each around a gap (a row only when chained); blocks of 20 and 20 that overlap by 11 (29 matches: no
    row) and by 10 (exactly 30)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = [gapped(rng, 20, 20, 0, 12), tandem(rng, 9, 11, 9), tandem(rng, 10, 10, 10)]
    return cc.named("r", [p[0] for p in pairs]), cc.named("x", [p[1] for p in pairs])


def tie_matches_case(seed=41):
    """equal sum S, decided by matches: X (70 bases, three substitutions: S = 61, 67 matches) and Y (61 bases, S = 61) in swapped
    order, so no join: X is the row"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X, Y = pieces(rng, 70, 61)
    return cc.named("r", [X + Y]), cc.named("x", [Y + cc.mutate(X, [17, 35, 52])])


def tie_blocks_case(seed=43):
    """equal S and matches, decided by fewer blocks: A -> B (20 + 20 around a gap) and Y (40) which can join neither"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q, t = gapped(rng, 20, 20, 0, 12)
    Y = cc.rand_seq(rng, 40)
    return cc.named("r", [q + "C" + Y]), cc.named("x", [Y + "G" + t])


def tie_index_case(seed=45):
    """equal values, decided by the block indices read backwards: Y1 and Y2 (40 each) in swapped order -- the row is Y1, the block of
    the smaller index; A1, A2 (30 each) swapped in front of B: A1 -> B and A2 -> B are worth the same, the smaller predecessor A1
    stays"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Y1, Y2, A1, A2, B = pieces(rng, 40, 40, 30, 30, 40)
    A1 = differ(rng, A1[:4], B[:4]) + A1[4:]
    A2 = differ(rng, A2[:4], B[:4]) + A2[4:-4] + differ(rng, A2[-4:], A1[-4:])
    return cc.named("r", [Y1 + Y2, A1 + A2 + B]), cc.named("x", [Y2 + Y1, A2 + A1 + B])


def tie_strand_case(seed=47):
    """equal values on both orientations ('+' stays): the target holds A + X + B forward and, behind it, A + X' + B reverse
    complemented"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q, t = gapped(rng, 30, 30, 0, 12)
    A, B = q[:30], q[30:]
    X2 = differ(rng, cc.rand_seq(rng, 12), B[:12], A[-12:])
    return cc.named("r", [q]), cc.named("x", [t + cc.rand_seq(rng, 7) + cc.rc(A + X2 + B)])


def minus_case(seed=49):
    """a chain on the '-' orientation: the target is the reverse complement of A + Y + B + Z + C"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q1, t1 = gapped(rng, 40, 30, 0, 20)
    q2, t2 = gapped(rng, 30, 50, 9, 0)
    return cc.named("r", [q1 + q2]), cc.named("x", [cc.rand_seq(rng, 5) + cc.rc(t1 + t2) + cc.rand_seq(rng, 11)])


def n_trim_cases(seed=51):
    """N inside the stretch a block loses: in the query's M (both blocks run over it), and in the target's second M"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q1, t1 = tandem(rng, 30, 40, 30)
    q2, t2 = tandem(rng, 33, 40, 30)
    return cc.named("r", [cc.with_n(q1, [50]), q2]), cc.named("x", [t1, cc.with_n(t2, [33 + 40 + 17])])


def group_case(n, seed=53):
    """one (query, target) pair of n blocks: the target is n pieces of 20 bases, the query the same pieces with one base inserted
    between neighbours, so piece k lies on diagonal -k"""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    P = pieces(rng, *([20] * n))
    return cc.named("r", ["".join(p + "ACGT"[(k * 7) % 4] for k, p in enumerate(P))[:-1]]), cc.named("x", ["".join(P)])


def random_cases(n_cases=40, seed=301):
    """small random inputs: 2-5 exons of 16-70 bases; 1-3 queries that are exon subsets in order; 1-4 targets, each a query with an
    exon skipped, an exon doubled, an indel of 1-9 bases, 0-2 % substitutions, now and then reverse complemented or holding an N"""
    out = []
    for c in range(n_cases):
        rng = np.random.Generator(np.random.PCG64(seed + c))
        exons = [cc.rand_seq(rng, int(rng.integers(16, 71))) for _ in range(int(rng.integers(2, 6)))]
        ref = []
        for _ in range(int(rng.integers(1, 4))):
            keep = [e for e in exons if rng.random() < 0.8] or exons[:1]
            ref.append("".join(keep))
        rec = []
        for _ in range(int(rng.integers(1, 5))):
            parts = [e for e in exons if rng.random() < 0.75] or exons[-1:]
            if rng.random() < 0.3:
                k = int(rng.integers(0, len(parts)))
                parts = parts[:k + 1] + parts[k:]
            t = "".join(parts)
            for _e in range(int(rng.integers(0, 3))):
                p, n = int(rng.integers(0, len(t))), int(rng.integers(1, 10))
                t = t[:p] + (cc.rand_seq(rng, n) if rng.random() < 0.5 else "") + t[p + (n if rng.random() < 0.5 else 0):]
            t = cc.mutate(t, np.nonzero(rng.random(len(t)) < rng.choice([0.0, 0.01, 0.02]))[0])
            if rng.random() < 0.15 and len(t):
                t = cc.with_n(t, rng.integers(0, len(t), 2))
            rec.append(cc.rc(t) if rng.random() < 0.4 else t)
        out.append((cc.named("r", ref), cc.named("x", rec)))
    return out


CASES = {"gaps": gap_cases, "trims": trim_cases, "trim edges": trim_edge_cases, "order": order_cases, "thresholds": threshold_cases,
         "tie: matches": tie_matches_case, "tie: blocks": tie_blocks_case, "tie: index": tie_index_case, "tie: strand": tie_strand_case,
         "minus": minus_case, "N in a trim": n_trim_cases}
GROUP_SIZES = (1, 2, 63, 64, 65, 130)
for _n in GROUP_SIZES:
    CASES["group of %d" % _n] = functools.partial(group_case, _n)
