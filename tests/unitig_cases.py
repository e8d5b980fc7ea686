"""Inputs and expectations for the batched unitig contraction (shn_unitigs_build, csrc/graph_gpu.hip), from the oracle alone.

The expectation for one partition is what load_single_jellyfish + the first Node.condense_all leave behind
(oracle.mbgraph.MBGraph.load_k1mers + condense_all): the final nodes in creation order, every node's out- and in-list in list
order, and the live edges in creation order (an MBGraph whose `link` stamps a serial number on each edge it creates: `link` is
the only place edges are made).  The cycle flag is held against a predicate computed from the rows, not against the kernel's
own notion.  The generators are seeded (random.Random); nothing is read from files.

Shared by tests/test_unitig_cases.py (CPU: the inputs are what they claim to be) and tests/test_unitigs_gpu.py."""
import random
import numpy as np
from oracle import mbgraph as omb

KS = (2, 4, 6, 12, 24, 25, 31)


# ---------------------------------------------------------------- the reference side
def rows_of(contigs, K):
    """the partition's k1-mer rows: every (K+1)-window of every contig of at least K+1 bases, in order"""
    return [c[i:i + K + 1] for c in contigs if len(c) >= K + 1 for i in range(len(c) - K)]


class StampedGraph(omb.MBGraph):
    """MBGraph that remembers the order in which its edges were created"""

    def __init__(self, K, L):
        super(StampedGraph, self).__init__(K, L)
        self.serial = {}

    def link(self, a, b, w):
        e = omb.Edge(w, a, b)
        self.serial[e] = len(self.serial)
        return e


def cycle_predicate(rows, K):
    """True iff the raw K-mer graph of the rows holds a pure cycle of condensable edges: links u -> v with outdeg(u) = 1,
    indeg(v) = 1, u != v (degrees counted per row, repeated rows included), and a component of links without a head."""
    ids = {}
    edges = []
    for r in rows:
        a, b = r[:-1], r[1:]
        u = ids.setdefault(a, len(ids))
        v = ids.setdefault(b, len(ids))
        edges.append((u, v))
    n = len(ids)
    outdeg, indeg = [0] * n, [0] * n
    for u, v in edges:
        outdeg[u] += 1
        indeg[v] += 1
    succ, pred = [-1] * n, [-1] * n
    for u, v in edges:
        if outdeg[u] == 1 and indeg[v] == 1 and u != v:
            succ[u] = v
            pred[v] = u
    reached = [False] * n
    for h in range(n):
        if pred[h] == -1:
            u = h
            while u != -1:
                reached[u] = True
                u = succ[u]
    return not all(reached)


def expected(contigs, K):
    """What the partition must look like after loading and the first condense_all."""
    rows = rows_of(contigs, K)
    g = StampedGraph(K, 0)
    g.load_k1mers([(r, 1) for r in rows])
    nk = len(g.nodes)
    g.condense_all()
    index = {id(n): i for i, n in enumerate(g.nodes)}
    live = sorted((g.serial[e], index[id(n)], index[id(e.out_node)]) for n in g.nodes for e in n.out_edges)
    return {"rows": rows, "n_kmers": nk, "cyclic": cycle_predicate(rows, K),
            "bases": [n.bases for n in g.nodes],
            "count": [int(n.count) for n in g.nodes],
            "prevalence": [int(n.prevalence) for n in g.nodes],
            "merged": [n.nid >= nk for n in g.nodes],
            "out_lists": [[index[id(e.out_node)] for e in n.out_edges] for n in g.nodes],
            "in_lists": [[index[id(e.in_node)] for e in n.in_edges] for n in g.nodes],
            "edge_seq": [(s, d) for _, s, d in live]}


def lists_of(view, n_nodes):
    """(out-lists, in-lists) of the nodes from the edge arrays of Unitigs.partition(): every node's ranks must be a permutation of
    0 .. degree-1"""
    outs = [[] for _ in range(n_nodes)]
    ins = [[] for _ in range(n_nodes)]
    for s, d, ro, ri in zip(view["e_src"].tolist(), view["e_dst"].tolist(), view["e_out_rank"].tolist(), view["e_in_rank"].tolist()):
        assert s < n_nodes and d < n_nodes, ("edge end out of range", s, d, n_nodes)
        outs[s].append((ro, d))
        ins[d].append((ri, s))
    res = []
    for lists in (outs, ins):
        cur = []
        for i, l in enumerate(lists):
            l.sort()
            assert [r for r, _ in l] == list(range(len(l))), ("ranks are not a permutation", i, l)
            cur.append([x for _, x in l])
        res.append(cur)
    return res


def compare(view, exp, K, what=""):
    """Unitigs.partition(p) against expected(): equality of everything, order included.  Returns True when the graph itself was
    compared, False for a partition flagged cyclic (only the K-mer count and the flag are defined then)."""
    assert view["n_kmers"] == exp["n_kmers"], (what, "n_kmers", view["n_kmers"], exp["n_kmers"])
    assert view["cyclic"] == exp["cyclic"], (what, "cyclic flag", view["cyclic"], exp["cyclic"])
    if exp["cyclic"]:
        return False
    n = len(exp["bases"])
    assert len(view["bases"]) == n, (what, "final nodes", len(view["bases"]), n)
    for i in range(n):
        assert view["bases"][i] == exp["bases"][i], (what, "bases of node", i)
    n_len, tail = view["n_len"].tolist(), view["n_tail_out"].tolist()
    assert n_len == exp["count"], (what, "n_len")
    assert [(K - 1) * ((n_len[i] - 1) + tail[i]) for i in range(n)] == exp["prevalence"], (what, "prevalence")
    assert len(view["e_src"]) == len(exp["edge_seq"]), (what, "edges", len(view["e_src"]), len(exp["edge_seq"]))
    outs, ins = lists_of(view, n)
    for i in range(n):
        assert outs[i] == exp["out_lists"][i], (what, "out-list of node", i, outs[i], exp["out_lists"][i])
        assert ins[i] == exp["in_lists"][i], (what, "in-list of node", i, ins[i], exp["in_lists"][i])
    got = list(zip(view["e_src"].tolist(), view["e_dst"].tolist()))
    if got != exp["edge_seq"]:
        at = next(i for i in range(len(got)) if got[i] != exp["edge_seq"][i])
        raise AssertionError((what, "edge order differs first at edge", at, got[at], exp["edge_seq"][at]))
    return True


def list_order_stats(exp, K):
    """How the expectation departs from row order: (nodes with >= 2 out-edges, of these with an out-list that is not in the row
    order of its junction k1-mers, nodes with >= 2 in-edges, of these with an in-list not in row order)"""
    first_row = {}
    for i, r in enumerate(exp["rows"]):
        first_row.setdefault(r, i)
    b = exp["bases"]
    mo = do = mi = di = 0
    for i in range(len(b)):
        o = [first_row[b[i][-K:] + b[j][K - 1]] for j in exp["out_lists"][i]]
        if len(o) >= 2:
            mo += 1
            do += o != sorted(o)
        o = [first_row[b[j][-K] + b[i][:K]] for j in exp["in_lists"][i]]
        if len(o) >= 2:
            mi += 1
            di += o != sorted(o)
    return mo, do, mi, di


# ---------------------------------------------------------------- generators
def rnd_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def cut_pieces(rng, contig, K, lo=20, hi=150):
    """the contig as pieces that overlap by exactly K bases: neighbours share a K-mer and no k1-mer, every k1-mer is in one piece"""
    if len(contig) < K + 1:
        return [contig]
    out, a = [], 0
    while True:
        n = rng.randint(max(lo, K + 1), max(hi, K + 1))
        if len(contig) - (a + n - K) < K + 1:            # what would be left holds no k1-mer: take it along
            out.append(contig[a:])
            return out
        out.append(contig[a:a + n])
        a += n - K


def distinct_runs(seqs_, K):
    """contigs with distinct k1-mers, as the extension leaves them: a run is cut where the next k1-mer was seen already"""
    seen, out = set(), []
    for s in seqs_:
        start = None
        for i in range(len(s) - K):
            w = s[i:i + K + 1]
            if w in seen:
                if start is not None:
                    out.append(s[start:i + K])
                    start = None
            else:
                seen.add(w)
                if start is None:
                    start = i
        if start is not None:
            out.append(s[start:])
    return out


def family_sequences(rng, K, n_families=8, n_seqs=7, length=600):
    """random base sequences with variants: a few SNPs or a deletion of K .. 2K bases each"""
    out = []
    for _ in range(n_families):
        base = rnd_seq(rng, length)
        out.append(base)
        for v in range(n_seqs - 1):
            s = list(base)
            if v % 3 == 2:
                a = rng.randrange(K, length - 3 * K - 1)
                del s[a:a + rng.randint(K, 2 * K)]
            else:
                for _s in range(rng.randint(2, 5)):
                    p = rng.randrange(length)
                    s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
            out.append("".join(s))
    return out


def family_case(K, seed, distinct=True, shuffle=True, **kw):
    """(contigs of one partition, the sequences they come from)"""
    rng = random.Random(seed * 1000 + K)
    seqs_ = family_sequences(rng, K, **kw)
    contigs = distinct_runs(seqs_, K) if distinct else list(seqs_)
    if shuffle:
        contigs = [p for c in contigs for p in cut_pieces(rng, c, K)]
        rng.shuffle(contigs)
    return contigs, seqs_


def cyclic_seq(rng, K):
    """a sequence whose K-windows, read around the circle, are all different"""
    n = 200 if K >= 12 else 2 * K
    while True:
        s = rnd_seq(rng, n)
        w = [(s + s)[i:i + K] for i in range(n)]
        if len(set(w)) == n:
            return s


def named_shapes(K, seed=5):
    """[(name, contigs, sequences to sample reads from, designed to hold a pure cycle)], each a partition of its own"""
    rng = random.Random(seed * 1000 + K)
    long_ = rnd_seq(rng, 5000 + K + 200)
    pieces = cut_pieces(rng, long_, K)
    rng.shuffle(pieces)
    cyc, cyc2, cyc3 = cyclic_seq(rng, K), cyclic_seq(rng, K), cyclic_seq(rng, K)
    rep = cyclic_seq(rng, K)
    m = rnd_seq(rng, 60 + K)
    fork = [rnd_seq(rng, 40) + m + rnd_seq(rng, 40), rnd_seq(rng, 40) + m[:K], m[-K:] + rnd_seq(rng, 40)]
    inside = rnd_seq(rng, 100) + "C" * (K + 30) + rnd_seq(rng, 100)
    if K >= 12:
        side = rnd_seq(rng, 150 + K)
        beside = [side, cyc2 + cyc2[:K], rnd_seq(rng, K + 1), cyc3 + cyc3[:K]]
    else:
        # (few K-mers exist: random neighbours would run through the cycle's K-mers.  A homopolymer that is not on the cycle
        # leaves it pure and still puts a node of its own beside it)
        x = next(c for c in "ACGT" if c * K not in (cyc2 + cyc2))
        side = x * (K + 5)
        beside = [side, cyc2 + cyc2[:K]]
    shapes = [
        ("empty_first", [], [], False),
        ("linear_long", [long_], [long_], False),
        ("linear_long_pieces", pieces, [long_], False),
        ("poly_a", ["A" * (K + 40)], ["A" * (K + 40)], False),
        ("poly_t", ["T" * (K + 40)], ["T" * (K + 40)], False),
        ("homopolymer_inside", [inside], [inside], False),
        ("empty_middle", [], [], False),
        ("pure_cycle", [cyc + cyc[:K]], [cyc + cyc], True),
        ("pure_cycle_beside_others", beside, [side, cyc2 + cyc2], True),
        ("cycle_with_tail", [rnd_seq(rng, 50 + K) + cyc + cyc[:K]], [cyc + cyc], False),
        ("twice_around", [rep + rep + rep[:K]], [rep + rep], False),
        ("fork_and_join", fork, fork[:1], False),
        ("k_plus_one", [rnd_seq(rng, K + 1)], [], False),
        ("k_plus_one_k_and_fewer", [rnd_seq(rng, K), rnd_seq(rng, K + 1), rnd_seq(rng, K - 1), rnd_seq(rng, 1), rnd_seq(rng, K + 1)], [], False),
        ("all_short", [rnd_seq(rng, K), rnd_seq(rng, 1), rnd_seq(rng, K - 1)], [], False),
        ("empty_last", [], [], False),
    ]
    return shapes


def sample_reads(seqs_, L, n, seed):
    rng = random.Random(seed)
    src = [s for s in seqs_ if len(s) >= L]
    out = []
    for _ in range(n if src else 0):
        s = rng.choice(src)
        a = rng.randrange(len(s) - L + 1)
        out.append(s[a:a + L])
    return out


def full_batch(K):
    """every named shape and the family cases (with and without the distinct-k1-mer step) in one call: [(name, contigs, designed
    cyclic)]; the batch ends in a partition without contigs (n_parts beyond the last part_of)"""
    shapes = [(n, c, d) for n, c, _s, d in named_shapes(K)]
    fam = [("family", family_case(K, 1)[0], False), ("family_repeated_rows", family_case(K, 2, distinct=False)[0], False),
           ("walk_order_control", family_case(K, 3, shuffle=False)[0], False)]
    return shapes[:6] + fam[:1] + shapes[6:10] + fam[1:] + shapes[10:]


def many_nodes_batch(K=25, seed=9):
    """>= 4 partitions with >= 4,096 final nodes in all (the host assembly then runs on threads): partitions of many short contigs
    (every contig a final node) between family partitions (edges)"""
    rng = random.Random(seed)
    out = []
    for i in range(5):
        out.append(("short_contigs_%d" % i, [rnd_seq(rng, rng.randint(K + 1, 2 * K)) for _ in range(1000)], False))
        if i % 2 == 0:
            out.append(("family_%d" % i, family_case(K, 20 + i)[0], False))
    return out


def large_batch(K=25, seed=13, n_parts=7):
    """roughly 0.3 M K-mers in one call: several blocks per kernel, contended atomics"""
    out = []
    for i in range(n_parts):
        out.append(("large_%d" % i, family_case(K, seed + i, n_families=20, n_seqs=5, length=2000)[0], False))
    return out


def flat_text_of(parts):
    """(text, off, part_of, n_contigs) of the partitions' contigs, as kmers_for_component lays them out"""
    flat = [c for cl in parts for c in cl]
    text = np.frombuffer("".join(flat).encode(), dtype=np.uint8) if flat else np.zeros(1, np.uint8)
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        off[1:] = np.cumsum([len(c) for c in flat], dtype=np.uint64)
    part_of = np.ascontiguousarray(np.repeat(np.arange(len(parts), dtype=np.uint32), [len(cl) for cl in parts]), dtype=np.uint32) \
        if flat else np.zeros(1, np.uint32)
    return text, off, part_of, len(flat)
