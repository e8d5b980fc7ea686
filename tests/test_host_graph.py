"""CPU: the product's host-side graph / sparse-flow logic (shannon_amd/mbgraph.py,
shannon_amd/sparse_flow.py) against the reference goldens.  Partition inputs come from the oracle
front stages; the LP trials are solved by the oracle's transport_vertex here (the HIP kernel is
checked against it bit for bit in tests/test_lp_gpu.py)."""
import numpy as np
import pytest
from golden_util import *
from oracle import seqs, count, extension, partition, lp as olp
from shannon_amd import mbgraph, sparse_flow, kmers_for_component as kfc

CASES = sorted(MANIFEST)


def oracle_solve_batch(ctx, reqs, seed):
    out = []
    for q in reqs:
        xs = np.zeros((q.m * q.n, q.trials))
        for t in range(q.trials):
            cc = olp.trial_costs(seed, q.pid, t, q.m * q.n)
            c = [[(cc[j * q.m + i] if q.p[j * q.m + i] > 0 else 0) for j in range(q.n)] for i in range(q.m)]
            x = olp.transport_vertex(q.a_s, q.b_s, c)
            for k in range(q.m * q.n):
                xs[k, t] = x[k % q.m][k // q.m]
        out.append(xs)
    return out


@pytest.mark.parametrize("name", CASES)
def test_product_graph_stage(name):
    g = load_case(name)
    K, paired = g["K"], g["paired"]
    psize = MANIFEST[name].get("partition_size", 500)
    inp = load_inputs(name)
    dbl = read_files(name, inp)
    tab = count.count_k1mers_dict([r for f in dbl for r in f], K + 1)
    res = extension.run_correction([(k, tab[k]) for k in sorted(tab, reverse=True)], comp_size_threshold=psize)
    pv = [part_vectors(len(cl), psize) for cl, _ in res.big_components]
    nc, k2c = partition.build_partitions([b[0] for b in res.big_components], [p[0] for p in pv], [p[1] for p in pv] if pv else None,
                                         res.remaining, res.allowed, K)
    if paired:
        o1, o2 = partition.route_reads_paired(dbl[0], dbl[1], nc, k2c, K)
    else:
        o1 = partition.route_reads(dbl[0], nc, k2c, K)
    files, _ = partition.partition_k1mers(nc, k2c, K)
    for comp, gp in g["partitions"].items():
        reads = [o1[comp], o2[comp]] if paired else [o1[comp]]
        gr, singles, comps = mbgraph.run_partition(files[comp], reads, K, paired)
        can = mbgraph.canonical(singles, comps)
        for k in can:
            assert approx_eq(can[k], gp["graph"][k]), (comp, k)
        assert [l for l in gr.log if "Bridged" in l] == [l for l in gp["mb_log"] if "Bridged" in l]


@pytest.mark.parametrize("name", CASES)
def test_product_sparse_flow_host_logic(name, monkeypatch):
    monkeypatch.setattr(sparse_flow, "solve_batch", oracle_solve_batch)
    g = load_case(name)
    seed = MANIFEST[name]["sf_seed"]
    for comp, gp in g["partitions"].items():
        comps = [(rc["nodes"], rc["edges"], rc["paths"]) for rc in gp["raw_components"]]
        trs = sparse_flow.sparse_flow_components(None, comps, seed)
        mine = "".join(sparse_flow.fasta_records("", str(c), tr) for c, tr in enumerate(trs))
        mine += sparse_flow.single_nodes_fasta("", gp["single_rows"])
        ref, mine = parse_fasta(gp["reconstructed_fasta"]), parse_fasta(mine)
        assert len(ref) == len(mine)
        for (h1, s1), (h2, s2) in zip(ref, mine):
            assert s1 == s2
            t1, t2 = h1.split("\t"), h2.split("\t")
            assert t1[0] == t2[0] and t1[2:] == t2[2:]
            if "Copycount" in t1[1]:
                assert t1[1] == t2[1]
            else:
                assert abs(float(t1[1]) - float(t2[1])) <= 1e-9 * max(1.0, abs(float(t1[1])))


_ORACLE_WALKS = {}


def _oracle_walks(name):
    """(k1-mer items, the seed loop's walks) of a golden case: walked once, shared by the thresholds"""
    if name not in _ORACLE_WALKS:
        dbl = read_files(name, load_inputs(name))
        tab = count.count_k1mers_dict([r for f in dbl for r in f], load_case(name)["K"] + 1)
        items = [(k, tab[k]) for k in sorted(tab, reverse=True)]
        kmers, k1 = extension.load_kmers(items)
        _ORACLE_WALKS[name] = (items, list(extension.python_walks(kmers, k1, 3)))
    return _ORACLE_WALKS[name]


# (case, threshold) -> (contigs per remaining bin, big components): the bin roll-over, the trailing empty bin and the METIS text
_BINS_PINNED = {("se_K24", 3): ([4, 4, 4, 0], 0), ("syn_pe_L250_K20_part1", 3): ([4, 2], 1), ("se_K24", 1): (None, 6)}


@pytest.mark.parametrize("threshold", [500, 3, 1])
@pytest.mark.parametrize("name", ["se_K24", "syn_part_s33", "syn_pe_L250_K20_part1"])
def test_bin_components_against_the_oracle(name, threshold):
    """extension_correction.bin_components (native DFS components, bins, METIS text) over the oracle's contigs and connections ==
    the oracle's components, single contigs, remaining bins and big components (extension_correction.py:417-513)"""
    from shannon_amd import extension_correction as ec
    items, walks = _oracle_walks(name)
    ref = extension.run_correction(items, comp_size_threshold=threshold, walks=walks)
    assert list(ref.connections) == list(range(1, len(ref.contigs) + 1))
    coff, cnb, cw = [0], [], []                              # the connections dict as CSR, in insertion order
    for a in ref.connections:
        cnb += list(ref.connections[a].keys())
        cw += list(ref.connections[a].values())
        coff.append(len(cnb))
    if (name, threshold) in _BINS_PINNED:
        bins, n_big = _BINS_PINNED[(name, threshold)]
        assert len(ref.big_components) == n_big and (bins is None or [len(b) for b in ref.remaining] == bins)
    got = ec.bin_components(ref.contigs, coff, cnb, cw, threshold)
    assert got.components == ref.components and list(got.components) == list(ref.components)
    assert got.connections == ref.connections and [list(v) for v in got.connections.values()] == [list(v) for v in ref.connections.values()]
    assert got.single_contigs == ref.single_contigs and [ref.contigs[i] for i in got.single_ids] == ref.single_contigs
    assert got.remaining == ref.remaining
    assert got.big_components == ref.big_components


def test_own_partitioner_is_balanced_and_deterministic():
    rng = np.random.default_rng(0)
    n = 300
    adj = [dict() for _ in range(n)]
    for _ in range(900):
        a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
        if a != b:
            w = int(rng.integers(1, 9))
            adj[a][b] = w
            adj[b][a] = w
    text = "%d\t%d\t001\n" % (n, sum(len(d) for d in adj) // 2) + "".join(
        "".join("%d\t%d\t" % (b + 1, w) for b, w in d.items()) + "\n" for d in adj)
    p = kfc.partition_graph(text, 6, 1000)
    assert p == kfc.partition_graph(text, 6, 1000)
    sizes = np.bincount(p, minlength=6)
    assert sizes.sum() == n and sizes.max() <= 2 * n / 6 and set(p) == set(range(6))


def test_own_partitioner_cut_quality():
    """The gpmetis stand-in against what bounds it (a8: gpmetis itself is external and heuristic -- parity unpinned; this measures
    the quality of the stand-in, a multilevel scheme like METIS's own): on graphs with a planted partition (dense inside the groups,
    sparse between them, vertices in random order; up to 6,000 contigs in 12 parts) the edge cut of partition_graph is within 15 %
    of the planted cut (the one-level greedy growth + refinement of rounds 1-3 ended 45 % above it at 1,000 vertices), far below a
    random balanced partition's, the balance bound holds, and the refinement never raises the cut of what it is given."""
    import math
    for seed, n, P, p_in, p_out in ((1, 400, 4, 0.06, 0.002), (2, 600, 6, 0.05, 0.003), (3, 1000, 10, 0.04, 0.001), (4, 6000, 12, 0.012, 0.0002)):
        rng = np.random.default_rng(seed)
        group = rng.permutation(n) % P
        M = rng.random((n, n))
        E = np.triu(M < np.where(group[:, None] == group[None, :], p_in, p_out), 1)
        ai, bi = np.nonzero(E)
        ws = rng.integers(1, 9, len(ai))
        adj = [dict() for _ in range(n)]
        for a, b, w in zip(ai.tolist(), bi.tolist(), ws.tolist()):
            adj[a][b] = w
            adj[b][a] = w
        text = "%d\t%d\t001\n" % (n, sum(len(d) for d in adj) // 2) + "".join(
            "".join("%d\t%d\t" % (b + 1, w) for b, w in d.items()) + "\n" for d in adj)
        al = kfc.parse_metis(text)
        mine = kfc.partition_graph(text, P, 1000)
        assert mine == kfc.partition_graph(text, P, 1000)                                   # deterministic
        cut = kfc.edge_cut(al, mine)
        planted = kfc.edge_cut(al, [int(g) for g in group])
        rnd = kfc.edge_cut(al, [int(x) for x in rng.permutation(n) % P])
        sizes = np.bincount(mine, minlength=P)
        assert sizes.sum() == n and sizes.min() >= 1 and sizes.max() <= 2.0 * n / P
        assert cut <= 1.15 * planted, (seed, cut, planted, rnd)                             # near the planted cut ...
        assert cut <= 0.5 * rnd, (seed, cut, planted, rnd)                                  # ... and far below a random partition's
        # the one-level scheme of rounds 1-3 (growth + refinement, no coarsening) is what the levels improve on
        flat = kfc.edge_cut(al, kfc.refine_partition(al, kfc._grow_partition(al, [1] * n, P), P, 1000))
        assert cut <= flat * 1.02, (seed, cut, flat)
        # the refinement only ever lowers the cut of what it is given
        assert kfc.edge_cut(al, kfc.refine_partition(al, [int(x) for x in rng.permutation(n) % P], P, 1000)) <= rnd


def _planted_graph(seed, n, P, deg_in, deg_out):
    """sparse planted partition: every vertex draws ~deg_in neighbours inside its group and ~deg_out outside (edge lists, not an
    n x n matrix: 50,000 vertices)"""
    rng = np.random.default_rng(seed)
    group = rng.permutation(n) % P
    members = [np.nonzero(group == g)[0] for g in range(P)]
    adj = [dict() for _ in range(n)]
    for v in range(n):
        inside = members[group[v]]
        for u in inside[rng.integers(0, len(inside), deg_in)].tolist() + rng.integers(0, n, deg_out).tolist():
            if u != v and (group[u] == group[v] or rng.random() < 1.0):
                w = int(rng.integers(1, 9))
                adj[v][u] = w
                adj[u][v] = w
    text = "%d\t%d\t001\n" % (n, sum(len(d) for d in adj) // 2) + "".join(
        "".join("%d\t%d\t" % (b + 1, w) for b, w in d.items()) + "\n" for d in adj)
    return text, group


def test_native_partitioner_equals_its_python_mirror():
    """shn_partition_metis / shn_metis_reweight (csrc/partition_host.hip) make the decisions of multilevel_partition /
    weight_updated_graph_py one for one: equal vectors and equal texts on random graphs of several shapes, vertices without
    neighbours and the two-run chain of kmers_for_component.py:221-234 included."""
    for seed, n, P, din, dout in ((1, 1, 1, 0, 0), (2, 7, 2, 2, 1), (3, 90, 3, 3, 1), (4, 700, 5, 4, 1), (5, 3000, 9, 5, 1), (6, 2500, 30, 3, 2)):
        text, _g = _planted_graph(seed, n, P, din, dout)
        a = kfc.partition_graph(text, P, 1000)
        assert a == kfc.partition_graph_py(text, P, 1000), (seed, n, P)
        t2 = kfc.weight_updated_graph(text, a, 5)
        assert t2 == kfc.weight_updated_graph_py(text, a, 5)
        assert kfc.partition_graph(t2, P, 1000) == kfc.partition_graph_py(t2, P, 1000)
        assert kfc.partition_graph(text, P, 300) == kfc.partition_graph_py(text, P, 300)        # a tighter balance bound


def test_native_partitioner_at_fifty_thousand_contigs():
    """the size of a real transcriptome's shared-exon component: 50,000 vertices in 100 parts (the reference's
    cap, kmers_for_component.py:217) -- within 15 % of the planted cut, balanced, deterministic, in seconds"""
    import time
    n, P = 50000, 100
    text, group = _planted_graph(11, n, P, 6, 1)
    t0 = time.time()
    mine = kfc.partition_graph(text, P, 1000)
    dt = time.time() - t0
    assert mine == kfc.partition_graph(text, P, 1000)
    al = kfc.parse_metis(text)
    cut, planted = kfc.edge_cut(al, mine), kfc.edge_cut(al, [int(g) for g in group])
    sizes = np.bincount(mine, minlength=P)
    assert sizes.sum() == n and sizes.min() >= 1 and sizes.max() <= 2.0 * n / P
    assert cut <= 1.15 * planted, (cut, planted)
    assert dt < 20.0, dt
    p2 = kfc.partition_graph(kfc.weight_updated_graph(text, mine, 5), P, 1000)               # the r2 run on the re-weighted graph
    assert np.bincount(p2, minlength=P).max() <= 2.0 * n / P


@pytest.mark.parametrize("name", CASES)
def test_native_contig_graph_matches_oracle(name):
    """shn_contig_graph (native host code, no GPU needed): duplicate_check + contig graph in the
    reference's order, fed with the oracle's unfiltered candidate contigs."""
    import ctypes as C, math
    from shannon_amd import _lib, build
    build.build(verbose=False)
    g = load_case(name)
    K = g["K"]
    inp = load_inputs(name)
    dbl = read_files(name, inp)
    tab = count.count_k1mers_dict([r for f in dbl for r in f], K + 1)
    kmers, k1 = extension.load_kmers([(k, tab[k]) for k in sorted(tab, reverse=True)])
    heaviest = sorted(kmers.items(), key=lambda kv: kv[1])
    traversed, cands = set(), []
    while heaviest:
        s, w = heaviest.pop()
        if w < 3:
            break
        if s in traversed:
            continue
        traversed.add(s)
        r_, rw, rn = extension._extend(s, True, traversed, kmers, k1)
        l_, lw, ln = extension._extend(s, False, traversed, kmers, k1)
        contig = "".join(reversed(l_)) + s + "".join(r_)
        avg = (rw + lw + kmers[s]) / max(1, rn + ln + 1)
        if len(contig) >= 75 and len(contig) * math.pow(avg, 0.25) >= 2 * 75 * math.pow(3, 0.25):
            cands.append(contig)
    ref = extension.run_correction([(k, tab[k]) for k in sorted(tab, reverse=True)])
    buf = np.frombuffer("".join(cands).encode(), dtype=np.uint8)
    offs = np.zeros(len(cands) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c) for c in cands])
    acc = np.zeros(len(cands), dtype=np.int32)
    na, nc = C.c_uint64(0), C.c_uint64(0)
    L = _lib.lib()
    _lib.check(L.shn_contig_graph(buf.ctypes.data, offs.ctypes.data, len(cands), k1, 15, 0.5, acc.ctypes.data, C.byref(na), None, None, None, C.byref(nc)))
    coff = np.zeros(na.value + 1, dtype=np.uint64)
    cnb = np.zeros(max(1, nc.value), dtype=np.int32)
    cw = np.zeros(max(1, nc.value), dtype=np.int32)
    _lib.check(L.shn_contig_graph(buf.ctypes.data, offs.ctypes.data, len(cands), k1, 15, 0.5, acc.ctypes.data, C.byref(na), coff.ctypes.data,
                                  cnb.ctypes.data, cw.ctypes.data, C.byref(nc)))
    assert [cands[i] for i in np.nonzero(acc)[0]] == ref.contigs
    conn = {a + 1: list(zip(cnb[int(coff[a]):int(coff[a + 1])].tolist(), cw[int(coff[a]):int(coff[a + 1])].tolist())) for a in range(na.value)}
    assert conn == {k: list(v.items()) for k, v in ref.connections.items()}      # same neighbours, weights AND insertion order


@pytest.mark.parametrize("name", CASES)
def test_native_graph_stage(name):
    """shn_mbgraph_run (native host code) == the Python mirror == the reference goldens."""
    from shannon_amd import mbgraph_native, build
    build.build(verbose=False)
    g = load_case(name)
    K, paired = g["K"], g["paired"]
    psize = MANIFEST[name].get("partition_size", 500)
    inp = load_inputs(name)
    dbl = read_files(name, inp)
    tab = count.count_k1mers_dict([r for f in dbl for r in f], K + 1)
    res = extension.run_correction([(k, tab[k]) for k in sorted(tab, reverse=True)], comp_size_threshold=psize)
    pv = [part_vectors(len(cl), psize) for cl, _ in res.big_components]
    nc, k2c = partition.build_partitions([b[0] for b in res.big_components], [p[0] for p in pv], [p[1] for p in pv] if pv else None,
                                         res.remaining, res.allowed, K)
    if paired:
        o1, o2 = partition.route_reads_paired(dbl[0], dbl[1], nc, k2c, K)
    else:
        o1 = partition.route_reads(dbl[0], nc, k2c, K)
    files, _ = partition.partition_k1mers(nc, k2c, K)
    for comp, gp in g["partitions"].items():
        reads = [o1[comp], o2[comp]] if paired else [o1[comp]]
        singles, comps, log = mbgraph_native.run_partition(files[comp], reads, K, paired)
        gr, s2, c2 = mbgraph.run_partition(files[comp], reads, K, paired)
        assert singles == s2                       # identical to the Python mirror, IDs and order included
        assert comps == c2
        assert ["Bridged %d nodes" % b for b in log["bridged"]] == [l for l in gr.log if "Bridged" in l]
        can = mbgraph.canonical(singles, comps)
        for k in can:
            assert approx_eq(can[k], gp["graph"][k]), (comp, k)


@pytest.mark.parametrize("name", CASES[:3])
def test_native_graph_stage_parallel_read_dedup(name, monkeypatch):
    """Large read sets are de-duplicated by several host threads (hash-sharded) and numbered in file order afterwards;
    forced here on the small golden cases: same graph as reading one read at a time."""
    monkeypatch.setenv("SHN_GRAPH_BULK_MIN", "1")
    test_native_graph_stage(name)


def test_native_find_reps_matches_python_and_oracle():
    """shn_find_reps (native) == shannon_amd.post.find_reps (Python) == oracle.post.find_reps."""
    import random
    from shannon_amd import post, build
    from oracle import post as opost
    build.build(verbose=False)
    rnd = random.Random(11)
    base = ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(150, 700))) for _ in range(60)]
    recs = []
    for i, b in enumerate(base):
        recs.append((">T%d x" % i, b))
        if i % 3 == 0:
            recs.append((">C%d" % i, b[7:-9] if len(b) > 260 else b))
        if i % 4 == 0:
            recs.append((">R%d" % i, seqs.reverse_complement(b)))
        if i % 5 == 0:
            recs.append((">Q%d" % i, seqs.reverse_complement(b[5:-3]) if len(b) > 240 else b))
        if i % 7 == 0:
            recs.append((">M%d" % i, b[:len(b) // 2] + "A" + b[len(b) // 2 + 1:]))
        if i % 11 == 0:
            recs.append((">T%d again" % i, b[3:]))                       # duplicate name -> dict overwrite
    lines = [x for h, s_ in recs for x in (h + "\n", s_ + "\n")]
    for ds in (True, False):
        a = post.find_reps_native(lines, ds)
        b = post.find_reps(lines, ds)
        c = opost.find_reps(lines, ds)
        assert a == b == c
    # enough records for the threaded scan of the native code (the occurrences must come out in record order)
    big = []
    for rep in range(60):
        for h, s_ in recs:
            big.append((h.split()[0] + "_%d" % rep + h[len(h.split()[0]):], s_[rep % 5:] if len(s_) > 300 else s_))
    lines = [x for h, s_ in big for x in (h + "\n", s_ + "\n")]
    assert len(big) > 4096
    for ds in (True, False):
        assert post.find_reps_native(lines, ds) == post.find_reps(lines, ds)
    full = post.finalize(lines, True)
    assert full == opost.finalize(lines, True)


@pytest.mark.parametrize("name", CASES[:4])
def test_contig_graph_fed_in_pieces_equals_one_call(name):
    """shn_cgraph (the contig stage fed block by block by the pipelined extension) == shn_contig_graph on all candidates."""
    from shannon_amd import build, extension_correction as ec
    build.build(verbose=False)
    g = load_case(name)
    inp = load_inputs(name)
    K = g["K"]
    dbl = read_files(name, inp)
    tab = count.count_k1mers_dict([r for f in dbl for r in f], K + 1)
    cands = extension.candidate_contigs([(k, tab[k]) for k in sorted(tab, reverse=True)]) if hasattr(extension, "candidate_contigs") else None
    if cands is None:                                    # any strings in a fixed order will do: accepted contigs + variants of them
        res = extension.run_correction([(k, tab[k]) for k in sorted(tab, reverse=True)])
        rng = np.random.default_rng(7)
        cands = []
        for c in res.contigs:
            cands.append(c)
            if len(c) > 120:
                cands += [c[10:-10], c[: len(c) // 2] + "".join("ACGT"[i] for i in rng.integers(0, 4, 40)) + c[len(c) // 2:]]
    acc, coff, cnb, cw = ec.contig_stage(cands, K + 1)
    cg = ec.ContigGraph(K + 1)
    cuts = [0, len(cands) // 5, len(cands) // 5, len(cands) // 2, len(cands)]
    accs = [cg.add(cands[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    got = np.concatenate(accs) if accs else np.zeros(0, np.int32)
    assert np.array_equal(got, acc)
    assert cg.connections() == (coff, cnb, cw)
    cg.close()
