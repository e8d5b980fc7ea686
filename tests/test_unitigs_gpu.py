"""GPU: the batched unitig contraction (shn_unitigs_build, csrc/graph_gpu.hip) against the sequential code it stands for --
oracle.mbgraph load_k1mers + condense_all -- on inputs chosen for it (tests/unitig_cases.py; tests/test_unitig_cases.py shows on
the CPU that they are what they claim to be).  Everything is equality: K-mer counts, the final nodes in creation order, every
node's out- and in-list in list order, the edges in creation order, the cycle flag against a predicate of its own."""
import numpy as np
import pytest
import unitig_cases as uc

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def expected(contigs, K):
    key = (K, tuple(contigs))
    if key not in _EXPECTED:
        _EXPECTED[key] = uc.expected(contigs, K)
    return _EXPECTED[key]


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def build(ctx, parts, K, flat):
    from shannon_amd import mbgraph_native
    return mbgraph_native.Unitigs(ctx, parts, K, flat_text=uc.flat_text_of(parts) if flat else None)


def check_batch(ctx, batch, K, flat):
    """every partition of the batch against the oracle; returns the views.  A partition flagged cyclic is not counted as compared,
    and exactly the designed ones are flagged."""
    U = build(ctx, [c for _n, c, _d in batch], K, flat)
    views, compared = [], 0
    for p, (name, contigs, designed) in enumerate(batch):
        exp = expected(contigs, K)
        assert exp["cyclic"] == designed, name
        v = U.partition(p)
        assert U.n_kmers(p) == v["n_kmers"]
        compared += uc.compare(v, exp, K, "%s (partition %d, K=%d)" % (name, p, K))
        views.append(v)
    assert compared == sum(1 for _n, _c, d in batch if not d)
    U.close()
    return views


def same_view(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("flat", [False, True], ids=["strings", "flat_text"])
@pytest.mark.parametrize("K", uc.KS)
def test_every_shape_in_one_batch_equals_the_oracle(ctx, K, flat):
    """the named shapes and the family cases of one K in one call: partitions without contigs first, in the middle and last"""
    batch = uc.full_batch(K)
    assert not batch[0][1] and not batch[-1][1]
    check_batch(ctx, batch, K, flat)


@pytest.mark.parametrize("K", [6, 25, 31])
def test_a_partition_alone_equals_itself_inside_a_batch(ctx, K):
    """batch independence, and the same K-mers in several partitions (per-partition table regions): the family case three times
    between other partitions, once more alone"""
    shapes = {n: c for n, c, _d in uc.full_batch(K)}
    fam = shapes["family"]
    batch = [("family", fam, False), ("linear_long_pieces", shapes["linear_long_pieces"], False), ("family", fam, False),
             ("pure_cycle", shapes["pure_cycle"], True), ("empty_middle", [], False), ("family_repeated_rows", shapes["family_repeated_rows"], False),
             ("family", list(fam), False), ("fork_and_join", shapes["fork_and_join"], False)]
    inside = check_batch(ctx, batch, K, False)
    for p, (name, contigs, designed) in enumerate(batch):
        alone = check_batch(ctx, [(name, contigs, designed)], K, p % 2 == 1)[0]
        assert same_view(alone, inside[p]), (name, p)
    assert same_view(inside[0], inside[2]) and same_view(inside[0], inside[6])


@pytest.mark.parametrize("flat", [False, True], ids=["strings", "flat_text"])
def test_many_final_nodes_in_many_partitions(ctx, flat):
    """>= 4 partitions and >= 4,096 final nodes: the host assembly of the result runs on threads"""
    check_batch(ctx, uc.many_nodes_batch(), 25, flat)


@pytest.mark.parametrize("flat", [False, True], ids=["strings", "flat_text"])
def test_large_batch(ctx, flat):
    """0.3 M K-mers in one call: several blocks per kernel, contended atomics in the table and the degree counts"""
    check_batch(ctx, uc.large_batch(), 25, flat)


# ---------------------------------------------------------------- into the graph stage
def graph_cases(K):
    cases = [(n, c, uc.sample_reads(s, 60, 300, 7), d) for n, c, s, d in uc.named_shapes(K)]
    for seed, kw in ((1, {}), (2, {"distinct": False})):
        c, s = uc.family_case(K, seed, **kw)
        cases.append(("family_%d" % seed, c, uc.sample_reads(s, 60, 300, 7), False))
    return cases


@pytest.mark.parametrize("check", [False, True], ids=["plain", "SHN_GRAPH_CHECK"])
@pytest.mark.parametrize("K", [12, 25, 31])
def test_graph_stage_continues_from_the_unitigs(ctx, monkeypatch, K, check):
    """shn_mbgraph_run_unitigs on every named shape and two family cases == the same call on the host path (load_k1mers +
    condense_all), ids and order included, and canonically == the oracle's run_partition.  Once more under SHN_GRAPH_CHECK=1: the
    built-in order-sensitive comparison of the two loaders must stay silent.  A partition with a pure cycle is flagged and built
    from its rows; without rows the call is refused."""
    from shannon_amd import mbgraph_native as mn, _lib
    from oracle import mbgraph as omb
    if check:
        monkeypatch.setenv("SHN_GRAPH_CHECK", "1")
    else:
        monkeypatch.delenv("SHN_GRAPH_CHECK", raising=False)
    cases = graph_cases(K)
    U = build(ctx, [c for _n, c, _r, _d in cases], K, False)
    flagged = 0
    for p, (name, contigs, reads, designed) in enumerate(cases):
        rows = uc.rows_of(contigs, K)
        rb = np.frombuffer("".join(rows).encode(), dtype=np.uint8) if rows else np.zeros(1, np.uint8)
        b1, o1 = mn._pack_reads(reads)
        host = mn.run_partition_arrays(rb, len(rows), K, b1, o1, ctx=ctx)
        got = mn.run_partition_arrays(rb, len(rows), K, b1, o1, ctx=ctx, unitigs=U, part=p)
        assert got == host, (name, K)
        _g, singles, comps = omb.run_partition([(r, 1) for r in rows], [reads], K)
        assert omb.canonical(got[0], got[1]) == omb.canonical(singles, comps), (name, K)
        view = U.partition(p)
        assert view["cyclic"] == designed, name
        if designed:
            flagged += 1
            with pytest.raises(_lib.ShannonError, match=r"cyclic partition needs the k1-mer rows \(code -1\)"):
                mn.run_partition_arrays(None, 0, K, b1, o1, ctx=ctx, unitigs=U, part=p)
        elif not check:
            assert mn.run_partition_arrays(None, 0, K, b1, o1, ctx=ctx, unitigs=U, part=p) == host, (name, K)
    assert flagged == 2
    U.close()


# ---------------------------------------------------------------- error returns
def test_bad_arguments_are_error_returns(ctx):
    """argument checks of the host side (in the non-ACGT case the insert kernel only counts the bad windows and the host returns
    the error after the scan); the context stays usable"""
    from shannon_amd import mbgraph_native as mn, _lib
    K = 25
    good = uc.family_case(K, 1)[0][:20]
    for bad in (good[3][:10] + "N" + good[3][11:], good[3][:10] + good[3][10].lower() + good[3][11:]):
        assert len(bad) >= K + 1
        with pytest.raises(_lib.ShannonError, match=r"outside ACGT \(code -1\)"):
            mn.Unitigs(ctx, [good[:3], good[4:6] + [bad], good[6:]], K)
    for k in (1, 32):
        with pytest.raises(_lib.ShannonError, match=r"bad argument \(code -1\)"):
            mn.Unitigs(ctx, [good], k)
    text, off, part_of, n = uc.flat_text_of([good[:5], good[5:9], good[9:]])
    for po in (part_of[::-1].copy(), np.where(part_of == 2, 3, part_of).astype(np.uint32)):       # descending; beyond n_parts
        with pytest.raises(_lib.ShannonError, match=r"part_of must be ascending and < n_parts \(code -1\)"):
            mn.Unitigs(ctx, [good[:5], good[5:9], good[9:]], K, flat_text=(text, off, po, n))
    # zero contigs: an empty, usable handle
    U = mn.Unitigs(ctx, [[], []], K)
    for p in (0, 1):
        v = U.partition(p)
        assert v["n_kmers"] == 0 == U.n_kmers(p) and not v["cyclic"] and v["bases"] == [] and len(v["e_src"]) == 0
        b1, o1 = mn._pack_reads([])
        assert mn.run_partition_arrays(None, 0, K, b1, o1, ctx=ctx, unitigs=U, part=p)[:2] == ([], [])
    with pytest.raises(_lib.ShannonError, match=r"\(code -1\)"):
        U.partition(2)
    U.close()
    # and the context goes on working
    check_batch(ctx, [("family_head", good, False)], K, False)
