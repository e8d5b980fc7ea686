"""CPU, oracle only: the inputs of tests/test_unitigs_gpu.py are what they claim to be, so that a green GPU test means something.
Nothing here touches the product; tests/unitig_cases.py holds the generators and the expectation."""
import pytest
import unitig_cases as uc

BIG_K = [K for K in uc.KS if K >= 12]


@pytest.mark.parametrize("K", BIG_K)
def test_family_cases_depart_from_row_order(K):
    """At least 10 final nodes whose out-list is not in the row order of their junction k1-mers, and 10 such in-lists: a kernel
    that ignored the merge times would pass otherwise.  (A seed that falls below the floor is to be changed, not the floor.)"""
    contigs, _ = uc.family_case(K, 1)
    exp = uc.expected(contigs, K)
    multi_out, diff_out, multi_in, diff_in = uc.list_order_stats(exp, K)
    print("K=%d: %d of %d out-lists and %d of %d in-lists not in row order" % (K, diff_out, multi_out, diff_in, multi_in))
    assert diff_out >= 10 and diff_in >= 10, (diff_out, diff_in)
    assert len(set(exp["rows"])) == len(exp["rows"])                  # the distinct-k1-mer step did its work
    # pieces overlap by K bases: K-mer ids are not ascending along the chains -- some merged node's K-mers were first seen out of order
    first = {}
    for r in exp["rows"]:
        first.setdefault(r[:-1], len(first))
        first.setdefault(r[1:], len(first))
    unordered = 0
    for b, m in zip(exp["bases"], exp["merged"]):
        ids = [first[b[i:i + K]] for i in range(len(b) - K + 1)]
        unordered += m and ids != sorted(ids)
    assert unordered >= 10, unordered


@pytest.mark.parametrize("K", BIG_K)
def test_family_cases_have_merged_nodes_and_x_nodes(K):
    for seed, kw in ((1, {}), (2, {"distinct": False})):
        exp = uc.expected(uc.family_case(K, seed, **kw)[0], K)
        assert sum(exp["merged"]) >= 10
        assert sum(1 for o, i in zip(exp["out_lists"], exp["in_lists"]) if len(o) >= 2 and len(i) >= 2) >= 10
    assert len(set(exp["rows"])) < len(exp["rows"])                   # without the distinct step: repeated rows = parallel edges
    par = sum(len(o) - len(set(o)) for o in exp["out_lists"])
    assert par >= 100, par


@pytest.mark.parametrize("K", [K for K in uc.KS if K <= 4])
def test_small_k_cases_are_dense(K):
    """all 4^K K-mers occur and nothing condenses: dense edge lists, every table region full of neighbours"""
    exp = uc.expected(uc.family_case(K, 2, distinct=False)[0], K)
    assert exp["n_kmers"] == 4 ** K == len(exp["bases"]) and not any(exp["merged"])
    assert min(len(o) for o in exp["out_lists"]) >= 4


@pytest.mark.parametrize("K", uc.KS)
def test_cycle_predicate_holds_exactly_where_designed(K):
    for name, contigs, designed in uc.full_batch(K):
        assert uc.cycle_predicate(uc.rows_of(contigs, K), K) == designed, (K, name)
    for batch in ((uc.many_nodes_batch(), uc.large_batch()) if K == 25 else ()):
        for name, contigs, designed in batch:
            assert not designed and not uc.cycle_predicate(uc.rows_of(contigs, 25), 25), name


@pytest.mark.parametrize("K", uc.KS)
def test_named_shapes_are_the_shapes(K):
    sh = {n: uc.expected(c, K) for n, c, _s, _d in uc.named_shapes(K)}
    names = [n for n, _c, _s, _d in uc.named_shapes(K)]
    assert names[0] == "empty_first" and names[-1] == "empty_last" and "empty_middle" in names[1:-1]
    for n in ("empty_first", "empty_middle", "empty_last", "all_short"):
        assert sh[n]["n_kmers"] == 0 and not sh[n]["bases"] and not sh[n]["rows"]
    assert sh["k_plus_one"]["n_kmers"] == 2 and len(sh["k_plus_one"]["rows"]) == 1
    assert len(sh["k_plus_one_k_and_fewer"]["rows"]) == 2
    for n in ("poly_a", "poly_t"):                                    # one K-mer, 40 parallel self-loops
        assert sh[n]["n_kmers"] == 1 and sh[n]["out_lists"] == [[0] * 40]
    assert sh["linear_long"]["rows"] != sh["linear_long_pieces"]["rows"] and sorted(sh["linear_long"]["rows"]) == sorted(sh["linear_long_pieces"]["rows"])
    assert any(s == d for s, d in sh["homopolymer_inside"]["edge_seq"])
    tw = sh["twice_around"]
    assert len(tw["bases"]) == tw["n_kmers"] and all(len(o) == 2 for o in tw["out_lists"])   # every row twice: nothing condenses
    if K >= 12:
        assert sh["linear_long"]["n_kmers"] >= 5000 and len(sh["linear_long"]["bases"]) == 1
        assert len(sh["linear_long_pieces"]["bases"]) == 1
        # a cycle with a tail leading in is not pure: the oracle yields a merged node with a self-loop
        cw = sh["cycle_with_tail"]
        assert not cw["cyclic"] and len(cw["bases"]) == 2 and any(s == d and cw["merged"][s] for s, d in cw["edge_seq"])
        fj = sh["fork_and_join"]
        assert any(len(o) >= 2 for o in fj["out_lists"]) and any(len(i) >= 2 for i in fj["in_lists"])
    # the pure cycles: the oracle itself has a defined answer (one node with a self-loop); a second one stands beside other nodes
    assert sh["pure_cycle"]["cyclic"] and len(sh["pure_cycle"]["bases"]) == 1 and sh["pure_cycle"]["edge_seq"] == [(0, 0)]
    assert sh["pure_cycle_beside_others"]["cyclic"] and len(sh["pure_cycle_beside_others"]["bases"]) >= 2


def test_batches_are_the_sizes_they_claim():
    many = uc.many_nodes_batch()
    assert len(many) >= 4 and sum(len(uc.expected(c, 25)["bases"]) for _n, c, _d in many) >= 4096      # the threaded host assembly
    assert any(len(uc.expected(c, 25)["edge_seq"]) >= 100 for _n, c, _d in many)
    n = sum(uc.expected(c, 25)["n_kmers"] for _n, c, _d in uc.large_batch())
    assert 300000 <= n <= 1000000, n


def test_compare_rejects_wrong_orders():
    """the comparison itself: a view made from the expectation passes; swapping two list ranks, two edge ids or two nodes fails"""
    import numpy as np
    K = 25
    exp = uc.expected(uc.family_case(K, 1)[0], K)
    n = len(exp["bases"])

    def view_of(e):
        orank, irank = {}, {}
        for i in range(n):
            for r, j in enumerate(e["out_lists"][i]):
                orank.setdefault((i, j), []).append(r)
            for r, j in enumerate(e["in_lists"][i]):
                irank.setdefault((j, i), []).append(r)
        src = [s for s, _ in e["edge_seq"]]
        dst = [d for _, d in e["edge_seq"]]
        ro = [orank[sd].pop(0) for sd in e["edge_seq"]]
        ri = [irank[sd].pop(0) for sd in e["edge_seq"]]
        u32 = lambda x: np.array(x, dtype=np.uint32)
        cnt = e["count"]
        tail = [p // (K - 1) - (c - 1) for p, c in zip(e["prevalence"], cnt)]
        return {"n_kmers": e["n_kmers"], "cyclic": e["cyclic"], "bases": list(e["bases"]), "n_len": u32(cnt), "n_tail_out": u32(tail),
                "e_src": u32(src), "e_dst": u32(dst), "e_out_rank": u32(ro), "e_in_rank": u32(ri)}

    assert uc.compare(view_of(exp), exp, K)
    v = view_of(exp)
    i = next(i for i in range(n) if len(set(exp["out_lists"][i])) >= 2)
    es = [x for x in range(len(v["e_src"])) if v["e_src"][x] == i][:2]
    v["e_out_rank"][es[0]], v["e_out_rank"][es[1]] = v["e_out_rank"][es[1]], v["e_out_rank"][es[0]]
    with pytest.raises(AssertionError, match="out-list"):
        uc.compare(v, exp, K)
    v = view_of(exp)
    x = next(x for x in range(len(v["e_src"]) - 1) if exp["edge_seq"][x] != exp["edge_seq"][x + 1])
    for k in ("e_src", "e_dst", "e_out_rank", "e_in_rank"):
        v[k][x], v[k][x + 1] = v[k][x + 1], v[k][x]
    with pytest.raises(AssertionError, match="edge order"):
        uc.compare(v, exp, K)
    v = view_of(exp)
    v["bases"][0], v["bases"][1] = v["bases"][1], v["bases"][0]
    with pytest.raises(AssertionError, match="bases of node"):
        uc.compare(v, exp, K)
    v = view_of(exp)
    v["e_out_rank"][es[0]] = v["e_out_rank"][es[1]]
    with pytest.raises(AssertionError, match="permutation"):
        uc.compare(v, exp, K)
