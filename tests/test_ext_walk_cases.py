"""CPU: the sequential walk reference of tests/ext_walk_cases.py against the oracle's seed loop (oracle/extension.py:python_walks), and
every planted case against what it is there for.  Nothing here loads the library."""
from collections import Counter
import numpy as np
import pytest
import ext_setup_cases as ec
import ext_walk_cases as wc

NONE32 = ec.NONE32


def _steps(w):
    live = wc.live_of(w)
    return live, w.n_right[live].astype(np.int64) + w.n_left[live]


@pytest.mark.parametrize("name", ["chain_canon", "loops_canon", "loops_fwd", "dense_6_canon", "dense_6_canon_one_count", "lengths_20_canon", "heavy"])
def test_reference_equals_the_oracle(name):
    """the same contigs, total weights and k1-mer counts, in the same order.  The oracle adds a palindrome's two strands up without a
    limit; the product's weights are 32-bit and clamp at 2^32 - 1 (ext_setup_cases.reference), so `heavy`, whose palindrome would
    weigh 2^33 - 2, is fed to the oracle with every weight clamped: the one place where the tables differ by definition"""
    from oracle import extension
    t = wc.table(name)
    ref, w = wc.expected(name, 3)
    items = [(s, min(c, NONE32)) for s, c in ec.dumped_items(t)]
    if name != wc.HEAVY:
        assert items == ec.dumped_items(t)
    kmers, k1 = extension.load_kmers(items)
    assert k1 == t.k
    want = list(extension.python_walks(kmers, k1, 3))
    live = wc.live_of(w)
    got = [(w.contigs[r], float(int(w.tot_weight[r])), int(w.n_right[r]) + int(w.n_left[r]) + 1) for r in live.tolist()]
    assert len(got) == len(want) and len(want) >= 4
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, "live walk %d (rank %d): %r, the oracle has %r" % (i, live[i], g, x)


@pytest.mark.parametrize("name,min_weight", wc.CASES)
def test_every_claim_lies_on_one_live_walk(name, min_weight):
    """every claimed oriented id on exactly one live walk's path, and on its owner's; void walks as the product writes them; the
    contigs spell their paths"""
    t = wc.table(name)
    ref, w = wc.expected(name, min_weight)
    ns = len(ref.order)
    assert len(w.n_right) == len(w.n_left) == len(w.tot_weight) == len(w.paths) == len(w.contigs) == len(w.depth) == ns
    seen = Counter(o for p in w.paths for o in p)
    assert not seen or max(seen.values()) == 1
    claimed = np.flatnonzero(w.owner >= 0)
    assert sorted(seen) == claimed.tolist() and ref.alive[claimed].all()
    void = w.n_right == NONE32
    assert (w.n_left[void] == 0).all() and (w.tot_weight[void] == 0).all()
    w2 = np.repeat(ref.weight, 2).astype(np.uint64)
    for r in range(ns):
        p = w.paths[r]
        if void[r]:
            assert p == [] and w.contigs[r] is None and w.owner[ref.order[r]] < r and w.depth[r] >= 1
            continue
        assert p[0] == ref.order[r] and (w.owner[p] == r).all() and len(p) == 1 + int(w.n_right[r]) + int(w.n_left[r])
        assert int(w2[p].sum()) == int(w.tot_weight[r])
        assert len(w.contigs[r]) == t.k + len(p) - 1
    # the contigs' windows are the paths' strings (checked on the longest walk of each case)
    if (~void).any():
        live, steps = _steps(w)
        r = int(live[np.argmax(steps)])
        nl = int(w.n_left[r])
        keys = wc.windows(w.contigs[r], t.k)
        p = w.paths[r]
        order = list(reversed(p[1 + int(w.n_right[r]):])) + [p[0]] + p[1:1 + int(w.n_right[r])]
        assert keys == ref.strings[order].tolist() and keys[nl] == int(ref.strings[ref.order[r]])


@pytest.mark.parametrize("name", wc.LENGTHS)
def test_lengths_give_exactly_the_planted_walks(name):
    t = wc.table(name)
    ref, w = wc.expected(name)
    assert len(t.keys) == wc.LENGTH_KMERS == 15278 and len(wc.LENGTH_PAIRS) == 105
    live = wc.live_of(w)
    got = list(zip(w.n_right[live].tolist(), w.n_left[live].tolist()))
    if not t.canonical:
        assert len(ref.order) == 15278 and got == list(wc.LENGTH_PAIRS) and live.tolist() == list(range(105))
    else:
        assert len(ref.order) == 2 * 15278 and live.tolist() == list(range(210))
        for i, ab in enumerate(wc.LENGTH_PAIRS):                      # a walk and its mirror, in the order of their seed strings
            assert sorted(got[2 * i:2 * i + 2]) == sorted([ab, ab[::-1]])
    assert Counter(got) == Counter(wc.LENGTH_PAIRS) + (Counter((b, a) for a, b in wc.LENGTH_PAIRS) if t.canonical else Counter())
    assert w.tot_weight[live].tolist() == [100000 - i // (2 if t.canonical else 1) + 5 * (a + b) for i, (a, b) in enumerate(got)]
    for n in (15, 16, 17, 63, 64, 65):                                # the hand-over and the memo chunk; to the left: 15, 16, 17, 64
        assert any(a == n for a, b in got) and (any(b == n for a, b in got) or (not t.canonical and n in (63, 65)))
    assert max(w.depth) == 1 and not (ref.flags & 3).any()


@pytest.mark.parametrize("name", wc.CHAINS)
def test_chain_is_a_chain(name):
    t = wc.table(name)
    tips, starts, detours = wc.chain_parts(name)
    assert len(t.keys) == 2000 and t.k == 26
    for mw, depth, n_seeds in ((3, 40, 2000), (100, 39, 40)):
        ref, w = wc.expected(name, mw)
        strands = 2 if t.canonical else 1
        assert len(ref.order) == n_seeds * strands and max(w.depth) == depth >= 39
        live = wc.live_of(w)
        assert live.tolist() == list(range(40 * strands))
        assert (w.n_right[live].astype(int) + w.n_left[live] == 49).all()
        if not t.canonical:
            assert (w.n_right[live] == 49).all()
            assert [w.contigs[r] for r in live.tolist()] == [starts[i] + detours[i][25:] for i in range(40)]
            assert [w.depth[r] for r in live.tolist()] == list(range(40))
    # ... and only because of the walk before: without walk i - 1 (its seed below min_weight), walk i takes its tip
    i = 7
    d = dict(zip(t.keys.tolist(), t.counts.tolist()))
    first = wc.windows(starts[i - 1][:26], 26)[0]
    d[wc._canon(first, 26) if t.canonical else first] = 1
    ref = ec.reference(np.array(list(d), np.uint64), np.array(list(d.values()), np.uint32), 26, t.canonical, 100)
    w = wc.walk_reference(ref, 26)
    assert starts[i] + tips[i][-1] in w.contigs and starts[i + 1] + tips[i + 1][-1] in w.contigs and max(w.depth) == i - 2


def test_loops_close_on_themselves():
    for name in wc.LOOPS:
        t = wc.table(name)
        parts = wc.loop_parts(name)
        ref, w = wc.expected(name)
        live, steps = _steps(w)
        pal = np.flatnonzero(ref.flags & 1)
        if not t.canonical:
            assert len(t.keys) == 300 + 299 + 275 + 22 and len(pal) == 0
            assert list(zip(w.n_right[live].tolist(), w.n_left[live].tolist()))[:3] == [(299, 0), (298, 0), (274, 0)]
            assert [w.contigs[r] for r in live[:3].tolist()] == [parts.circle, parts.rho, parts.hairpin]
        else:
            assert len(t.keys) == 300 + 299 + 138 + 22 and len(pal) == 1      # the hairpin's strands share their k1-mers
            assert sorted(steps.tolist(), reverse=True)[:5] == [299, 299, 298, 298, 274]
            hair = int(live[steps == 274][0])
            assert 2 * int(pal[0]) in w.paths[hair] and w.contigs[hair] == parts.hairpin
            assert ec.str_of(t.keys[pal[0]], 26) == parts.hairpin[137:163]
        # the circle walk stops at its own seed, the rho walk at its own claim in the middle of its path
        circle = int(live[0])
        assert ref.order[circle] in ref.rows[w.paths[circle][-1]].tolist()
        rho = int(live[steps == 298][0])
        assert any(o in w.paths[rho][1:-1] for o in ref.rows[w.paths[rho][-1]].tolist() if o >= 0)
        # the 2-cycle: some walk holds both of its k1-mers, one after the other
        ac, ca = ("AC" * 26)[:26], ("CA" * 26)[:26]
        assert any(c and (ac + "A" in c or ca + "C" in c) for c in w.contigs)


# the longest walk of every dense case.  Low-complexity k1-mers are dropped (the most frequent base on k1 - 2 places or more): of the
# 4,096 6-mers 3,480 are left, so no walk at k1 = 6 can come near 3,000 steps
DENSE_LONGEST = {"dense_6_fwd": 2273, "dense_6_canon": 1471, "dense_7_fwd": 9374, "dense_7_canon": 10720, "dense_6_canon_one_count": 851}


@pytest.mark.parametrize("name", wc.DENSE)
def test_dense_tables_hold_every_k1mer(name):
    t = wc.table(name)
    ref, w = wc.expected(name)
    k = t.k
    both = set(t.keys.tolist()) | set(ec.revcomp(t.keys, k).tolist())
    assert len(both) == 4 ** k and len(t.keys) == (4 ** k if not t.canonical else (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2)
    assert 2080 <= len(t.keys) <= 16384
    counts = set(t.counts.tolist())
    assert counts == ({6} if name.endswith("one_count") else {1, 2, 3, 4, 5, 6})
    live, steps = _steps(w)
    assert int(steps.max()) == DENSE_LONGEST[name]
    if k == 7:
        assert steps.max() >= 3000
    assert int((w.n_right == NONE32).sum()) >= 1000
    # four candidates at most steps of the longest walk's graph, and ties among them
    full = (ref.rows[ref.alive][:, :4] >= 0).sum(axis=1)
    assert (full >= 3).mean() > 0.5
    assert max(w.depth) >= 5
    if name.endswith("one_count"):
        assert set(ref.weight[(ref.flags & 2) == 0].tolist()) == {6, 12}


def test_heavy_totals_pass_two_to_the_35():
    t = wc.table(wc.HEAVY)
    ref, w = wc.expected(wc.HEAVY)
    assert len(t.keys) == 36 and (t.counts == NONE32).all() and t.canonical
    pal = np.flatnonzero(ref.flags & 1)
    assert len(pal) == 1 and ref.weight[pal[0]] == NONE32             # clamped, not doubled
    assert ec.str_of(t.keys[pal[0]], 26) == wc.heavy_parts()[0][5:31]
    live, steps = _steps(w)
    assert int(w.tot_weight.max()) > 1 << 35 and int(w.tot_weight.max()) == 12 * NONE32
    on = [r for r in live.tolist() if 2 * int(pal[0]) in w.paths[r]]
    assert len(on) == 1 and int(w.tot_weight[on[0]]) > 1 << 32
    assert int(w.tot_weight.sum()) == NONE32 * len(np.flatnonzero(w.owner >= 0))


def test_seed_tables_have_exactly_n_seeds():
    for n in wc.SEED_COUNTS:
        t = wc.table("seeds_%d" % n)
        ref, w = wc.expected("seeds_%d" % n)
        assert len(ref.order) == n and not t.canonical and len(t.keys) == n + 3 * ((n + 2) // 3)
        assert (w.n_right != NONE32).all() and (w.n_left == 0).all()
        assert Counter(w.n_right.tolist()) == Counter({3: (n + 2) // 3, 0: n - (n + 2) // 3}) - Counter({0: 0})
        assert max(w.depth) == 0
    for name, n_keys in (("empty", 0), ("no_seed", 50)):
        t = wc.table(name)
        ref, w = wc.expected(name)
        assert len(t.keys) == n_keys and len(ref.order) == 0 and len(w.n_right) == 0 and w.paths == []
