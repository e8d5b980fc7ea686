"""CPU: the brute-force reference of the extension set-up (tests/ext_setup_cases.py) against the oracle's load_kmers and its heaviest-first
sort, and every case against what it is there for.  Nothing here loads the library."""
import numpy as np
import pytest
import ext_setup_cases as ec
from ext_setup_cases import U64


def _strings_of(ref, k):
    return [ec.str_of(s, k) for s in ref.strings.tolist()]


@pytest.mark.parametrize("name,min_weight", [("half_6", 3), ("all_5_fwd", 4), ("size_65", 3), ("edge_20_canon", 3)])
def test_reference_equals_the_oracle(name, min_weight):
    """weights, dropped k1-mers and the seed order of the reference are load_kmers' and the seed loop's own sort; the rows are the
    neighbours the oracle's walk would look up, string by string"""
    from oracle import extension
    t = ec.table(name)
    ref = ec.reference(t.keys, t.counts, t.k, t.canonical, min_weight)
    items = ec.dumped_items(t)
    kmers, k1 = extension.load_kmers(items)
    assert k1 == t.k
    strings = _strings_of(ref, t.k)
    mine = {strings[o]: float(ref.weight[o >> 1]) for o in np.flatnonzero(ref.alive).tolist()}
    assert mine == kmers
    dropped = {s for s, _ in items} - set(kmers)
    assert dropped == {s for s, _ in items if extension.low_complexity(s)}
    assert dropped == {strings[o] for o in range(len(strings)) if ref.flags[o >> 1] & 2 and (o % 2 == 0 or t.canonical)}
    heaviest = sorted(kmers.items(), key=lambda kv: kv[1])          # (python_walks: stable, popped from the end)
    want = []
    while heaviest:
        s, w = heaviest.pop()
        if w < min_weight:
            break
        want.append(s)
    assert len(want) > 10 and [strings[o] for o in ref.order.tolist()] == want
    assert np.array_equal(ref.seed_rank[ref.order], np.arange(len(want)))
    assert (ref.seed_rank == ec.NONE32).sum() == len(strings) - len(want)
    # rows, by strings
    ident = {s: o for o, s in enumerate(strings) if ref.alive[o]}
    for o, s in enumerate(strings):
        if not ref.alive[o]:
            assert (ref.rows[o] == -1).all()
            continue
        for b, c in enumerate("ACGT"):
            assert ref.rows[o][b] == ident.get(s[1:] + c, -1), (s, c)
            assert ref.rows[o][4 + b] == ident.get(c + s[:-1], -1), (c, s)


def test_sizes_cut_by_min_weight():
    for name, mw in ec.SIZE_RUNS:
        t = ec.table(name)
        assert len(t.keys) == int(name[5:]) and t.k == 26 and t.canonical
        if len(t.keys):
            assert t.counts.min() >= 1 and t.counts.max() <= 6
    assert {int(n[5:]) for n, _ in ec.SIZE_RUNS} == set(ec.SIZES)
    t = ec.table("size_5000")
    n_seeds = {mw: len(ec.reference(t.keys, t.counts, 26, True, mw).order) for mw in (1, 3, 7)}
    assert n_seeds[1] == 10000 and 0 < n_seeds[3] < 10000 and n_seeds[7] == 0
    for n in (64, 65, 1023, 1024, 1025):                             # the 64-lane and 1024-thread edges see seeds and non-seeds
        t = ec.table("size_%d" % n)
        r = ec.reference(t.keys, t.counts, 26, True, 3)
        assert 0 < len(r.order) < 2 * n


def test_the_tail_table_makes_the_records_kernel_stride():
    n = len(ec.table("tail").keys)
    assert n == ec.TAIL_N and (8 * n) % 64 != 0
    for b in ec.TAIL_BLOCKS:
        assert 8 * n > 256 * b and b < ec.default_adj_blocks(n)


def test_small_k_tables_hold_every_k1mer():
    want = {"all_4_fwd": (256, 0), "all_5_fwd": (1024, 0), "half_4": (136, 16), "half_5": (512, 0), "half_6": (2080, 64)}
    for name, (n, n_pal) in want.items():
        t = ec.table(name)
        r = ec.reference(t.keys, t.counts, t.k, t.canonical, 3)
        assert len(t.keys) == n and int((r.flags & 1).sum()) == n_pal
        both = set(t.keys.tolist()) | set(ec.revcomp(t.keys, t.k).tolist())
        assert len(both) == 4 ** t.k                                 # with the reverse complements: every string
        n_lc = int((r.flags >> 1).sum())
        assert n_lc == sum(max(ec.str_of(v, t.k).count(c) for c in "ACGT") >= t.k - 2 for v in t.keys.tolist())
        assert 0 < n_lc < n and n_lc * 10 > (8 * n if t.k == 4 else 4 * n if t.k == 5 else 0)      # 232 of all 256 strings, 424 of 1024
        assert len(r.order) > 0
    # the ties of half_6 are heavy: six counts over 2080 keys, palindromes among them
    r = ec.reference(*ec.table("half_6"), 1)
    assert len(set(r.weight.tolist())) <= 12 and (r.flags[r.order >> 1] & 1).sum() > 20


@pytest.mark.parametrize("name", ec.EDGE_K)
def test_edge_tables_hold_their_plants(name):
    t = ec.table(name)
    k = t.k
    r = ec.reference(t.keys, t.counts, k, t.canonical, 3)
    have = set(t.keys.tolist())
    for what, group in ec.edge_plants(k, t.canonical).items():
        stored = ec.canonical_of(np.array(group, dtype=np.uint64), k) if t.canonical else np.array(group, dtype=np.uint64)
        assert set(stored.tolist()) <= have, what
        mx = ec.max_base_count(stored, k)
        if what.startswith("k-3"):
            assert (mx == k - 3).all() and not (r.flags[np.isin(t.keys, stored)] & 2).any()
        if what.startswith("k-2"):
            assert (mx == k - 2).all() and (r.flags[np.isin(t.keys, stored)] & 2).all()
    assert 0 in have and (t.canonical or ec.mask_of(k) in have)
    if k % 2 == 0:
        assert int((r.flags & 1).sum()) == (10 if t.canonical else 0)
    assert 2900 < len(t.keys) < 6000
    full_r, full_l = (r.rows[:, :4] >= 0).all(axis=1), (r.rows[:, 4:] >= 0).all(axis=1)
    assert full_r.sum() >= 250 and full_l.sum() >= 250               # rows with all four entries
    # the 2-cycle: two orientations, each the other's successor
    succ = [set(row[:4][row[:4] >= 0].tolist()) for row in r.rows]
    assert any(o != p and o in succ[p] for o in range(len(succ)) for p in succ[o])
    if k == 31 and t.canonical:                                       # a k1-mer whose successor is its own reverse complement
        assert any((o ^ 1) in succ[o] for o in range(len(succ)))


def test_weight_tables_reach_the_clamp_and_bit_31():
    t = ec.table("weights_extreme")
    r = ec.reference(t.keys, t.counts, 26, True, 3)
    pal = (r.flags & 1) == 1
    assert pal.sum() == 27 and (~pal).sum() == 27
    for c in ec.EXTREME_COUNTS:
        assert (r.weight[pal & (t.counts == c)] == min(2 * c, 0xFFFFFFFF)).all() and (pal & (t.counts == c)).sum() == 3
        assert (r.weight[~pal & (t.counts == c)] == c).all() and (~pal & (t.counts == c)).sum() == 3
    assert {0xFFFFFFFE, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF} <= set(r.weight.tolist())
    assert len(r.order) == 8 * 3 + 2 * 7 * 3                          # no seeds: counts 1 and 2 of the others, 1 of the palindromes
    t = ec.table("weights_one_count")
    r = ec.reference(t.keys, t.counts, 26, True, 3)
    assert len(t.keys) == 2000 and len(set(t.counts.tolist())) == 1 and len(r.order) == 4000
    assert np.array_equal(r.strings[r.order], np.sort(r.strings))     # purely by string
    par = (r.order & 1).astype(np.int64)
    assert np.abs(np.diff(par)).sum() > 1000                          # the orientations interleave
    t = ec.table("weights_bit31")
    r = ec.reference(t.keys, t.counts, 26, True, 3)
    low = t.counts & 0x7FFFFFFF
    for c in np.unique(low).tolist():
        assert set((t.counts[low == c] >> 31).tolist()) == {0, 1}
    w = r.weight[r.order >> 1].astype(np.int64)
    assert (np.diff(w) <= 0).all() and len(r.order) == 1200


def test_the_collision_table_overflows_four_lines_in_a_row():
    c = ec.collision_case()
    t = c.table
    assert len(t.keys) == 4096 and c.lines == 1025 and c.last == 1024 and t.k == 26 and t.canonical
    home = ec.home_lines(t.keys, c.lines)
    assert home.min() >= 0 and home.max() < c.lines
    per_line = np.bincount(home, minlength=c.lines)
    for name, d, cnt in ec.COLLIDE_HOMED:
        assert per_line[getattr(c, name) + d] >= cnt
    keys = t.keys[ec.host_table_order(t.keys)]
    lc = ec.low_complexity(keys, 26)
    count, stored = ec.simulate_dictionary(keys, lc, c.lines)
    assert (count[c.L:c.L + 4] > ec.FD_SLOTS).all()                   # whatever the order: 45 keys start at L, 35 go on, ...
    assert (count > ec.FD_SLOTS).sum() >= 5
    assert ((stored >= 0) & (stored != ec.home_lines(keys, c.lines))).sum() >= 30
    # ... and in any order: M, M2 and M3 keep ten of the keys homed at them and send the others on; the three lines after each hold
    # fewer keys of their own than slots, and what they have left takes the newcomers
    sure = 0
    for first in (c.M, c.M2, c.M3):
        after = per_line[first + 1:first + 4]
        assert (after <= ec.FD_SLOTS).all() and per_line[first - 3:first].max() <= ec.FD_SLOTS
        sure += min(per_line[first] - ec.FD_SLOTS, 3 * ec.FD_SLOTS - after.sum())
    assert sure >= 30
    assert ((stored < 0) & ~lc).sum() >= 1
    assert count[c.lines:].sum() > 0                                  # the spare lines are in use
    # the 45 + 8 + 8 keys around L alone are more than four lines hold: one of them is stored nowhere in ANY order
    assert per_line[c.L:c.L + 4].sum() > 4 * ec.FD_SLOTS
    assert len(c.absent) == 200 and not np.isin(c.absent, t.keys).any()
    ah = ec.home_lines(c.absent, c.lines)
    assert set(ah.tolist()) == {c.L, c.L + 1, c.L + 2, c.L + 3, c.M, c.last}
    assert len(c.low_complexity) >= 4 and np.isin(c.low_complexity, t.keys).all()
    r = ec.reference(t.keys, t.counts, 26, True, 3)
    assert (r.flags & 1).sum() == 3
    # every crowded key is looked up from two rows
    assert len(c.picked) == sum(cnt for _, _, cnt in ec.COLLIDE_HOMED) and np.isin(c.picked, t.keys).all()
    refs = np.bincount(r.rows[r.rows >= 0] >> 1, minlength=len(t.keys))
    assert (refs[np.isin(t.keys, c.picked)] >= 2).all()


def test_the_mirrors_of_the_device_arithmetic():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 64, size=1000, dtype=np.uint64)
    for b in (1, 1025, 17501, (1 << 32) - 1):
        assert ec.mulhi(a, b).tolist() == [(int(x) * b) >> 64 for x in a.tolist()]
    for k in (4, 5, 20, 31, 32):
        x = rng.integers(0, 1 << 64, size=200, dtype=np.uint64) & U64(ec.mask_of(k))
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        want = [ec.key_of("".join(comp[c] for c in reversed(ec.str_of(v, k)))) for v in x.tolist()]
        assert ec.revcomp(x, k).tolist() == want
        assert ec.max_base_count(x, k).tolist() == [max(ec.str_of(v, k).count(c) for c in "ACGT") for v in x.tolist()]


def test_layout1_reads_hold_homopolymers_and_a_palindrome():
    for k1, both in ec.LAYOUT1:
        reads = ec.layout1_reads(k1)
        assert reads.shape == (3000, 100) and reads.max() == 3
        assert (reads[:40] == 3).all() and (reads[40:70] == 0).all()
        if k1 % 2 == 0:
            p = ec.layout1_palindrome(k1)
            key = np.array([ec.key_of(p)], dtype=np.uint64)
            assert len(p) == k1 and ec.revcomp(key, k1)[0] == key[0] and not ec.low_complexity(key, k1)[0]
            text = "".join(ec.ALPHA[c] for c in reads[72])
            assert p in text
