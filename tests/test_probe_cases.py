"""CPU: the brute force of tests/probe_cases.py against the oracle's k1mers2component on the two golden cases with several
partitions, against a hand-written example, and every case builder against the precondition it states."""
import pytest
from golden_util import MANIFEST, load_case, part_vectors
import probe_cases as pc

MULTI_PARTITION_CASES = ["syn_part_s33", "syn_pe_L250_K20_part1"]


@pytest.mark.parametrize("name", MULTI_PARTITION_CASES)
def test_brute_force_equals_the_oracle_on_the_golden_partitions(name):
    from oracle import partition
    g = load_case(name)
    K, psize = g["K"], MANIFEST[name].get("partition_size", 500)
    big = [b["contigs"] for b in g["big_components"]]
    pv = [part_vectors(len(cl), psize) for cl in big]
    nc, k2c = partition.build_partitions(big, [p[0] for p in pv], [p[1] for p in pv], g["remaining"], {}, K)
    assert list(nc) == list(g["partitions"]) and len(nc) >= 16
    number = {comp: i for i, comp in enumerate(nc)}
    want = {km: frozenset(number[c] for c in e[0]) for km, e in k2c.items()}
    got = pc.expected_sets([nc[comp] for comp in nc], K + 1)
    assert got == want
    assert sum(len(s) == 2 for s in got.values()) > 1000         # (gpmetis run + r2 run: these cases are about pairs)


def test_brute_force_on_a_hand_written_example():
    # k1 = 3.     partition 0            partition 1     partition 2 (a contig too short, an empty one)     partition 3
    parts = [["ACGTA", "CGT"], ["GTAC", "TTT"], ["AC", "", "TACG"], ["TTTT", "ACG"]]
    # windows: ACG CGT GTA | CGT ; GTA TAC | TTT ; TAC ACG ; TTT TTT | ACG      -- a dozen
    want = {"ACG": {0, 2, 3}, "CGT": {0}, "GTA": {0, 1}, "TAC": {1, 2}, "TTT": {1, 3}}
    assert sum(max(len(c) - 2, 0) for p in parts for c in p) == 12
    assert pc.expected_sets(parts, 3) == {km: frozenset(s) for km, s in want.items()}
    runs = pc.window_runs(parts, 3)
    assert runs["ACG"] == (0, 2, 3) and runs["CGT"] == (0, 0) and runs["TTT"] == (1, 3, 3)
    assert pc.expected_sets(parts, 5) == {"ACGTA": frozenset([0])} and pc.expected_sets(parts, 6) == {}
    assert [pc.key_of(km) for km in ("AAA", "AAC", "TTT", "ACG")] == [0, 1, 63, 6]
    text, off, part_of, n = pc.flatten(parts)
    assert n == 9 and bytes(text) == b"ACGTACGTGTACTTTACTACGTTTTACG" and part_of.tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3]
    assert off.tolist() == [0, 5, 8, 12, 15, 17, 17, 21, 25, 28]


CASES = [(pc.single_repeat_in_contig, ()), (pc.single_shared_in_partition, ()), (pc.multi, ()), (pc.relaunch, ()), (pc.width_2, ()),
         (pc.width_32_poly, ()), (pc.degenerate_lengths, ()), (pc.no_window, ()), (pc.all_empty, ()), (pc.no_contig, ()),
         (pc.empty_ends, ())] + [(pc.pairs, (n,)) for n in pc.PAIR_N_PARTS] + [(pc.pairs, (257, 32)), (pc.multi, (32,))] + \
        [(pc.mixed, (k1,)) for k1 in (21, 26, 32)]


@pytest.mark.parametrize("builder,args", CASES, ids=lambda v: v.__name__ if callable(v) else "-".join(map(str, v)))
def test_every_case_meets_its_own_precondition(builder, args):
    parts, k1, need = builder(*args)
    sets, runs = pc.require(parts, k1, need)
    assert set(sets) == set(runs) and all(frozenset(runs[km]) == sets[km] and list(runs[km]) == sorted(runs[km]) for km in sets)
    text, off, part_of, n = pc.flatten(parts)
    assert n == sum(len(p) for p in parts) and int(off[-1]) == sum(len(c) for p in parts for c in p)
    assert all(part_of[i] <= part_of[i + 1] for i in range(n - 1)) and (n == 0 or int(part_of[n - 1]) < len(parts))
