"""CPU: the chained form of --compare ("Chained rows").  The brute force of tests/compare_chain_cases.py on inputs
worked by hand and its table against its enumeration; every case builder against the situation its name claims; psl_lines of a
multi-block row column by column; analyze / false_positive on multi-block lines; the command's --chain."""
import os
import subprocess
import sys
import numpy as np
import pytest
import compare_cases as cc
import compare_chain_cases as c3
from conftest import ROOT

L, M, R = "ACGGTCATTGCAGGATCCAT", "GCAAGTCGGATATTCCGAGT", "ACCGTAGGCTAAT"          # 20, 20 and 13 bases


def blocks_and_chain(q, t):
    b = c3.blocks_of(q, t)
    return b, c3.best_chain(q, t, b)


# ---------------------------------------------------------------------------------------------------------------- the brute force
def test_brute_force_by_hand_gap():
    """L + M against L + TTTT + M: L on diagonal 0; M on diagonal 4, which also takes the T in front of it (L ends in T, and so does
    TTTT): q[19:40).  It follows L with v = 20 - 19 = 1 and enters as q[20:40): two blocks of 20, four target bases between them"""
    q, t = L + M, L + "TTTT" + M
    assert c3.blocks_of(q, t) == [(0, 0, 20, 20, 0), (4, 19, 40, 21, 0)]
    assert c3.overlap((0, 0, 20, 20, 0), (4, 19, 40, 21, 0)) == 1 and c3.overlap((4, 19, 40, 21, 0), (0, 0, 20, 20, 0)) is None
    want = [(0, 0, 0, 40, 0, 0, 40, 0, 0, 0, 1, 4, 2, ((20, 0, 0), (20, 20, 24)))]
    assert c3.brute_chain_rows([("r", q)], [("x", t)], True) == want == c3.brute_chain_rows([("r", q)], [("x", t)], False)
    assert cc.brute_rows([("r", q)], [("x", t)], True) == []                         # unchained: 21 matches are no row
    assert c3.brute_chain_rows([("r", q)], [("x", t)], True, min_matches=41) == []


def test_brute_force_by_hand_trim_on_the_other_strand():
    """L + M + R against the reverse complement of L + M + M + R (73 bases).  On '-': L + M on diagonal 0, q[0:40); M + R on diagonal
    20 with the T in front of it, q[19:53), which loses v = 40 - 19 = 21 positions and enters as q[40:53) -> oriented target
    [60:73), forward [0:13); the first block oriented [0:40), forward [33:73).  Nothing between them in the query, M's second copy
    in the target"""
    q, t = L + M + R, L + M + M + R
    assert c3.blocks_of(q, t) == [(0, 0, 40, 40, 0), (20, 19, 53, 34, 0)]
    assert c3.recount(q, t, (20, 19, 53, 34, 0), 21) == (13, 0)
    want = [(0, 0, 1, 53, 0, 0, 53, 0, 0, 0, 1, 20, 2, ((40, 0, 33), (13, 40, 0)))]
    assert c3.brute_chain_rows([("r", q)], [("x", cc.rc(t))], False) == want
    assert c3.brute_chain_rows([("r", q)], [("x", cc.rc(t))], True) == []
    assert c3.brute_chain_rows([("r", q)], [("x", t)], True) == [(0, 0, 0, 53, 0, 0, 53, 0, 0, 0, 1, 20, 2, ((40, 0, 0), (13, 40, 60)))]


def test_join_rule():
    A = (0, 0, 50, 50, 0)
    assert c3.overlap(A, (0, 60, 90, 30, 0)) is None                                 # one diagonal
    assert c3.overlap(A, (5, 60, 90, 30, 0)) == 0 and c3.overlap(A, (-20, 70, 100, 30, 0)) == 0
    assert c3.overlap(A, (5, 40, 90, 50, 0)) == 10                                   # the query decides
    assert c3.overlap(A, (-15, 60, 90, 30, 0)) == 5                                  # the target decides: 50 - 45
    assert c3.overlap(A, (5, 21, 51, 30, 0)) == 29 and c3.overlap(A, (5, 20, 50, 30, 0)) is None     # one base left; none
    assert c3.overlap((5, 60, 90, 30, 0), A) is None


def test_table_equals_enumeration():
    """the O(r^2) table against every chain of every order, wherever the enumeration is affordable"""
    n = 0
    small = [make() for name, make in c3.CASES.items() if not name.startswith("group of")] + [c3.group_case(n) for n in (2, 5, 10)]
    for ref, rec in c3.random_cases() + small + [make() for _n, make in cc.NAMED_CASES if _n != "long diagonals"]:
        for _qn, q in ref:
            for _tn, x in rec:
                for t in (x.upper(), cc.rc(x.upper())):
                    b = c3.blocks_of(q.upper(), t)
                    if 2 <= len(b) <= c3.ENUMERATE_UP_TO:
                        assert c3.best_chain_table(q.upper(), t, b) == c3.best_chain_enumerated(q.upper(), t, b)
                        n += 1
    assert n >= 100


# ---------------------------------------------------------------------------------------------------------------- the case builders
def rows_by_pair(name, ss=True, **kw):
    return {(r[0], r[1]): r for r in c3.brute_of_case(name, ss, **kw)}


def test_gap_cases_hold_gaps():
    got = rows_by_pair("gaps")
    assert got[0, 0][3:] == (90, 0, 0, 90, 0, 0, 0, 1, 30, 2, ((40, 0, 0), (50, 40, 70)))         # the target alone holds 30 more
    assert got[1, 1][3:] == (80, 0, 0, 105, 0, 1, 25, 0, 0, 2, ((45, 0, 0), (35, 70, 45)))        # the query alone
    assert got[2, 2][3:] == (80, 0, 0, 110, 0, 1, 30, 1, 50, 2, ((40, 0, 0), (40, 70, 90)))       # both, of different lengths
    assert got[3, 3][3:] == (110, 0, 0, 150, 0, 1, 40, 0, 0, 2, ((50, 0, 0), (60, 90, 50)))       # the middle exon absent in the target
    assert got[4, 4][3:] == (110, 0, 0, 110, 0, 0, 0, 1, 40, 2, ((50, 0, 0), (60, 50, 90)))       # and in the query
    ref, rec = c3.gap_cases()
    assert [r[3] for r in cc.brute_rows(ref, rec, True) if r[0] == r[1]] == [50, 45, 40, 60, 60]   # unchained: the larger piece


def test_trim_cases_hold_their_overlaps():
    ref, rec = c3.trim_cases()
    k = 0
    for v in (1, 31, 32, 33, 70):
        for ll in (40, 41, 71):
            q, t = ref[k][1], rec[k][1]
            b, (val, parts) = blocks_and_chain(q, t)
            assert b == [(0, 0, ll + v, ll + v, 0), (v, ll, ll + v + 45, v + 45, 0)], (v, ll)
            assert [p[:2] for p in parts] == [(0, 0), (1, v)] and val == (ll + v + 45, ll + v + 45, -2)
            k += 1
    offs = np.cumsum([0] + [len(s) for _n, s in ref])[:-1] + [40, 41, 71] * 5
    assert len({int(o) % 32 for o in offs}) >= 8                                     # block B starts at many places of a packed word


def test_trim_edge_cases():
    ref, rec = c3.trim_edge_cases()
    b, (val, parts) = blocks_and_chain(ref[0][1], rec[0][1])
    assert b[1][2] - b[1][1] == 21 and parts[1][:3] == (1, 20, 1)                    # v = len_B - 1: one base is left
    b, (val, parts) = blocks_and_chain(ref[1][1], rec[1][1])
    assert len(b) == 2 and b[1][2] - b[1][1] == 20 and c3.overlap(b[0], b[1]) is None and len(parts) == 1    # v = len_B: refused
    assert max(0, b[0][2] - b[1][1]) == 20
    got = rows_by_pair("trim edges")
    assert got[2, 2][8:] == (0, 0, 1, 12, 2, ((62, 0, 0), (60, 62, 74)))              # duplication in the target: the query overlaps
    assert got[3, 3][8:] == (1, 12, 0, 0, 2, ((62, 0, 0), (60, 74, 62)))              # the mirror: the target overlaps
    b = c3.blocks_of(ref[3][1], rec[3][1])
    assert b[0][2] - b[1][1] == 0 and (b[0][2] + b[0][0]) - (b[1][1] + b[1][0]) == 12


def test_order_cases():
    ref, rec = c3.order_cases()
    b, (val, parts) = blocks_and_chain(ref[0][1], rec[0][1])
    assert len(b) == 2 and c3.overlap(b[0], b[1]) is None and c3.overlap(b[1], b[0]) is None and val == (60, 60, -1)
    b, (val, parts) = blocks_and_chain(ref[1][1], rec[1][1])
    assert [x[0] for x in b] == [0, 30, -50]                                         # A, B, C: the diagonals of B and C cross
    assert c3.overlap(b[0], b[1]) == 0 and c3.overlap(b[0], b[2]) == 0 and c3.overlap(b[1], b[2]) is None
    assert val == (90, 90, -2) and [p[0] for p in parts] == [0, 1]


def test_threshold_cases():
    ref, rec = c3.threshold_cases()
    assert cc.brute_rows(ref, rec, False) == []                                      # no block alone holds 30 matches
    got = rows_by_pair("thresholds")
    assert sorted(got) == [(0, 0), (2, 2)]
    assert got[0, 0][3:5] == (40, 0) and got[0, 0][13] == ((20, 0, 0), (20, 20, 32))
    assert got[2, 2][3:5] == (30, 0) and got[2, 2][13] == ((20, 0, 0), (10, 20, 30))
    assert blocks_and_chain(ref[1][1], rec[1][1])[1][0] == (29, 29, -2)              # 20 + 9: one short
    assert rows_by_pair("thresholds", True, min_matches=29)[1, 1][3] == 29


def test_tie_cases():
    ref, rec = c3.tie_matches_case()
    b, (val, parts) = blocks_and_chain(ref[0][1], rec[0][1])
    assert [(x[3] - 2 * x[4], x[3]) for x in b] == [(61, 67), (61, 61)] and c3.overlap(b[0], b[1]) is None and val == (61, 67, -1)
    ref, rec = c3.tie_blocks_case()
    b, (val, parts) = blocks_and_chain(ref[0][1], rec[0][1])
    assert len(b) == 3 and c3.chain_of(ref[0][1], rec[0][1], b, (0, 1))[0] == (40, 40, -2) and val == (40, 40, -1) and parts[0][0] == 2
    ref, rec = c3.tie_index_case()
    b, (val, parts) = blocks_and_chain(ref[0][1], rec[0][1])
    assert [(x[3], x[4]) for x in b] == [(40, 0), (40, 0)] and c3.overlap(b[0], b[1]) is None and parts[0][0] == 0
    q, t = ref[1][1], rec[1][1]
    b, (val, parts) = blocks_and_chain(q, t)
    assert c3.chain_of(q, t, b, (0, 2))[0] == c3.chain_of(q, t, b, (1, 2))[0] == val == (70, 70, -2) and [p[0] for p in parts] == [0, 2]
    ref, rec = c3.tie_strand_case()
    q, x = ref[0][1], rec[0][1]
    assert blocks_and_chain(q, x)[1][0] == blocks_and_chain(q, cc.rc(x))[1][0] == (60, 60, -2)
    assert [r[2] for r in c3.brute_of_case("tie: strand", False)] == [0]


def test_minus_and_n_cases():
    (row,) = c3.brute_of_case("minus", False)
    ref, rec = c3.minus_case()
    n = len(rec[0][1])
    assert row[:8] == (0, 0, 1, 150, 0, 0, 159, 5) and row[8:13] == (1, 9, 1, 20, 3)
    assert row[13] == ((40, 0, n - 11 - 40), (60, 40, n - 11 - 40 - 20 - 60), (50, 109, 5))
    assert c3.brute_of_case("minus", True) == ()
    ref, rec = c3.n_trim_cases()
    b, (val, parts) = blocks_and_chain(ref[0][1].upper(), rec[0][1])
    assert [x[4] for x in b] == [1, 1] and parts[1][1] == 40 and ref[0][1][50] == "N" and val == (97, 99, -2)      # B loses its N, A keeps it
    b, (val, parts) = blocks_and_chain(ref[1][1], rec[1][1])
    assert [x[4] for x in b] == [0, 1] and parts[1][1:] == (40, 30, 0) and val == (103, 103, -2)


@pytest.mark.parametrize("n", c3.GROUP_SIZES)
def test_group_cases_hold_n_blocks(n):
    ref, rec = c3.group_case(n)
    assert len(ref[0][1]) == 21 * n - 1 and len(rec[0][1]) == 20 * n
    (row,) = c3.brute_of_case("group of %d" % n, True, 1)
    assert row[12] == n and row[8:10] == ((n - 1, n - 1) if n > 1 else (0, 0))
    assert [b[2] - b[1] for b in row[13]] == list(range(0, -n, -1))                  # piece k on diagonal -k: all n blocks chained


def test_random_cases_hold_chains():
    multi = trimmed = minus = 0
    for ref, rec in c3.random_cases():
        for r in c3.brute_chain_rows(ref, rec, False):
            multi += r[12] > 1
            minus += r[2]
            trimmed += r[12] > 1 and sum(b[0] for b in r[13]) < r[6] - r[5] - r[9] and r[9] == 0
            assert sum(b[0] for b in r[13]) == r[3] + r[4] and r[6] <= len(ref[r[0]][1])
    assert multi >= 40 and minus >= 10


# ---------------------------------------------------------------------------------------------------------------- the host half
def three_block_minus_row(compare):
    # query of 300, target of 500; '-': oriented blocks q[10:50) -> t[100:140), q[50:110) -> t[160:220), q[130:200) -> t[230:300)
    return compare.ChainRows(*(np.array(c, dtype=np.uint32) for c in ([0], [1], [1], [165], [5], [10], [200], [200], [1], [20], [2], [30], [3])),
                             np.array([0, 3], dtype=np.uint64),
                             *(np.array(c, dtype=np.uint32) for c in ([40, 60, 70], [10, 50, 130], [360, 280, 200])))


def test_psl_lines_of_a_three_block_row():
    from shannon_amd import compare
    ref, rec = [("r0", "A" * 300)], [("x0", "G" * 150), ("x1", "T" * 500)]
    (line,) = compare.psl_lines(three_block_minus_row(compare), ref, rec)
    col = line.split("\t")
    assert len(col) == 21
    assert col[0:2] == ["165", "5"] and col[2:4] == ["0", "0"]                       # matches, misMatches; repMatches, nCount
    assert col[4:8] == ["1", "20", "2", "30"]                                        # qNumInsert, qBaseInsert, tNumInsert, tBaseInsert
    assert col[8:11] == ["-", "r0", "300"] and col[11:13] == ["10", "200"]           # strand, qName, qSize; qStart, qEnd
    assert col[13:15] == ["x1", "500"] and col[15:17] == ["200", "400"]              # tName, tSize; tStart = 500 - 300, tEnd = 500 - 100
    assert col[17] == "3" and col[18:] == ["40,60,70,", "10,50,130,", "360,280,200,"]
    # a one-block ChainRows line is the Rows line
    one = compare.ChainRows(*(np.array(c, dtype=np.uint32) for c in ([0], [1], [0], [100], [2], [10], [112], [30], [0], [0], [0], [0], [1])),
                            np.array([0, 1], dtype=np.uint64), *(np.array(c, dtype=np.uint32) for c in ([102], [10], [30])))
    assert compare.psl_lines(one, ref, rec) == compare.psl_lines(compare.Rows(*one[:8]), ref, rec)
    assert compare.psl_lines(c3.chain_rows_of(compare, []), ref, rec) == []


def test_analysis_reads_five_columns():
    """analyze and false_positive on multi-block lines = on one-block lines with the same columns 0, 9, 10, 13 and 14"""
    from shannon_amd import compare
    n = 0
    for ref, rec in c3.random_cases()[:12] + [c3.gap_cases(), c3.minus_case()]:
        rows = c3.brute_chain_rows(ref, rec, False)
        chained = compare.psl_lines(c3.chain_rows_of(compare, rows), ref, rec)
        single = compare.psl_lines(compare.Rows(*(np.array([r[f] for r in rows], dtype=np.uint32) for f in range(8))), ref, rec)
        assert [[l.split("\t")[c] for c in (0, 9, 10, 13, 14)] for l in chained] == [[l.split("\t")[c] for c in (0, 9, 10, 13, 14)] for l in single]
        assert compare.analyze(chained) == compare.analyze(single) and compare.false_positive(rec, chained) == compare.false_positive(rec, single)
        n += sum(1 for l in chained if l.split("\t")[17] != "1")
    assert n >= 10


def test_chain_rows_round_trip():
    from shannon_amd import compare
    rows = list(c3.brute_of_case("gaps", True)) + list(c3.brute_of_case("trims", True))
    assert c3.as_tuples(c3.chain_rows_of(compare, rows)) == rows


# ---------------------------------------------------------------------------------------------------------------- the command
def _command(*args):
    return subprocess.run([sys.executable, "-m", "shannon_amd.compare"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_command_takes_chain_anywhere(tmp_path):
    ref = tmp_path / "ref.fasta"
    ref.write_text(">r\nACGT\n")
    out = str(tmp_path)
    for args in (("--chain", out, str(ref)), (out, "--chain", str(ref)), (out, str(ref), "--chain"), (out, str(ref), "-s", "--chain"), ("--chain", "-s", out, str(ref))):
        p = _command(*args)                                   # an OUT without shannon.fasta: the arguments were accepted, the run refused
        assert p.returncode == 2 and "shannon.fasta: no such file" in p.stderr and "usage" not in p.stderr and p.stdout == "", args
    for args in ((out, str(ref), "--fast"), (out, str(ref), "--chains"), (out, str(ref), "--chain", "--fast"), ("--chain",), (out, "--chain")):
        p = _command(*args)
        assert p.returncode == 2 and p.stderr.startswith("usage: python -m shannon_amd.compare OUT REF.fasta [-s] [--chain]\n") and p.stdout == "", args
    assert sorted(os.listdir(out)) == ["ref.fasta"]


def test_entry_points_take_chain():
    import inspect
    from shannon_amd import compare, reference_api
    for f in (compare.rows, compare.compare_texts, compare.compare, reference_api.run_MB_SF_compare):
        p = inspect.signature(f).parameters["chain"]
        assert p.default is False
    assert list(inspect.signature(compare.compare).parameters) == ["out_dir", "ref_fasta", "strand_specific", "ctx", "chain"]
