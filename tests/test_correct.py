"""CPU: python -m shannon_amd.correct.  The command line, the launch of the ranks, and the brute force of
tests/correct_cases.py: held against quorum_cases.brute_correct, worked by hand on two reads, and checked for the span classes the
GPU comparison stands on."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT
import quorum_cases as qc
import correct_cases as cc


def _files(tmp_path, *names):
    out = []
    for n in names:
        p = tmp_path / n
        p.write_text("@r\nACGT\n+\nIIII\n")
        out.append(str(p))
    return out


def parse(*argv):
    from shannon_amd import correct
    return correct.parse_args(["correct"] + [str(a) for a in argv])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_lanes_split_as_in_quant(tmp_path):
    a, b, c = _files(tmp_path, "a.fq", "b.fq", "c.fq")
    comma = tmp_path / "x,y.fq"
    comma.write_text("@r\nACGT\n+\nIIII\n")
    o = parse("-o", tmp_path / "out", "--single", a + "," + b + "," + c)
    assert o["single"] == [a, b, c] and "left" not in o
    assert parse("-o", tmp_path / "out", "--single", comma)["single"] == [str(comma)]        # a value that names an existing file is one file
    o = parse("-o", tmp_path / "out", "--left", a + "," + b, "--right", c + "," + a)
    from shannon_amd import correct
    assert correct.lanes_of(o) == [(a, c), (b, a)]
    assert o["k"] == 24 and o["q"] == 5 and o["anchor"] == 3 and o["window"] == 10 and o["errors"] == 3 and o["trim"] is False and "min_len" not in o
    o = parse("-o", tmp_path / "out", "--single", a, "--trim", "-k", "20")
    assert o["trim"] is True and o["min_len"] == 20                                           # --min_len defaults to k
    assert parse("-o", tmp_path / "out", "--single", a, "--trim", "--min_len", "1")["min_len"] == 1
    assert "no such file" in parse("-o", tmp_path / "out", "--single", a + "," + str(tmp_path / "none.fq"))


def test_refused_at_parse_time(tmp_path):
    a, b, c = _files(tmp_path, "a.fq", "b.fq", "c.fq")
    base = ["-o", tmp_path / "out", "--single", a]
    assert "--left lists 2 files, --right 1" in parse("-o", tmp_path / "out", "--left", a + "," + b, "--right", c)
    for extra, word in ((["-k", "14"], "-k 14 is outside 15 .. 32"), (["-k", "33"], "-k 33 is outside 15 .. 32"), (["--errors", "5"], "--errors 5 is outside 0 .. 4"),
                        (["--anchor", "0"], "--anchor 0 is outside 1 .."), (["--trim", "--min_len", "0"], "--min_len 0 is outside 1 .."),
                        (["--min_len", "30"], "--min_len belongs to --trim"), (["-k", "x"], "-k x is not an integer"), (["--gpus", "0"], "--gpus 0 is outside"),
                        (["--single", b], "--single given twice"), (["--left", b], "exclude each other"), (["--frob"], "unknown option --frob")):
        msg = parse(*(base + extra))
        assert isinstance(msg, str) and word in msg, (extra, msg)
    assert isinstance(parse(*(base + ["-k", "15", "--errors", "4", "--anchor", "1"])), dict) and isinstance(parse(*(base + ["-k", "32", "--errors", "0"])), dict)
    full = tmp_path / "full"
    full.mkdir()
    (full / "x").write_text("x")
    assert "not empty" in parse("-o", full, "--single", a)
    # ... with exit code 2, a message and the usage, from the command itself
    p = subprocess.run([sys.executable, "-m", "shannon_amd.correct", "-o", str(tmp_path / "out"), "--single", a, "--errors", "5"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")), timeout=300)
    assert p.returncode == 2 and "--errors 5 is outside 0 .. 4" in p.stdout and "usage: python -m shannon_amd.correct" in p.stdout
    assert not (tmp_path / "out").exists()


def test_gpus_starts_that_many_ranks_from_a_parent_that_touches_no_gpu(tmp_path):
    a, b = _files(tmp_path, "a.fq", "b.fq")
    env = dict(os.environ, SHN_CLI_BACKEND="gloo", SHN_CLI_LAUNCH_PROBE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "shannon_amd.correct", "-o", str(tmp_path / "out"), "--left", a + "," + b, "--right", b + "," + a, "--trim", "--gpus", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "launch probe: 3 ranks met, 2 paired lanes, k 24, trim 24, out=" in p.stdout


# ---------------------------------------------------------------------------------------------------------------- the brute force
@pytest.mark.parametrize("name", qc.SCENARIOS)
def test_brute_force_agrees_with_quorum_cases(name):
    files = qc.scenario(name)["files"]
    out, stats, table = qc.brute_apply(files)
    res = cc.brute_run(files)
    assert res["files"] == out and {n: res["stats"][n] for n in stats} == stats
    for f, reads in zip(files, res["reads"]):
        for (bases, _ql), r in zip(f, reads):
            text, st = qc.brute_correct(bases, table)
            assert (r["text"], r["anchored"], r["substitutions"], r["stopped"], r["reverts"]) == (text, st["anchored"], st["substitutions"], st["stopped"], st["reverts"])
            # rule 6: the span holds the anchor window and every substitution that stays; what a revert set back lies outside it
            if r["anchored"]:
                assert 0 <= r["lo"] <= r["hi"] - qc.K and r["hi"] <= len(text)
                assert all(r["lo"] <= p < r["hi"] for p in range(len(text)) if text[p] != qc.norm(bases)[p])
                assert all(p >= r["hi"] for p in r["reverted_right"]) and all(p < r["lo"] for p in r["reverted_left"])
            else:
                assert (r["lo"], r["hi"]) == (0, 0)


def test_brute_force_agrees_on_ragged_reads_and_other_parameters():
    files = qc.ragged_case(n=600)
    for kw in ({}, {"k": 17, "a": 2, "w": 6, "e": 2}, {"k": 31, "e": 4}, {"e": 1, "w": 20}):
        out, stats, table = qc.brute_apply(files, **kw)
        res = cc.brute_run(files, table=table, **kw)
        assert res["files"] == out and {n: res["stats"][n] for n in stats} == stats


def test_spans_worked_by_hand():
    """k = 5, A = 2, W = 3, E = 1 on two reads over the transcript T = CAGATTTTCATATTA, which nothing continues beyond its last base
    and whose 5-mers (and their reverse complements) are 11 different ones, so that every step below has the one candidate named"""
    T, k = "CAGATTTTCATATTA", 5
    table = qc.brute_table([[(T, "I" * len(T))] * 2], k=k)
    assert len(table) == 11 and set(table.values()) == {2}
    # read 1: T with base 9 wrong (C for A) and its last two bases wrong (AC for TA).  Anchor CAGAT at 0, i0 = 0.  Steps d = 0 .. 3 look
    # at bases 5 .. 8 and find them in the table.  Step 4, base 9: TTTCC is absent, TTTCA is the one candidate: substituted.  Steps
    # 5 .. 7, bases 10 .. 12: present.  Step 8, base 13: ATATA is absent; ATATT is in the table and so is ATATG (the reverse complement
    # of CATAT): two candidates, and the read's next base C settles nothing (TATTC and TATGC are both absent): the walk stops.
    # e_f = 8, hi = 0 + 5 + 8 = 13; base 9 stays mended.  There is no walk to the left (i0 = 0): lo = 0.
    r1 = "CAGATTTTCCTATAC"
    got = cc.brute_read(r1, table, k=k, a=2, w=3, e=1)
    assert (got["text"], got["lo"], got["hi"], got["substitutions"], got["stopped"], got["reverts"], got["reverted_right"]) == (T[:13] + "AC", 0, 13, 1, 1, 0, [])
    # read 2: bases 9 and 10 wrong (CA for AT).  Step 4, base 9: substituted as above.  Step 5, base 10: TTCAA is absent, TTCAT the one
    # candidate, and step 4 is inside the window: base 9 is set back, the walk ends.  e_f = 4, hi = 9 -- the first reverted position.
    r2 = "CAGATTTTCCAATTA"
    got = cc.brute_read(r2, table, k=k, a=2, w=3, e=1)
    assert (got["text"], got["lo"], got["hi"], got["reverts"], got["reverted_right"], got["substitutions"]) == (r2, 0, 9, 1, [9], 0)
    # rule 7 on the two as single reads: M = 10 keeps read 1 cut to 13 bases and leaves read 2 (span 9) out; M = 9 keeps both
    run = cc.brute_run([[(r1, "#" * 15), (r2, "#" * 15)]], k=k, a=2, w=3, e=1, trim=True, min_len=10, table=table)
    assert run["files"] == [[T[:13]]] and run["kept"] == [0] and run["trim"] == {"kept": 1, "trimmed": 1, "bases_cut": 2, "below_min": 1, "pairs_dropped": 0}
    run = cc.brute_run([[(r1, "#" * 15), (r2, "#" * 15)]], k=k, a=2, w=3, e=1, trim=True, min_len=9, table=table)
    assert run["files"] == [[T[:13], r2[:9]]] and run["trim"] == {"kept": 2, "trimmed": 2, "bases_cut": 8, "below_min": 0, "pairs_dropped": 0}


def test_every_span_class_occurs():
    """the trim input of the GPU tests exercises every class of span, under the M the GPU tests use"""
    files, idx = cc.trim_case()
    M = cc.TRIM_M
    assert M > qc.K
    res = cc.brute_run(files, trim=True, min_len=M)
    reads = [(f, i, r) for f in (0, 1) for i, r in enumerate(res["reads"][f])]
    kept = set(res["kept"])
    L = lambda r: len(r["text"])
    span = lambda r: r["hi"] - r["lo"]
    classes = {
        "kept whole": [x for x in reads if x[1] in kept and x[2]["lo"] == 0 and x[2]["hi"] == L(x[2])],
        "cut at the 3' end only": [x for x in reads if x[1] in kept and x[2]["lo"] == 0 and x[2]["hi"] < L(x[2])],
        "cut at the 5' end only": [x for x in reads if x[1] in kept and x[2]["lo"] > 0 and x[2]["hi"] == L(x[2])],
        "cut at both ends": [x for x in reads if x[1] in kept and x[2]["lo"] > 0 and x[2]["hi"] < L(x[2])],
        "cut by a window revert": [x for x in reads if x[2]["reverted_right"] and x[2]["hi"] == x[2]["reverted_right"][0]],
        "cut by a window revert and kept": [x for x in reads if x[1] in kept and x[2]["reverted_right"] and x[2]["hi"] == x[2]["reverted_right"][0]],
        "cut by a window revert on the left": [x for x in reads if x[2]["reverted_left"] and x[2]["lo"] == x[2]["reverted_left"][-1] + 1],
        "dropped for having no anchor": [x for x in reads if not x[2]["anchored"] and L(x[2]) >= qc.K],
        "dropped for L < k": [x for x in reads if L(x[2]) < qc.K],
        "dropped with a span of M - 1": [x for x in reads if span(x[2]) == M - 1 and x[1] not in kept],
        "kept with a span of M": [x for x in reads if span(x[2]) == M and x[1] in kept],
        "a pair dropped because of one mate only": [i for i in range(len(files[0])) if (span(res["reads"][0][i]) >= M) != (span(res["reads"][1][i]) >= M)],
    }
    empty = [name for name, members in classes.items() if not members]
    assert not empty, empty
    assert res["trim"]["pairs_dropped"] == len(files[0]) - len(kept) > 0 and res["trim"]["trimmed"] > 0
    # the names say what they were built for
    r = res["reads"][0]
    assert (r[idx["cut_3"]]["lo"], r[idx["cut_3"]]["hi"]) == (0, 50) and (r[idx["cut_5"]]["lo"], r[idx["cut_5"]]["hi"]) == (10, 60)
    assert (r[idx["cut_both"]]["lo"], r[idx["cut_both"]]["hi"]) == (8, 68)
    assert span(r[idx["span_m_minus_1"]]) == M - 1 and span(r[idx["span_m"]]) == M
    # single-end, the default M = k: the reads a revert cut are kept, cut
    single = cc.brute_run(files[:1], trim=True)
    assert idx["revert_right"] in single["kept"] and single["trim"]["pairs_dropped"] == 0


def test_the_lane_effect():
    """a k-mer with 2 high-quality windows in lane 1 and 1 in lane 2 is an anchor (A = 3) only in the sum, and a read is corrected only
    because of that: the brute force over both lanes differs from the brute force lane by lane"""
    lanes, (pl, pi), clean = cc.lane_effect_case()
    t1, t2 = qc.brute_table([lanes[0]]), qc.brute_table([lanes[1]])
    both = qc.brute_table([lanes[0] + lanes[1]])
    assert any(t1.get(x, 0) == 2 and t2.get(x, 0) == 1 and both[x] == 3 for x in both)
    assert max(t1.values()) < qc.A and max(t2.values()) < qc.A
    together = cc.brute_run([lanes[0] + lanes[1]])
    apart = [cc.brute_run([l]) for l in lanes]
    probe = len(lanes[0]) + pi if pl else pi
    assert together["files"][0][probe] == clean != apart[pl]["files"][0][pi] == qc.norm(lanes[pl][pi][0])
    assert together["files"][0] != apart[0]["files"][0] + apart[1]["files"][0]
    assert together["stats"]["substitutions"] == 1 and sum(a["stats"]["anchored"] for a in apart) == 0
