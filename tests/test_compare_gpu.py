"""GPU: --compare.  shn_compare_rows (csrc/compare.hip) through shannon_amd.compare.rows against the brute force of
tests/compare_cases.py (written from the rule), field for field; then compare() and the command on a finished
output directory.  Everything is an integer or a text: every comparison is exact."""
import os
import subprocess
import sys
import numpy as np
import pytest
import compare_cases as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def gpu_rows(ctx, ref, rec, ss, **kw):
    from shannon_amd import compare
    return cc.as_tuples(compare.rows(ctx, ref, rec, ss, **kw))


@pytest.mark.parametrize("ss", [False, True], ids=["both strands", "strand-specific"])
@pytest.mark.parametrize("name,make", cc.NAMED_CASES, ids=[n for n, _m in cc.NAMED_CASES])
def test_rows_equal_brute_force(ctx, name, make, ss):
    ref, rec = make()
    want = cc.brute_rows(ref, rec, ss)
    got = gpu_rows(ctx, ref, rec, ss)
    assert got == want and len(want) >= 1


def test_named_cases_hold_what_they_are_for(ctx):
    """the rows that say a case exercises its path: passes of the wave, the tie rules, the thresholds"""
    ref, rec = cc.long_diagonal_cases()
    got = {(r[0], r[1]): r for r in gpu_rows(ctx, ref, rec, True)}
    assert got[0, 0][3:7] == (2046, 3, 0, 2049)                      # three substitutions inside one segment of 2,049 bases
    assert got[1, 1][5:7] == (0, 2100) and got[1, 1][4] == 6         # across position 2,048
    assert got[2, 2][5:7] == (0, 2048) and got[2, 2][4] == 1         # ends in front of it
    ref, rec = cc.strand_cases()
    got = {(r[0], r[1]): r for r in gpu_rows(ctx, ref, rec, False)}
    assert got[0, 0][2] == 1 and got[0, 0][3] == 120 and got[0, 0][7] == 12        # '-', tStart on the forward strand
    assert got[1, 1][2] == 0 and got[1, 1][3] == 48                  # the palindrome: both orientations alike, '+' stays
    assert got[2, 2][2] == 1 and got[2, 2][3] == 100                 # the clean '-' copy beats the '+' copy with a substitution
    ref, rec = cc.threshold_cases()
    got = {(r[0], r[1]): r for r in gpu_rows(ctx, ref, rec, True)}
    assert (0, 0) not in got and (1, 1) not in got and got[2, 2][3:5] == (30, 0) and got[3, 3][3:5] == (30, 1)
    ref, rec = cc.tie_cases()
    got = {(r[0], r[1]): r for r in gpu_rows(ctx, ref, rec, True)}
    assert got[0, 0][3:7] == (44, 2, 27, 73)                         # score 40 in 40, 43 and 46 positions: the longest
    assert got[1, 1][3:7] == (40, 0, 10, 50)                         # two islands alike: the first
    assert got[2, 2][3:8] == (45, 0, 10, 55, 20)                     # two diagonals alike: the smaller one


def test_empty_sets(ctx):
    ref, rec = cc.diagonal_cases()
    assert gpu_rows(ctx, [], rec, False) == [] and gpu_rows(ctx, ref, [], False) == [] and gpu_rows(ctx, [], [], True) == []
    assert gpu_rows(ctx, [("a", "")], [("b", "")], False) == []


def test_min_matches_and_stats(ctx):
    ref, rec = cc.threshold_cases()
    st = {}
    got = gpu_rows(ctx, ref, rec, True, min_matches=29, stats=st)
    assert got == cc.brute_rows(ref, rec, True, min_matches=29) and len(got) == 3
    assert st["rows"] == 3 and st["candidates"] >= 3 and st["hits"] >= st["candidates"] and st["records"] == sum(len(s) - 15 for _n, s in rec)


@pytest.mark.parametrize("block", range(4))
def test_random_inputs(ctx, block):
    """40 small random inputs with planted shared segments, substitutions and N, ten a test, both settings of the strand switch"""
    n_rows = 0
    for c, (ref, rec) in enumerate(cc.random_cases()[10 * block:10 * block + 10]):
        for ss in (False, True):
            want = cc.brute_rows(ref, rec, ss)
            assert gpu_rows(ctx, ref, rec, ss) == want, (block, c, ss)
            n_rows += len(want)
    assert n_rows >= 10


def test_refusals(ctx):
    from shannon_amd import compare, _lib
    with pytest.raises(_lib.ShannonError, match="2\\^20 bases or more"):
        compare.rows(ctx, [("q", "ACGT" * (1 << 18))], [("t", "ACGTACGTACGTACGTACGT")])


# ---------------------------------------------------------------------------------------------------------------- a finished OUT
@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """a small assembly: synth's pairs of two genes through shannon.main, and the planted isoforms as the reference FASTA (over
    lines of 70 bases, one header with a second token)"""
    import shannon
    from shannon_amd import synth
    d = tmp_path_factory.mktemp("compare_cli")
    (r1, r2), iso = synth.make_dataset(3000, 2, seed=5, sigma=0.5)
    synth.write_fasta(str(d / "r1.fasta"), r1)
    synth.write_fasta(str(d / "r2.fasta"), r2)
    out = d / "OUT"
    os.environ["SHN_MALLOC_TUNE"] = "0"
    try:
        assert shannon.main(["shannon.py", "-o", str(out), "--left", str(d / "r1.fasta"), "--right", str(d / "r2.fasta")]) == 0
    finally:
        del os.environ["SHN_MALLOC_TUNE"]
    known = [("T%d gene=%d" % (k, k // 2), s) for k, s in enumerate(synth.codes_to_strings(iso))]
    ref = d / "known.fasta"
    ref.write_text(cc.fasta_text(known, width=70))
    return {"dir": d, "out": out, "ref": ref, "known": [(n.split()[0], s) for n, s in known]}


def mirror_files(known, final_text, ss):
    """the four texts from the brute force's rows through the module's host functions"""
    from shannon_amd import compare
    rec = compare.records(final_text)
    want = cc.brute_rows(known, rec, ss)
    r = compare.Rows(*(np.array([w[f] for w in want], dtype=np.uint32) for f in range(8)))
    lines = compare.psl_lines(r, known, rec)
    log = compare.analyze(lines)
    rev, n_rec, tot = compare.false_positive(rec, lines)
    return {"reconstr_per.txt": "".join(l + "\n" for l in lines), "reconstr_log.txt": log, "reconstr_rev_log.txt": rev, "compare_log.txt": log}, n_rec, tot, len(want)


def check_files(F, texts):
    sample = "OUT"
    alld = F["out"] / "TEMP" / (sample + "_allalgo_output")
    for name, text in texts.items():
        p = (F["out"] if name == "compare_log.txt" else alld) / name
        assert p.read_text() == text, name
    assert (alld / "reference.fasta").read_bytes() == F["ref"].read_bytes()


def test_compare_on_a_finished_run(ctx, finished, capsys):
    from shannon_amd import compare
    F = finished
    final, log = (F["out"] / "shannon.fasta").read_bytes(), (F["out"] / "log.txt").read_bytes()
    listing = sorted(os.listdir(str(F["out"])))
    texts, n_rec, tot, n_rows = mirror_files(F["known"], final.decode(), False)
    capsys.readouterr()
    st = compare.compare(str(F["out"]), str(F["ref"]), ctx=ctx)
    assert capsys.readouterr().out == "%d,%d\n" % (n_rec, tot)
    assert st["rows"] == n_rows >= len(F["known"]) and st["rec"] == n_rec and tot == final.count(b">")
    check_files(F, texts)
    assert (F["out"] / "shannon.fasta").read_bytes() == final and (F["out"] / "log.txt").read_bytes() == log
    assert sorted(os.listdir(str(F["out"]))) == sorted(listing + ["compare_log.txt"])
    # most of a planted isoform of a small clean run comes back in one transcript
    best = [l.split("\t") for l in texts["reconstr_log.txt"].splitlines() if not l.startswith("#")]
    assert len(best) == len(F["known"]) and max(int(b[2]) / int(b[3]) for b in best) >= 0.9


def test_command(finished):
    """python -m shannon_amd.compare OUT REF.fasta -s in a process of its own: the files of the strand-specific comparison"""
    F = finished
    final = (F["out"] / "shannon.fasta").read_bytes()
    texts, n_rec, tot, _n = mirror_files(F["known"], final.decode(), True)
    p = subprocess.run([sys.executable, "-m", "shannon_amd.compare", str(F["out"]), str(F["ref"]), "-s"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.splitlines()[-1] == "%d,%d" % (n_rec, tot)
    check_files(F, texts)
    assert (F["out"] / "shannon.fasta").read_bytes() == final
