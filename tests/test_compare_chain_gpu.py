"""GPU: the chained form of --compare.  shn_compare_chains (csrc/compare.hip) through shannon_amd.compare.rows(chain=True) against
the brute force of tests/compare_chain_cases.py (written from the rule, DESIGN.md 3.12 "Chained rows"), rows and blocks field for
field; then compare(chain=True) and the command's --chain on a finished output directory.  Everything is an integer or a text:
every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
import compare_cases as cc
import compare_chain_cases as c3
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def gpu_chains(ctx, ref, rec, ss, **kw):
    from shannon_amd import compare
    return c3.as_tuples(compare.rows(ctx, ref, rec, ss, chain=True, **kw))


NAMED = [n for n in c3.CASES if not n.startswith("group of")]


@pytest.mark.parametrize("ss", [False, True], ids=["both strands", "strand-specific"])
@pytest.mark.parametrize("name", NAMED)
def test_chains_equal_brute_force(ctx, name, ss):
    """gaps in the target, the query and both; overlaps of 1, 31, 32, 33 and 70 at three alignments; one base left and a refused
    join; tandem duplications; swapped exons and crossing diagonals; the row threshold; the four ties; '-'; N in a trim"""
    ref, rec = c3.CASES[name]()
    want = list(c3.brute_of_case(name, ss))
    assert gpu_chains(ctx, ref, rec, ss) == want
    assert len(want) >= 1 or (name == "minus" and ss)


def test_threshold_with_and_without_the_chain(ctx):
    from shannon_amd import compare
    ref, rec = c3.threshold_cases()
    assert cc.as_tuples(compare.rows(ctx, ref, rec, True)) == []                     # two blocks of 20: no row without ..
    got = gpu_chains(ctx, ref, rec, True)
    assert [(r[0], r[3], r[12]) for r in got] == [(0, 40, 2), (2, 30, 2)]           # .. one with; 29 matches none, 30 one
    assert [(r[0], r[3]) for r in gpu_chains(ctx, ref, rec, True, min_matches=29)] == [(0, 40), (1, 29), (2, 30)]


@pytest.mark.parametrize("n", c3.GROUP_SIZES)
def test_group_sizes(ctx, n):
    """groups of 1, 2, 63, 64, 65 and 130 blocks: the lane loop and the shuffle tree at their edges"""
    ref, rec = c3.group_case(n)
    want = list(c3.brute_of_case("group of %d" % n, True, 1))
    st = {}
    assert gpu_chains(ctx, ref, rec, True, min_matches=1, stats=st) == want and want[0][12] == n
    assert st["candidates"] == n and st["groups"] == 1 and st["blocks"] == n and st["multi_block_rows"] == (1 if n > 1 else 0)


@pytest.mark.parametrize("ss", [False, True], ids=["both strands", "strand-specific"])
@pytest.mark.parametrize("name,make", [c for c in cc.NAMED_CASES if c[0] != "long diagonals"], ids=[n for n, _m in cc.NAMED_CASES if n != "long diagonals"])
def test_unchained_cases_chained(ctx, name, make, ss):
    """the inputs of the unchained rule under the chained one: segment ends, both signs of d, strands, N, ties, repeats and a
    low-complexity run (a group of many blocks), isoforms, sequences of 0, 4, 15 and 16 bases"""
    ref, rec = make()
    assert gpu_chains(ctx, ref, rec, ss) == c3.brute_chain_rows(ref, rec, ss)


def test_empty_sets(ctx):
    ref, rec = c3.gap_cases()
    assert gpu_chains(ctx, [], rec, False) == [] and gpu_chains(ctx, ref, [], False) == [] and gpu_chains(ctx, [], [], True) == []
    assert gpu_chains(ctx, [("a", "")], [("b", "")], False) == []
    q = cc.rand_seq(np.random.Generator(np.random.PCG64(3)), 64)
    st = {}
    assert gpu_chains(ctx, [("a", q[:15]), ("b", ""), ("c", q[:16])], [("x", q[:15]), ("y", q[:16]), ("z", "")], False, min_matches=16, stats=st) == \
        [(2, 1, 0, 16, 0, 0, 16, 0, 0, 0, 0, 0, 1, ((16, 0, 0),))]
    assert st["blocks"] == 1 and st["multi_block_rows"] == 0


@pytest.mark.parametrize("block", range(4))
def test_random_inputs(ctx, block):
    """40 small random inputs with skipped and doubled exons, indels, substitutions and N, ten a test, both strand settings"""
    n_rows = n_multi = 0
    for c, (ref, rec) in enumerate(c3.random_cases()[10 * block:10 * block + 10]):
        for ss in (False, True):
            want = c3.brute_chain_rows(ref, rec, ss)
            assert gpu_chains(ctx, ref, rec, ss) == want, (block, c, ss)
            n_rows += len(want)
            n_multi += sum(1 for r in want if r[12] > 1)
    assert n_rows >= 10 and n_multi >= 5


def test_without_chain_nothing_changes(ctx):
    """chain=False through the entry points that gained the switch: shn_compare_rows' rows, its four timer groups and no fifth"""
    from shannon_amd import compare, _lib
    for make in (c3.gap_cases, c3.trim_cases, cc.isoform_cases, cc.strand_cases):
        ref, rec = make()
        for ss in (False, True):
            q_text, q_off = compare._text_of([s for _n, s in ref])
            t_text, t_off = compare._text_of([s for _n, s in rec])
            h = C.c_void_p()
            _lib.check(_lib.lib().shn_compare_rows(ctx.h, q_text.ctypes.data, q_off.ctypes.data, len(ref), t_text.ctypes.data, t_off.ctypes.data, len(rec),
                                                   1 if ss else 0, 30, C.byref(h)))
            try:
                sizes = np.zeros(4, dtype=np.uint64)
                _lib.check(_lib.lib().shn_cmprows_sizes(h, sizes.ctypes.data))
                out = np.zeros((8, max(int(sizes[0]), 1)), dtype=np.uint32)
                _lib.check(_lib.lib().shn_cmprows_export(h, out.ctypes.data))
                with pytest.raises(_lib.ShannonError, match="shn_compare_rows'"):
                    _lib.check(_lib.lib().shn_cmprows_chain_sizes(h, np.zeros(3, dtype=np.uint64).ctypes.data))
            finally:
                _lib.lib().shn_cmprows_destroy(h)
            direct = [tuple(r) for r in out[:, :int(sizes[0])].T.tolist()]
            ctx.timer_reset()
            got = compare.rows(ctx, ref, rec, ss, chain=False)
            assert isinstance(got, compare.Rows) and cc.as_tuples(got) == direct == cc.brute_rows(ref, rec, ss)
            assert sorted(k for k in ctx.timers() if k.startswith("compare.")) == ["compare.index", "compare.rows", "compare.score", "compare.seeds"]
            fa, fb = cc.fasta_text(ref), cc.fasta_text(rec)
            texts, st = compare.compare_texts(ctx, fa, fb, ss, chain=False)
            assert (texts, st) == compare.compare_texts(ctx, fa, fb, ss) and "blocks" not in st
            assert texts["reconstr_per.txt"].splitlines() == compare.psl_lines(got, ref, rec)
    ref, rec = c3.gap_cases()
    ctx.timer_reset()
    compare.rows(ctx, ref, rec, False, chain=True)
    assert sorted(k for k in ctx.timers() if k.startswith("compare.")) == ["compare.chain", "compare.index", "compare.score", "compare.seeds"]


def test_refusals(ctx):
    from shannon_amd import compare, _lib
    with pytest.raises(_lib.ShannonError, match="2\\^20 bases or more"):
        compare.rows(ctx, [("q", "ACGT" * (1 << 18))], [("t", "ACGTACGTACGTACGTACGT")], chain=True)


# ---------------------------------------------------------------------------------------------------------------- a finished OUT
@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """the small assembly of test_compare_gpu.py: synth's pairs of two genes through shannon.main, the planted isoforms as the
    reference FASTA"""
    import shannon
    from shannon_amd import synth
    d = tmp_path_factory.mktemp("compare_chain_cli")
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
    """the four texts from the brute force's chained rows through the module's host functions"""
    from shannon_amd import compare
    rec = compare.records(final_text)
    want = c3.brute_chain_rows(known, rec, ss)
    lines = compare.psl_lines(c3.chain_rows_of(compare, want), known, rec)
    log = compare.analyze(lines)
    rev, n_rec, tot = compare.false_positive(rec, lines)
    return {"reconstr_per.txt": "".join(l + "\n" for l in lines), "reconstr_log.txt": log, "reconstr_rev_log.txt": rev, "compare_log.txt": log}, n_rec, tot, want


def check_files(F, texts):
    alld = F["out"] / "TEMP" / "OUT_allalgo_output"
    for name, text in texts.items():
        p = (F["out"] if name == "compare_log.txt" else alld) / name
        assert p.read_text() == text, name
    assert (alld / "reference.fasta").read_bytes() == F["ref"].read_bytes()


def test_compare_with_the_chain_on_a_finished_run(ctx, finished, capsys):
    from shannon_amd import compare
    F = finished
    final, log = (F["out"] / "shannon.fasta").read_bytes(), (F["out"] / "log.txt").read_bytes()
    texts, n_rec, tot, want = mirror_files(F["known"], final.decode(), False)
    multi = sum(1 for r in want if r[12] > 1)
    capsys.readouterr()
    st = compare.compare(str(F["out"]), str(F["ref"]), ctx=ctx, chain=True)
    assert capsys.readouterr().out == "rows with more than one block: %d of %d\n%d,%d\n" % (multi, len(want), n_rec, tot)
    assert st["rows"] == len(want) >= len(F["known"]) and st["rec"] == n_rec and st["multi_block_rows"] == multi
    check_files(F, texts)
    assert (F["out"] / "shannon.fasta").read_bytes() == final and (F["out"] / "log.txt").read_bytes() == log


def test_command_with_the_chain(finished):
    """python -m shannon_amd.compare --chain OUT REF.fasta -s in a process of its own"""
    F = finished
    final, log = (F["out"] / "shannon.fasta").read_bytes(), (F["out"] / "log.txt").read_bytes()
    texts, n_rec, tot, want = mirror_files(F["known"], final.decode(), True)
    p = subprocess.run([sys.executable, "-m", "shannon_amd.compare", "--chain", str(F["out"]), str(F["ref"]), "-s"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.splitlines()[-2:] == ["rows with more than one block: %d of %d" % (sum(1 for r in want if r[12] > 1), len(want)), "%d,%d" % (n_rec, tot)]
    check_files(F, texts)
    assert (F["out"] / "shannon.fasta").read_bytes() == final and (F["out"] / "log.txt").read_bytes() == log
