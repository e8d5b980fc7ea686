"""CPU: `python -m shannon_amd.quant` -- the brute force of tests/quant_cases.py on a hand-checked input, the fragment-length model
of single reads (abundance.eff_lengths_model) against it and against a bound that follows from the model, the case builders the GPU
tests rely on, and the command's argument checks (nothing of which touches the library or a GPU)."""
import numpy as np
import pytest
import filter_fp_cases as fc
import quant_cases as qc


# ---------------------------------------------------------------------------------------------------------------- the brute force
def test_brute_force_on_a_hand_checked_input():
    t0 = "ACGTTGCAAGGCTTACGATCAGGATCCATG"               # 30 bases
    t1 = "TTTTTTTTTTTTTTTTTTTTGGGGG"                     # 25 bases
    T = [t0, t1, "ACGTACGTACGT", "ACGTTGCAAGGCTTANGATCAGGATCCATG"]      # + one of 12 bases, + t0 with an N: neither takes part
    P = qc.Transcripts(T)
    assert P.placements(t0[3:18]) == [(0, 3, 0)]                       # 15 bases, no mismatch allowed
    assert P.placements(fc.mutate(t0[3:18], [4])) == []
    assert P.placements(t0[3:17]) == []                                # 14 bases: never
    assert P.placements(t0) == [(0, 0, 0)]                             # ends exactly at the last base; thr = 1
    assert P.placements(fc.mutate(t0, [29])) == [(0, 0, 1)]
    assert P.placements(fc.mutate(t0, [0, 29])) == []
    assert P.placements(qc.with_n(t0, [10])) == [(0, 0, 1)]
    assert P.placements(qc.with_n(t0[:29], [10])) == []                # 29 bases: thr 0, an N is one too many
    assert P.placements(t0[1:] + "A") == []                            # would hang over the end by one
    assert P.placements("T" * 15) == [(1, u, 0) for u in range(6)]     # six starts on one transcript
    reads = [t0[3:18], fc.rc(t0[3:18]), "T" * 15, "A" * 15, "ACGTACGTACGTACG", t0[3:17]]
    assert qc.brute_sets(T, reads, False) == [(0,), (0,), (1,), (1,), (), ()]
    assert qc.brute_sets(T, reads, True) == [(0,), (), (1,), (), (), ()]
    classes, mapped = qc.brute_classes(qc.brute_sets(T, reads, False))
    assert classes == {(0,): 2, (1,): 2} and mapped == 4
    # the minimum cost over the orientations decides: forward costs 1 on t0, the reverse complement 0 on u = RC(t0)
    u = fc.rc(t0)
    assert qc.brute_sets([fc.mutate(t0, [7]), u], [t0], False) == [(1,)]
    assert qc.brute_sets([fc.mutate(t0, [7]), u], [t0], True) == [(0,)]
    assert qc.brute_sets([t0, u], [t0], False) == [(0, 1)]             # equal costs: both


def test_the_case_builders_are_what_they_say():
    T, reads, want = qc.orientation_case()
    for ss in (False, True):
        assert qc.brute_sets(T, reads, ss) == want[ss]
    P = qc.Transcripts(T)
    assert len(P.placements(reads[0])) == 1 and len(P.placements(fc.rc(reads[0]))) == 1      # both orientations, two starts, one transcript
    assert fc.rc(reads[1]) == reads[1]
    T, reads, unmapped = qc.end_case()
    sets = qc.brute_sets(T, reads, False)
    assert [i for i, C in enumerate(sets) if not C] == unmapped and sets[0] == (1,) and sets[1] == (1,) and sets[-1] == (1,)
    for case in (qc.budget_case, qc.n_case):
        T, reads, mapped = case()
        for ss in (False, True):
            sets = qc.brute_sets(T, reads, ss)
            assert [bool(C) for C in sets] == [(not ss) if m is None else m for m in mapped]
    for n_tr in (1, 2, 33):
        T, reads = qc.unsorted_case(n_tr)
        assert qc.brute_sets(T, reads, True) == [tuple(range(n_tr))] * 3
    T, reads = qc.length_case(qc.LENGTHS, 66)
    sets = qc.brute_sets(T, reads, False)
    assert sorted(set(len(r) for r in reads)) == qc.LENGTHS
    assert not any(C for C, r in zip(sets, reads) if len(r) == 14) and all(any(C for C, r in zip(sets, reads) if len(r) == L) for L in qc.LENGTHS[1:])


# ---------------------------------------------------------------------------------------------------------------- the model
def test_eff_lengths_model_equals_the_brute_force():
    from shannon_amd import abundance
    lens = [0, 1, 14, 15, 100, 150, 199, 200, 201, 260, 399, 400, 999, 1000, 1001, 5000]
    for mean, sd in ((200.0, 20.0), (180.0, 35.5), (30.0, 5.0), (1500.0, 10.0)):
        got = abundance.eff_lengths_model(lens, mean, sd)
        want = qc.brute_eff_model(lens, mean, sd)
        assert got.dtype == np.float64 and got.tolist() == want.tolist(), (mean, sd)     # the same operations in the same order: equal
    assert abundance.eff_lengths_model(lens).tolist() == qc.brute_eff_model(lens).tolist()
    assert abundance.eff_lengths_model([100, 5000], 1500.0, 10.0).tolist() == [100.0, 5000.0]     # no weight at all below 1,000: len
    with pytest.raises(ValueError):
        abundance.eff_lengths_model([100], 200.0, 0.0)


def test_eff_lengths_model_bound():
    """len >= 400: the window 0..min(len, 999) holds 0..400, which is symmetric about 200 -- its mean is 200 exactly -- and what
    lies beyond 400 weighs less than exp(-50) each: |mu - 200| < 1e-9.  mu = len + 1 - eff."""
    from shannon_amd import abundance
    lens = [400, 401, 450, 600, 999, 1000, 3000]
    eff = abundance.eff_lengths_model(lens)
    for n, e in zip(lens, eff.tolist()):
        assert abs((n + 1.0 - e) - 200.0) < 1e-9, (n, e)
    e150 = float(abundance.eff_lengths_model([150])[0])
    assert 1.0 <= e150 < 150.0
    # a transcript much shorter than the model's fragments still gets a positive effective length
    assert all(x > 0.0 for x in abundance.eff_lengths_model(range(0, 60)).tolist()[1:])


# ---------------------------------------------------------------------------------------------------------------- the command
@pytest.fixture()
def files(tmp_path):
    fa = tmp_path / "t.fasta"
    fa.write_text(">a first\nACGTACGTACGTACGTACGT\nACGT\n>b\nTTTTGGGGCCCCAAAATTTT\n")
    reads = tmp_path / "r.fa"
    reads.write_text(">0\nACGTACGTACGTACGTACGT\n")
    return {"fa": str(fa), "r": str(reads), "out": str(tmp_path / "OUT"), "dir": tmp_path}


def test_targets():
    from shannon_amd import quant
    assert quant.targets(">a first\nacgt\nAC\n\n>b\nTT\n") == (["a", "b"], ["ACGTAC", "TT"])          # multi-line, the first token
    with pytest.raises(quant.QuantError, match="a occurs twice"):
        quant.targets(">a\nACGT\n>b\nAC\n>a x\nGG\n")
    with pytest.raises(quant.QuantError, match="b has no sequence"):
        quant.targets(">a\nACGT\n>b\n>c\nGG\n")
    with pytest.raises(quant.QuantError, match="without a target id"):
        quant.targets(">\nACGT\n")
    assert quant.targets(">short\nACG\n>n\nACGTNNNN\n") == (["short", "n"], ["ACG", "ACGTNNNN"])       # nothing refused for length or content


def test_main_refuses_bad_arguments(files, capsys):
    from shannon_amd import quant
    fa, r, out = files["fa"], files["r"], files["out"]

    def refused(argv, message):
        capsys.readouterr()
        assert quant.main(["quant"] + argv) == 2
        err = capsys.readouterr().err
        assert message in err, err
        assert not (files["dir"] / "OUT").exists()

    refused([fa, "--single", r], "-o DIR is needed")
    refused([fa, "-o", out, "--single", r, "--left", r, "--right", r], "exclude each other")
    refused([fa, "-o", out, "--single", r, "--left", r], "exclude each other")
    refused([fa, "-o", out, "--left", r, "--right", r, "-l", "180"], "single-end")
    refused([fa, "-o", out, "--left", r, "--right", r, "--sd", "30"], "single-end")
    refused([fa, "-o", out, "--left", r], "reads are needed")
    refused([fa, "-o", out], "reads are needed")
    refused(["-o", out, "--single", r], "TRANSCRIPTS.fasta")
    refused([fa, "-o", out, "--single", r, "--cutoff", "x"], "not a number")
    refused([fa, "-o", out, "--single", r, "--sd", "0"], "above 0")
    refused([fa, "-o", out, "--single", r, "--frobnicate"], "unknown option")
    refused([fa, "-o", out, "--single", str(files["dir"] / "nope.fa")], "no such file")
    dup = files["dir"] / "dup.fasta"
    dup.write_text(">a\nACGTACGTACGTACGTACGT\n>a\nTTTTGGGGCCCCAAAATTTT\n")
    refused([str(dup), "-o", out, "--single", r], "a occurs twice")
    empty = files["dir"] / "empty.fasta"
    empty.write_text(">a\n>b\nTTTTGGGGCCCCAAAATTTT\n")
    refused([str(empty), "-o", out, "--single", r], "a has no sequence")


def test_parse_args_accepts_the_documented_forms(files):
    from shannon_amd import quant
    fa, r, out = files["fa"], files["r"], files["out"]
    o = quant.parse_args(["quant", fa, "-o", out, "--single", r, "-s", "--cutoff", "2.5", "-l", "180", "--sd", "25"])
    assert o == {"fasta": fa, "out_dir": out, "single": r, "strand_specific": True, "cutoff": 2.5, "mean": 180.0, "sd": 25.0}
    o = quant.parse_args(["quant", "--left", r, "--right", r, "-o", out, fa])
    assert o == {"fasta": fa, "out_dir": out, "left": r, "right": r, "strand_specific": False}
