"""CPU: the host half of --kallisto_cutoff -- the command line's gate (shannon.py:289-318), the decision against the reference's
own filter_using_kallisto (fixture tests/golden/kallisto_decide.json.gz, made by tests/golden/make_kallisto_golden.py), the text
of abundance.tsv, the effective lengths, and the brute force of the GPU tests on inputs small enough to check by hand."""
import gzip, json, math, os
import numpy as np
import pytest
from conftest import ROOT
import abundance_cases as ac
import filter_fp_cases as fc

ON = "OPTIONS --kallisto_cutoff: Kallisto will be run to filter low expression transcripts below "
OFF = "OPTIONS WARNING: --kallisto_cutoff NOT enabled. Option only works with fastq input."


def _parse(args, capsys):
    import shannon
    o = shannon.parse_args(["shannon.py"] + args)
    return o, capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("files", [["a.fastq", "b.fastq"], ["a.fq", "b.fq"], ["a.fq", "b.fasta"]])
def test_cli_fastq_by_name_enables_the_flag(capsys, files):
    o, out = _parse(["-o", "OUT", "--left", files[0], "--right", files[1], "--kallisto_cutoff", "2"], capsys)
    assert o.kallisto_cutoff == 2.0 and isinstance(o.kallisto_cutoff, float)
    assert o.ignored == [] and o.noted == []
    assert out.count(ON + "2.0") == 1 and OFF not in out


def test_cli_fastq_flag_enables_it_for_any_name(capsys):
    o, out = _parse(["-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "--kallisto_cutoff", "0.75", "--fastq", "--bogus"], capsys)
    assert o.kallisto_cutoff == 0.75 and o.ignored == ["--bogus"]
    assert ON + "0.75" in out
    o, _out = _parse(["--fastq", "--kallisto_cutoff", "1e1", "-o", "OUT", "--left", "a.txt", "--right", "b.txt"], capsys)       # (any order)
    assert o.kallisto_cutoff == 10.0 and o.ignored == []


def test_cli_fasta_flag_turns_it_off(capsys):
    o, out = _parse(["-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--fasta", "--kallisto_cutoff", "2"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == ["--kallisto_cutoff"]
    assert out.count(OFF) == 1 and ON not in out
    o, out = _parse(["-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--fastq", "--fasta", "--kallisto_cutoff", "2"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == ["--kallisto_cutoff"] and OFF in out


def test_cli_fasta_input_keeps_it_ignored(capsys):
    o, out = _parse(["-o", "OUT", "--left", "x.fasta", "--right", "y.fasta", "--bogus", "--kallisto_cutoff", "2", "--other"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == ["--bogus", "--kallisto_cutoff", "--other"]          # (in the order given)
    assert out.count(OFF) == 1 and ON not in out
    o, out = _parse(["-o", "OUT", "--single", "x.fasta", "--kallisto_cutoff", "not-a-number"], capsys)        # (never parsed, as in the reference)
    assert o.ignored == ["--kallisto_cutoff"] and OFF in out


def test_cli_single_end_fastq_gives_a_note(capsys):
    o, out = _parse(["-o", "OUT", "--single", "r.fastq", "--kallisto_cutoff", "2"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == []
    notes = [n for n in o.noted if "--kallisto_cutoff" in n]
    assert len(notes) == 1 and "single-end" in notes[0] and "nothing is filtered" in notes[0]
    assert ON + "2.0" in out


@pytest.mark.parametrize("flag", ["-p", "--gpus"])
def test_cli_several_ranks_give_a_note(capsys, flag):
    o, out = _parse(["-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--kallisto_cutoff", "2", flag, "2"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == []
    notes = [n for n in o.noted if "--kallisto_cutoff" in n]
    assert len(notes) == 1 and "one-process" in notes[0] and "nothing is" in notes[0]
    assert ON + "2.0" in out


def test_cli_bad_values(capsys):
    import shannon
    assert shannon.parse_args(["shannon.py", "-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--kallisto_cutoff"]) == 2
    assert shannon.parse_args(["shannon.py", "-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--kallisto_cutoff", "much"]) == 2
    assert "needs a number" in capsys.readouterr().out
    o, _out = _parse(["-o", "OUT", "--left", "a.fq", "--right", "b.fq"], capsys)
    assert o.kallisto_cutoff is None and o.ignored == []


# ---------------------------------------------------------------------------------------------------------------- decision
@pytest.fixture(scope="module")
def golden():
    return json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "kallisto_decide.json.gz"), "rt"))["cases"]


def test_fixture_covers_what_it_should(golden):
    kinds = {c["what"] for c in golden}
    assert {"cov equal the cutoff", "cov one ulp below the cutoff", "cov one ulp above the cutoff", "texts", "lines before the first header"} <= kinds
    for c in golden:
        if c["what"].startswith("cov "):
            _name, _len, el, ecn, _tpm = c["tsv"].splitlines()[1].split()
            cov = float(ecn) / float(el) * c["L"]
            want = {"cov equal the cutoff": cov, "cov one ulp below the cutoff": math.nextafter(cov, math.inf),
                    "cov one ulp above the cutoff": math.nextafter(cov, -math.inf)}[c["what"]]
            assert c["cutoff"] == want
            assert bool(c["kept"]) == (c["what"] != "cov one ulp below the cutoff")
    texts = [c for c in golden if c["what"] == "texts"]
    heads = [l for l in texts[0]["fasta"].splitlines() if l.startswith(">")]
    table = {l.split()[0] for l in texts[0]["tsv"].splitlines()[1:]}
    assert any(len(h.split()) > 1 for h in heads) and any(h.split()[0][1:] not in table for h in heads)
    assert "\n\n" in texts[0]["fasta"] and any(float(l.split()[3]) == 0.0 for l in texts[0]["tsv"].splitlines()[1:])
    assert texts[0]["fasta"].count("\n") > 2 * len(heads)                      # sequences over several lines
    assert any(c["kept"] not in ("", c["fasta"]) for c in texts)               # some cutoff keeps a part


def test_decide_equals_filter_using_kallisto(golden):
    from shannon_amd import abundance
    for c in golden:
        assert abundance.decide(c["tsv"], c["fasta"], c["cutoff"], c["L"]) == c["kept"], c["what"]


def test_decide_write_now_carries_over():
    from shannon_amd import abundance
    tsv = abundance.HEADER + "a\t100\t60.0\t10.0\t5.0\nb\t100\t60.0\t0.1\t5.0\n"
    fa = "ACGT\n>b\nAAAA\nCCCC\n>a more tokens\nGGGG\n\nTTTT\n>c\nACAC\n"
    assert abundance.decide(tsv, fa, 2.5, 200) == "ACGT\n>a more tokens\nGGGG\n\nTTTT\n"
    assert abundance.decide(tsv, fa, 0.0, 200) == "ACGT\n>b\nAAAA\nCCCC\n>a more tokens\nGGGG\n\nTTTT\n"
    assert abundance.decide(tsv, fa, 1e9, 200) == "ACGT\n"


# ---------------------------------------------------------------------------------------------------------------- table
def test_abundance_tsv_round_trips_the_floats():
    from shannon_amd import abundance
    vals = [0.1 + 0.2, 1e-8, 123456.789e-3, 2.0 / 3.0, 0.0, 1e22]
    t = {"names": ["t%d" % i for i in range(len(vals))], "length": [100 + i for i in range(len(vals))], "eff_length": [v + 1.0 for v in vals],
         "est_counts": vals, "tpm": [v * 3.0 for v in vals]}
    text = abundance.abundance_tsv(t)
    lines = text.splitlines()
    assert lines[0] == "target_id\tlength\teff_length\test_counts\ttpm" and text.endswith("\n") and len(lines) == len(vals) + 1
    for i, l in enumerate(lines[1:]):
        name, n, el, ecn, tpm = l.split("\t")
        assert (name, int(n)) == ("t%d" % i, 100 + i)
        assert float(el) == vals[i] + 1.0 and float(ecn) == vals[i] and float(tpm) == vals[i] * 3.0
    # what the decision reads is what was computed
    assert abundance.decide(text, ">t3\nACGT\n", (2.0 / 3.0) / (2.0 / 3.0 + 1.0) * 200, 200) == ">t3\nACGT\n"


def test_eff_lengths_follow_the_rule():
    from shannon_amd import abundance
    hist = np.zeros(501, np.uint64)
    hist[200], hist[300], hist[500] = 3, 1, 7
    lens = [10, 199, 200, 250, 300, 499, 500, 501, 4000, 0]
    got = abundance.eff_lengths(lens, hist)
    want = [10.0, 199.0, 1.0, 51.0, 300 - 225.0 + 1, 499 - 225.0 + 1, 500 - (600 + 300 + 3500) / 11 + 1, 501 - (600 + 300 + 3500) / 11 + 1,
            4000 - (600 + 300 + 3500) / 11 + 1, 0.0]
    assert got.tolist() == want
    assert got.tolist() == ac.brute_eff(lens, [int(x) for x in hist]).tolist()
    assert abundance.eff_lengths([100, 1000], np.zeros(501, np.uint64)).tolist() == [100.0, 1000.0]          # an empty histogram
    h2 = np.zeros(501, np.uint64)
    h2[300] = 1
    assert abundance.eff_lengths([300, 301], h2).tolist() == [1.0, 2.0]
    assert abundance.tpm_of([1.0, 3.0, 0.0], [10.0, 10.0, 5.0]) == [250000.0, 750000.0, 0.0] and abundance.tpm_of([0.0], [5.0]) == [0.0]


# ---------------------------------------------------------------------------------------------------------------- brute force
def test_brute_force_on_a_hand_checked_input():
    """the brute force the GPU tests trust, on inputs small enough to check by eye"""
    t = "ACGTTGCAAGGCTTAACCGGATATCGCGATTACAGGCATTCAGGACTTACGGATCCATGCAAGCTTGGCACTGGCCGTCGTTTTACAACGTCGTGACTGGGAAAAC"
    x, y = t[5:35], t[60:90]
    T = [t, t + "ACGTAGCATCGACTAGCAT", t[:40], "ACGTACGTAC", t[:50] + "N" + t[50:]]
    frags = ac.brute_fragments(T, [x, x[:14], t[0:30]], [fc.rc(y), fc.rc(y), fc.rc(T[1][-30:])], True)
    # the first pair lies on transcripts 0 and 1 (the one with the N and the short ones take part in nothing), the 14-base mate never
    # places, the third pair reaches into transcript 1's own tail: one placement, span = its whole length
    assert frags == [((0, 1), 2, 85), ((), 0, None), ((1,), 1, len(T[1]))]
    classes, hist, mapped = ac.brute_classes(frags)
    assert classes == {(0, 1): 1, (1,): 1} and mapped == 2 and sum(hist) == 1 and hist[len(T[1])] == 1
    swapped = ac.brute_fragments(T, [fc.rc(y)], [x], False)
    assert swapped == [((0, 1), 2, 85)] and ac.brute_fragments(T, [fc.rc(y)], [x], True) == [((), 0, None)]


def test_brute_em_closed_form_and_stop_rule():
    lists, n_c, eff, m = ac.em_cases()["shared pair"]
    alpha, rounds, tested = ac.brute_em(lists, n_c, eff, m)
    # equal effective lengths: the shared 20 are split 30 : 10
    assert rounds == 50 and np.allclose(alpha, [45.0, 15.0], rtol=1e-12, atol=0) and tested[0] < 1e-12
    lists, n_c, eff, m = ac.em_cases()["a transcript in no class"]
    alpha, rounds, _ = ac.brute_em(lists, n_c, eff, m)
    assert alpha[2] == 0.0 and alpha[3] == 7.0 and abs(alpha.sum() - 62.0) < 1e-9
    for name, (lists, n_c, eff, m) in ac.em_cases().items():
        alpha, rounds, tested = ac.brute_em(lists, n_c, eff, m)
        assert rounds % 50 == 0 and rounds <= 200 and len(tested) == rounds // 50, name
        assert abs(alpha.sum() - sum(n_c)) < 1e-6 * sum(n_c), name                  # every fragment is given to somebody
        assert not any(0.5e-2 <= r <= 2e-2 for r in tested), (name, tested)       # the stated condition of the GPU comparison
    assert max(len(M) for M in ac.em_cases()["a class of 65"][0]) == 65
    assert sum(1 for M in ac.em_cases()["a transcript in 130 classes"][0] if 0 in M) == 130
    eff = ac.em_cases()["eff a factor 100 apart"][2]
    assert eff.max() / eff.min() > 100


def test_shared_exon_case_has_the_set_sizes_it_names():
    T, r1, r2, want = ac.shared_exon_case()
    classes, _hist, mapped = ac.brute_classes(ac.brute_fragments(T, r1, r2, True))
    assert {len(C): n for C, n in classes.items()} == want == {65: 5, 64: 4, 2: 3, 1: 6} and mapped == len(r1) - 1


def test_em_bits_fixture_covers_every_em_case():
    """tests/golden/abundance_em_bits.json (the GPU test's reference): every em_cases() entry with its own n_c and 65 bootstrap rows, the
    union case with its five"""
    with open(os.path.join(ROOT, "tests", "golden", "abundance_em_bits.json")) as f:
        cases = json.load(f)["cases"]
    assert sorted(cases) == sorted(ac.em_golden_names()) == sorted(list(ac.em_cases()) + ["union"])
    for name, rows in cases.items():
        assert [r[0] for r in rows] == (["u%d" % k for k in range(5)] if name == "union" else ["n_c"] + ["b%d" % b for b in range(65)]), name
        assert all(r[1] % 50 == 0 and 50 <= r[1] <= 10000 and len(r[2]) == 64 and int(r[2], 16) >= 0 for r in rows), name
    assert ac.em_golden_case("union")[3] == [r[0] for r in cases["union"]] and ac.em_golden_case("shared pair")[1].shape == (66, 3)
