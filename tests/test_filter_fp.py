"""CPU: the host half of --filter_FP -- the keep / drop decision and the rec.log / reconstructed.fasta texts against the
reference's own write_filtered_tr (fixture tests/golden/filter_fp_decide.json.gz, made by tests/golden/make_filter_fp_golden.py),
the brute force of the GPU tests on a hand-checked input, and the command line's handling of the flag."""
import gzip, json, os
import pytest
from conftest import ROOT
import filter_fp_cases as fc


@pytest.fixture(scope="module")
def golden():
    return json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "filter_fp_decide.json.gz"), "rt"))["cases"]


def test_fixture_covers_what_it_should(golden):
    from shannon_amd import filter_fp
    lens, seen = set(), set()
    for c in golden:
        _names, seqs = filter_fp.records(c["fasta"])
        assert len(seqs) == len(c["hits"])
        for s, h in zip(seqs, c["hits"]):
            lens.add(len(s))
            k = (9 * len(s) + 9) // 10
            seen.add("below" if h == k - 1 else "at" if h == k else "full" if h == len(s) else "zero" if h == 0 else "other")
        assert any(len(l.split()) > 1 for l in c["fasta"].splitlines() if l.startswith(">"))
    assert set(range(1, 41)) <= lens and max(lens) == 5000
    assert {"below", "at", "full", "zero"} <= seen


def test_filter_text_equals_write_filtered_tr(golden):
    from shannon_amd import filter_fp
    for c in golden:
        kept, log = filter_fp.filter_text(c["fasta"], c["hits"])
        assert log == c["log"]
        assert kept == c["kept"]
        assert filter_fp.filter_text(c["fasta"].encode(), c["hits"]) == (kept, log)          # (the pipeline's texts are bytes)


def test_decide_is_the_float_comparison(golden):
    from shannon_amd import filter_fp
    for c in golden:
        names, seqs = filter_fp.records(c["fasta"])
        kept_names = [l[1:] for l in c["kept"].splitlines() if l.startswith(">")]
        d = filter_fp.decide(c["hits"], [len(s) for s in seqs])
        assert [n for n, k in zip(names, d) if k] == kept_names
    assert filter_fp.decide([9, 8, 0, 0, 1], [10, 10, 0, 1, 1]) == [True, False, True, False, True]
    # the rule's own words: hits >= len * 0.9 in double -- wherever that differs from the integer form 10 hits >= 9 len, the double wins
    for n in range(1, 20001):
        for h in ((9 * n + 9) // 10 - 1, (9 * n + 9) // 10):
            assert filter_fp.decide([h], [n]) == [h >= n * 0.9]


def test_filter_text_refuses_a_wrong_number_of_hits():
    from shannon_amd import filter_fp
    with pytest.raises(ValueError):
        filter_fp.filter_text(">a\nACGT\n", [1, 2])


def test_brute_force_on_a_hand_checked_input():
    """the brute force the GPU tests trust, on an input small enough to check by eye"""
    t = "ACGTTGCAAGGCTTAACCGGATATCGCGATTACAGGCATTCAGGACTTACGGATCCATGCAAGCTTGGCACTGGCCGTCGTTTTACAACGTCGTGACTGGGAAAAC"
    x, y = t[5:35], t[60:90]
    case = fc.make_case([t, t[:40]], [0, 0], 1, [x, x, x[:14]], [fc.rc(y), fc.rc(t[61:91]), fc.rc(y)], ([0, 0, 0], [0, 1, 2]), True)
    hits, placed = fc.brute_hits(case, want_placed=True)
    assert hits == [30 + 31, 0] and placed == 2                     # [5, 35) and [60, 91); the 14-base mate never places
    case["ss"] = False
    case["r1"], case["r2"] = case["r2"], case["r1"]                 # mates swapped: the second oriented pair finds them
    assert fc.brute_hits(case) == [61, 0]
    case["ss"] = True
    assert fc.brute_hits(case) == [0, 0]
    assert fc.brute_hits(fc.make_case([t], [0], 1, [fc.mutate(x, [3])], [fc.rc(y)], ([0], [0]), True)) == [60]      # 1 <= 30 // 30
    assert fc.brute_hits(fc.make_case([t], [0], 1, [fc.mutate(x, [3, 20])], [fc.rc(y)], ([0], [0]), True)) == [0]
    assert fc.brute_hits(fc.make_case([t], [0], 1, [x[:29] + "N"], [fc.rc(y)], ([0], [0]), True)) == [60]
    assert fc.keep([9, 8], [10, 10]) == [True, False]


# ---------------------------------------------------------------------------------------------------------------- command line
def _parse(args, capsys):
    import shannon
    o = shannon.parse_args(["shannon.py"] + args)
    return o, capsys.readouterr().out


def test_cli_filter_fp_is_no_longer_ignored(capsys):
    o, out = _parse(["-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "-s", "--filter_FP", "--compare", "ref.fasta"], capsys)
    assert "--filter_FP" not in o.ignored and o.ignored == ["--compare"]
    assert o.filter_fp is True and o.double_stranded is False and o.reads == ["a.fasta", "b.fasta"]
    assert out.count("OPTIONS --filter_FP: False-positive filtering enabled") == 1
    assert not any("filter_FP" in n for n in o.noted)


def test_cli_repeated_filter_fp_is_harmless(capsys):
    o, out = _parse(["--filter_FP", "-o", "OUT", "--left", "a.fasta", "--filter_FP", "--right", "b.fasta"], capsys)
    assert o.filter_fp is True and o.ignored == [] and out.count("False-positive filtering enabled") == 1


def test_cli_single_end_gives_a_note_and_no_filter(capsys):
    o, _out = _parse(["-o", "OUT", "--single", "a.fasta", "--filter_FP"], capsys)
    assert o.filter_fp is False and o.ignored == []
    notes = [n for n in o.noted if "--filter_FP" in n]
    assert len(notes) == 1 and "single-end" in notes[0] and "run_MB_SF_fn.py:110" in notes[0]


def test_cli_other_flags_parse_as_before(capsys):
    o, out = _parse(["-o", "OUT", "--single", "r.fasta", "-K", "31", "--partition", "300", "-p", "3", "--gpus", "2", "--kmer_hard_cutoff", "2",
                     "--kmer_soft_cutoff", "5", "--inDisk", "--bogus", "--kallisto_cutoff", "1"], capsys)
    assert (o.K, o.partition_size, o.nJobs, o.n_gpus, o.kmer_hard_cutoff, o.min_weight, o.min_length) == (31, 300, 3, 2, 2, 5, 75)
    assert o.double_stranded is True and o.filter_fp is False and o.ignored == ["--bogus", "--kallisto_cutoff"]
    assert len(o.noted) == 1 and o.noted[0].startswith("--inDisk")
    assert "OPTIONS --kmer_hard_cutoff: Kmer hard cutoff set to 2" in out and "OPTIONS --kmer_soft_cutoff: Kmer soft cutoff set to 5" in out
    import shannon
    assert shannon.parse_args(["shannon.py", "--version"]) == 0 and shannon.parse_args(["shannon.py", "-K"]) == 2


def test_cli_flag_without_inputs_still_ends_with_the_usage_error(capsys):
    import shannon
    assert shannon.main(["shannon.py", "--filter_FP"]) == 2
    assert "need -o OUT" in capsys.readouterr().out
