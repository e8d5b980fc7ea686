"""CPU: --quorum.  The brute force of tests/quorum_cases.py on two reads checked by hand, the situations the GPU
tests hold the kernels against (each input really is the situation its name says), the conditions of the planted-error input,
and the command line's gate."""
import pytest
import quorum_cases as qc


def _parse(args, capsys):
    import shannon
    capsys.readouterr()
    o = shannon.parse_args(["shannon.py"] + args)
    return o, capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------------- the rule by hand
SUPPORT = [("GATTACAGGC", "IIIIIIIIII")] * 3
# the seven 4-windows of GATTACAGGC as canonical forms: GATT -> AATC (its reverse complement is smaller), TTAC -> GTAA, the rest
# are their own
CANON = ("AATC", "ATTA", "GTAA", "TACA", "ACAG", "CAGG", "AGGC")


def test_by_hand_a_low_quality_error_is_mended_forward():
    """k = 4, A = 2.  The probe GATTAC[T]GGC has quality # at base 6: its windows 0, 1, 2 are HQ (AATC, ATTA, GTAA: 4 each), those
    over base 6 are not.  Anchor: window 0.  Forward: A and C follow (ATTA, TTAC present); at base 6 TACT (canonical AGTA) is not
    in the table; of TACA, TACC (GGTA), TACG (CGTA) only TACA is: T becomes A, and AGG, GGC follow."""
    files = [[("GATTACTGGC", "IIIIII#III")] + SUPPORT]
    table = qc.brute_table(files, k=4, q=5)
    assert table == {"AATC": 4, "ATTA": 4, "GTAA": 4, "TACA": 3, "ACAG": 3, "CAGG": 3, "AGGC": 3}
    assert set(table) == set(CANON)
    got, st = qc.brute_correct("GATTACTGGC", table, k=4, a=2, w=10, e=3)
    assert got == "GATTACAGGC"
    assert st == {"anchored": 1, "substitutions": 1, "stopped": 0, "reverts": 0}


def test_by_hand_an_n_at_base_0_is_mended_backward():
    """k = 4, A = 2.  NATTACAGGC: window 0 holds the N, so the anchor is window 1 (ATTA, 3 + 1).  Forward everything is present.
    Backward at base 0 there is no read letter: AATT (its own reverse complement), CATT (AATG), TATT (AATA) are not in the table,
    GATT (AATC) is: the N becomes G."""
    files = [[("NATTACAGGC", "IIIIIIIIII")] + SUPPORT]
    table = qc.brute_table(files, k=4, q=5)
    assert table == {"AATC": 3, "ATTA": 4, "GTAA": 4, "TACA": 4, "ACAG": 4, "CAGG": 4, "AGGC": 4}
    got, st = qc.brute_correct("NATTACAGGC", table, k=4, a=2, w=10, e=3)
    assert got == "GATTACAGGC"
    assert st == {"anchored": 1, "substitutions": 1, "stopped": 0, "reverts": 0}
    # with A = 5 no window is an anchor: the read stays as it is, N included
    assert qc.brute_correct("NATTACAGGC", table, k=4, a=5, w=10, e=3) == ("NATTACAGGC", {"anchored": 0, "substitutions": 0, "stopped": 0, "reverts": 0})


def test_by_hand_quality_and_case():
    assert qc.hq_bits("ACgtN", "I&%I&", q=5) == [True, True, False, True, False]        # (& is 5, % is 4, N is never hq)
    assert qc.norm("acgtRn") == "ACGTNN" and qc.can("TTTT") == "AAAA" and qc.can("ACGT") == "ACGT"


# ---------------------------------------------------------------------------------------------------------------- the situations
# what the brute force does with the probe read of every situation: (result: "clean" or "as it was", substitutions, stopped, reverts)
EXPECT = {
    "mid": ("clean", 1, 0, 0), "first_window": ("clean", 1, 0, 0), "last_base": ("clean", 1, 0, 0), "base_0": ("clean", 1, 0, 0),
    "lookahead_settles": ("clean", 1, 0, 0), "lookahead_fails": ("as it was", 0, 1, 0), "no_candidate": ("as it was", 0, 1, 0),
    "n_base": ("clean", 1, 0, 0), "fourth_forward": ("as it was", 0, 1, 1), "fourth_backward": ("as it was", 0, 1, 1),
    "mates_two_lengths": ("clean", 1, 0, 0),
}


@pytest.mark.parametrize("name", qc.SCENARIOS)
def test_every_situation_is_what_its_name_says(name):
    case = qc.scenario(name)
    table = qc.brute_table(case["files"])
    f, i = case["probe"]
    bases, _quals = case["files"][f][i]
    got, st = qc.brute_correct(bases, table)
    if name == "no_anchor":
        assert st["anchored"] == 0 and got == qc.norm(bases)
    elif name == "short":
        assert len(bases) < qc.K and st["anchored"] == 0 and got == bases
    else:
        what, subs, stopped, reverts = EXPECT[name]
        assert st == {"anchored": 1, "substitutions": subs, "stopped": stopped, "reverts": reverts}
        assert got == (case["clean"] if what == "clean" else qc.norm(bases))
        assert (what == "clean") == (got != qc.norm(bases))
    # the support reads are clean: none of them changes (mates_two_lengths has a mended read in either file)
    out, stats, _t = qc.brute_apply(case["files"])
    assert stats["changed"] == (2 if name == "mates_two_lengths" else 1 if name in EXPECT and EXPECT[name][0] == "clean" else 0)
    assert all(len(o) == len(r) for o, r in zip(out, case["files"]))


def test_first_window_anchor_is_not_window_0():
    case = qc.scenario("first_window")
    table = qc.brute_table(case["files"])
    bases = case["files"][0][0][0]
    assert table.get(qc.can(bases[:qc.K]), 0) == 0 and table.get(qc.can(bases[6:6 + qc.K]), 0) >= qc.A


def test_planted_errors_come_back_and_clean_reads_stay():
    """the conditions of the planted-error input, on the brute force: at least 95 % of the altered reads come back to their clean
    text, no clean read is changed"""
    files, clean = qc.planted_case()
    out, stats, _t = qc.brute_apply(files)
    altered = back = 0
    for f in range(2):
        assert len(files[f]) == len(files[0]) >= 400
        for (bases, _q), c, o in zip(files[f], clean[f], out[f]):
            if bases != c:
                altered += 1
                back += o == c
            else:
                assert o == c
    assert altered == (2 * len(files[0]) + 4) // 5
    assert back >= 0.95 * altered, (back, altered)
    assert stats["changed"] >= back


def test_two_error_mates_come_back_too():
    """the input of the --kallisto_cutoff test: the mates with two errors (more than the one mismatch a 50-base mate may carry when
    it is placed) are mended by the brute force, one substitution in either direction from the clean window between them"""
    files, clean, double = qc.kallisto_case()
    out, _stats, table = qc.brute_apply(files)
    assert len(double) == 12 and all(i % 5 == 1 for i in double)
    for i in double:
        bases = files[0][i][0]
        assert sum(a != b for a, b in zip(bases, clean[0][i])) == 2 and files[0][i][1].count("#") == 2
        got, st = qc.brute_correct(bases, table)
        assert got == clean[0][i] == out[0][i] and st == {"anchored": 1, "substitutions": 2, "stopped": 0, "reverts": 0}
        assert out[1][i] == clean[1][i] == files[1][i][0]


# ---------------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("argv", [["--left", "a.fastq", "--right", "b.fastq"], ["--single", "a.fq"], ["--left", "a.fa", "--right", "b.fa", "--fastq"]])
def test_cli_fastq_enables_the_flag(capsys, argv):
    o, out = _parse(["-o", "OUT"] + argv + ["--quorum", "--quorum"], capsys)
    assert o.quorum is True and o.ignored == [] and o.noted == []
    assert out.splitlines().count("OPTIONS --quorum: read error correction with quality scores enabled") == 1


@pytest.mark.parametrize("argv", [["--left", "a.fasta", "--right", "b.fasta"], ["--left", "a.fq", "--right", "b.fq", "--fasta"]])
def test_cli_fasta_warns_and_ignores(capsys, argv):
    o, out = _parse(["-o", "OUT"] + argv + ["--compare", "ref.fa", "--quorum", "--nprocs"], capsys)
    assert o.quorum is False and o.ignored == ["--compare", "--quorum", "--nprocs"] and o.noted == []
    assert "OPTIONS WARNING: --quorum NOT enabled. Option only works with fastq input." in out.splitlines()
    assert "OPTIONS --quorum:" not in out


def test_cli_ignored_flags_keep_their_order(capsys):
    o, _out = _parse(["-o", "OUT", "--single", "a.fasta", "--quorum", "--kallisto_cutoff", "2"], capsys)
    assert o.ignored == ["--quorum", "--kallisto_cutoff"]
    o, _out = _parse(["-o", "OUT", "--single", "a.fasta", "--kallisto_cutoff", "2", "--quorum"], capsys)
    assert o.ignored == ["--kallisto_cutoff", "--quorum"]
    o, _out = _parse(["-o", "OUT", "--single", "a.fasta", "--x", "--quorum", "--y", "--kallisto_cutoff", "2", "--z"], capsys)
    assert o.ignored == ["--x", "--quorum", "--y", "--kallisto_cutoff", "--z"]


@pytest.mark.parametrize("ranks", [["-p", "2"], ["--gpus", "2"]])
def test_cli_ranks_get_a_note(capsys, ranks):
    o, out = _parse(["-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--quorum"] + ranks, capsys)
    assert o.quorum is False and o.ignored == []
    assert len(o.noted) == 1 and o.noted[0].startswith("--quorum: ") and "nothing is corrected" in o.noted[0]
    assert "OPTIONS --quorum: read error correction with quality scores enabled" in out


# what the existing tests pin of parse_args, taken again without the flag: (argv, {attribute: value}, lines printed)
PINNED = [
    (["-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "-s", "--filter_FP", "--compare", "ref.fasta"],
     {"ignored": ["--compare"], "filter_fp": True, "double_stranded": False, "reads": ["a.fasta", "b.fasta"], "noted": []},
     ["OPTIONS --filter_FP: False-positive filtering enabled"]),
    (["-o", "OUT", "--single", "r.fasta", "--inDisk"], {"in_disk": True, "noted": [], "ignored": []}, ["OPTIONS --inDisk: In Memory mode disabled"]),
    (["-o", "OUT", "--left", "a.fq", "--right", "b.fq"], {"kallisto_cutoff": None, "ignored": [], "noted": []}, []),
    (["-o", "OUT", "--left", "a.fq", "--right", "b.fq", "--kallisto_cutoff", "2"], {"kallisto_cutoff": 2.0, "ignored": [], "noted": []},
     ["OPTIONS --kallisto_cutoff: Kallisto will be run to filter low expression transcripts below 2.0"]),
    (["-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "--nprocs", "--kallisto_cutoff", "2", "--compare", "r.fa"],
     {"kallisto_cutoff": None, "ignored": ["--nprocs", "--kallisto_cutoff", "--compare"], "noted": []},
     ["OPTIONS WARNING: --kallisto_cutoff NOT enabled. Option only works with fastq input."]),
]


@pytest.mark.parametrize("argv,attrs,lines", PINNED)
def test_cli_without_the_flag_nothing_changes(capsys, argv, attrs, lines):
    o, out = _parse(argv, capsys)
    assert o.quorum is False
    for name, value in attrs.items():
        assert getattr(o, name) == value, name
    assert out.splitlines() == lines and "quorum" not in out
    # and with it, on these inputs, only what the flag itself says is added
    o2, out2 = _parse(argv + ["--quorum"], capsys)
    fastq = argv[3].endswith("q")
    assert o2.quorum is fastq
    assert o2.ignored == attrs["ignored"] + ([] if fastq else ["--quorum"]) and o2.noted == attrs["noted"]
    assert [l for l in out2.splitlines() if "quorum" not in l] == lines


def test_cli_single_end_kallisto_note_stays(capsys):
    o, _out = _parse(["-o", "OUT", "--single", "a.fq", "--kallisto_cutoff", "2", "--quorum"], capsys)
    assert o.quorum is True and o.kallisto_cutoff is None
    assert len(o.noted) == 1 and o.noted[0].startswith("--kallisto_cutoff: single-end input is not built")
