"""GPU: `python -m shannon_amd.quant`.  shn_abundance_classes_single (csrc/abundance.hip) through shannon_amd.abundance against the brute
force of tests/quant_cases.py (written from the rule, DESIGN.md 3.13, without seeds): compatibility sets, classes, mapped and read
counts are integers and compared exactly; quantify_single's alpha to a relative 1e-9 (absolute 1e-12) with the rounds used equal
(the figures of DESIGN.md 3.10); then the command on single-end and on paired files."""
import numpy as np
import pytest
import abundance_cases as ac
import filter_fp_cases as fc
import quant_cases as qc
from test_abundance_gpu import merged, upload

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def gpu_classes(ctx, T, reads, ss):
    from shannon_amd import abundance, device
    d = upload(ctx, reads) if reads else device.Reads.from_strings(ctx, [])
    try:
        return abundance.classes_single(ctx, T, d, ss)
    finally:
        d.close()


def check_classes(ctx, T, reads, ss, sets=None):
    """the device's classes of the reads against the brute force's sets (computed here unless given)"""
    sets = sets if sets is not None else qc.brute_sets(T, reads, ss)
    want, mapped = qc.brute_classes(sets)
    cl = gpu_classes(ctx, T, reads, ss)
    got = merged(cl)
    print("classes (ss %s): brute force %s\n                   device      %s" % (ss, sorted(want.items())[:12], sorted(got.items())[:12]))
    assert got == want
    assert len(cl["n_c"]) == len(want)                        # equal sets collapse (no 64-bit collision at these sizes)
    assert cl["mapped"] == mapped == int(cl["n_c"].sum()) and cl["fragments"] == len(reads)
    assert len(cl["hist"]) == 0                               # single reads: no span, 0 bins
    return sets, cl


# ------------------------------------------------------------------------------------------------ compatibility sets
@pytest.mark.parametrize("ss", [True, False])
def test_read_lengths_fixed(ctx, ss):
    """a set of one length for every length at which the seed count or the word count of a read steps"""
    for L in qc.LENGTHS:
        T, reads = qc.length_case([L], 12, seed=100 + L)
        sets, cl = check_classes(ctx, T, reads, ss)
        assert (cl["mapped"] == 0) == (L == 14), L


@pytest.mark.parametrize("ss", [True, False])
def test_read_lengths_ragged(ctx, ss):
    T, reads = qc.length_case(qc.LENGTHS, 66)
    sets, cl = check_classes(ctx, T, reads, ss)
    assert 0 < cl["mapped"] < 66
    if not ss:
        one = gpu_classes(ctx, T, reads, True)                # every second read is a reverse complement
        assert one["mapped"] < cl["mapped"]


@pytest.mark.parametrize("ss", [True, False])
def test_transcript_ends(ctx, ss):
    """a read that ends exactly at its transcript's last base maps; one base over either end -- with the neighbour's base -- does not"""
    T, reads, unmapped = qc.end_case()
    sets, _cl = check_classes(ctx, T, reads, ss)
    assert [i for i, C in enumerate(sets) if not C] == unmapped


@pytest.mark.parametrize("ss", [True, False])
def test_mismatch_budget(ctx, ss):
    T, reads, mapped = qc.budget_case()
    sets, _cl = check_classes(ctx, T, reads, ss)
    assert [bool(C) for C in sets] == [(not ss) if m is None else m for m in mapped]


@pytest.mark.parametrize("ss", [True, False])
def test_reads_with_n(ctx, ss):
    T, reads, mapped = qc.n_case()
    sets, _cl = check_classes(ctx, T, reads, ss)
    assert [bool(C) for C in sets] == [(not ss) if m is None else m for m in mapped]


@pytest.mark.parametrize("ss", [True, False])
def test_orientations(ctx, ss):
    """both orientations on one transcript: listed once; a palindromic read; a better reverse placement beats a worse forward one
    unless strand-specific; a transcript of 12 bases and one with an N take part in nothing"""
    T, reads, want = qc.orientation_case()
    sets, cl = check_classes(ctx, T, reads, ss)
    assert sets == want[ss]
    assert not any(4 in C or 5 in C for C in sets)
    off = cl["class_off"].astype(np.int64)
    assert all(off[c + 1] - off[c] == 1 for c in range(len(cl["n_c"])))


# ---------------------------------------------------------------------------------------------------------------- classes
@pytest.mark.parametrize("n_tr", [1, 2, 32, 33, 64, 65, 1001])
def test_a_list_that_arrives_unsorted(ctx, n_tr):
    """every read's placements arrive as the odd transcripts, then the even ones: sorted by insertion (up to 32 ids) or by heapsort
    (33 and more), one class of all transcripts"""
    T, reads = qc.unsorted_case(n_tr)
    sets, cl = check_classes(ctx, T, reads, True)
    assert sets == [tuple(range(n_tr))] * 3
    assert cl["members"].tolist() == list(range(n_tr)) and cl["n_c"].tolist() == [3] and cl["mapped"] == 3


@pytest.fixture(scope="module")
def count_reference():
    """the brute force's sets of count_case's 257 reads, computed once"""
    T, reads = qc.count_case()
    return T, reads, {ss: qc.brute_sets(T, reads, ss) for ss in (True, False)}


@pytest.mark.parametrize("ss", [True, False])
def test_read_counts_at_wave_and_block_edges(ctx, count_reference, ss):
    T, reads, sets = count_reference
    for n in (1, 63, 64, 65, 255, 256, 257):
        _sets, cl = check_classes(ctx, T, reads[:n], ss, sets=sets[ss][:n])
        assert cl["fragments"] == n
    assert 0 < sum(1 for C in sets[ss] if C) < 257
    again = gpu_classes(ctx, T, reads, ss)                    # the export is identical across two runs
    for k in ("class_off", "members", "n_c"):
        assert np.array_equal(cl[k], again[k])


def test_no_reads_and_nothing_to_map_onto(ctx):
    T, reads = qc.count_case()
    for ss in (True, False):
        cl = gpu_classes(ctx, T, [], ss)
        assert cl["mapped"] == 0 and cl["fragments"] == 0 and len(cl["n_c"]) == 0 and cl["class_off"].tolist() == [0] and len(cl["hist"]) == 0
        cl = gpu_classes(ctx, ["ACGTACGT", "ACGTNACGTACGTACGTACGTACGT"], reads, ss)
        assert cl["mapped"] == 0 and cl["fragments"] == len(reads) and len(cl["n_c"]) == 0 and cl["class_off"].tolist() == [0]
        cl = gpu_classes(ctx, [], reads, ss)
        assert cl["mapped"] == 0 and len(cl["n_c"]) == 0
        rng = np.random.Generator(np.random.PCG64(77))
        cl = gpu_classes(ctx, [fc.rand_seq(rng, 300)], reads[:70], ss)          # transcripts, but none the reads map onto
        assert cl["mapped"] == 0 and cl["class_off"].tolist() == [0]


def test_bad_arguments_are_refused(ctx):
    import ctypes as C
    from shannon_amd import _lib
    L = _lib.lib()
    d = upload(ctx, ["ACGTACGTACGTACGTACGT"])
    text = np.frombuffer(b"ACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
    good, bad0, down = (np.array(x, dtype=np.uint64) for x in ([0, 24], [1, 24], [0, 24, 12]))
    h = C.c_void_p()
    try:
        for args, msg in (((None, text.ctypes.data, good.ctypes.data, 1, d.h, 0, C.byref(h)), "NULL argument"),
                          ((ctx.h, text.ctypes.data, good.ctypes.data, 1, None, 0, C.byref(h)), "NULL argument"),
                          ((ctx.h, None, good.ctypes.data, 1, d.h, 0, C.byref(h)), "NULL argument"),
                          ((ctx.h, text.ctypes.data, None, 1, d.h, 0, C.byref(h)), "NULL argument"),
                          ((ctx.h, text.ctypes.data, good.ctypes.data, 1, d.h, 0, None), "NULL argument"),
                          ((ctx.h, text.ctypes.data, bad0.ctypes.data, 1, d.h, 0, C.byref(h)), "t_off\\[0\\] is not 0"),
                          ((ctx.h, text.ctypes.data, down.ctypes.data, 2, d.h, 0, C.byref(h)), "t_off not monotone")):
            ctx.timer_reset()
            with pytest.raises(_lib.ShannonError, match="shn_abundance_classes_single: " + msg):
                _lib.check(L.shn_abundance_classes_single(*args))
            assert not any(k.startswith("abundance.") for k in ctx.timers()), "nothing launched"
            assert not h.value
        # a handle without a histogram: 0 bins, export takes a NULL hist
        _lib.check(L.shn_abundance_classes_single(ctx.h, text.ctypes.data, good.ctypes.data, 1, d.h, 0, C.byref(h)))
        sizes = np.zeros(6, dtype=np.uint64)
        _lib.check(L.shn_abundance_sizes(h, sizes.ctypes.data))
        assert sizes.tolist() == [1, 1, 1, 1, 1, 0]
        off, mem, n_c = np.zeros(2, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        _lib.check(L.shn_abundance_export(h, off.ctypes.data, mem.ctypes.data, n_c.ctypes.data, None))
        assert off.tolist() == [0, 1] and mem.tolist() == [0] and n_c.tolist() == [1]
        L.shn_abundance_destroy(h)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope="module")
def isoforms():
    """isoform_case and the brute force's table for it, strand-specific and not, computed once"""
    names, T, reads, rare = qc.isoform_case()
    return names, T, reads, rare, {ss: qc.brute_table(T, reads, ss) for ss in (True, False)}


@pytest.mark.parametrize("ss", [True, False])
def test_quantify_single_against_the_brute_force(ctx, isoforms, ss):
    from shannon_amd import abundance
    names, T, reads, _rare, tables = isoforms
    T, names = T + ["ACGTNACGTACGTACGTACGT" * 3, "ACGTACGTAC"], names + ["withN", "short10"]
    B = tables[ss]                                            # (the two extra transcripts take part in no set: the brute force's classes stay)
    eff = qc.brute_eff_model([len(t) for t in T])
    # the stated condition: at no tested round does the largest relative change lie where rounding could move the stop
    assert not any(0.5e-2 <= r <= 2e-2 for r in B["tested"]) and B["rounds"] <= 200, B["tested"]
    keys = sorted(B["classes"])
    want, rounds, tested = ac.brute_em([list(k) for k in keys], [B["classes"][k] for k in keys], eff, len(T))
    assert not any(0.5e-2 <= r <= 2e-2 for r in tested), tested
    d = upload(ctx, reads)
    try:
        t = abundance.quantify_single(ctx, names, T, d, ss)
    finally:
        d.close()
    assert t["names"] == names and t["length"] == [len(s) for s in T]
    assert t["eff_length"] == eff.tolist() and t["mapped"] == B["mapped"] and t["fragments"] == len(reads) and t["classes"] == len(B["classes"])
    got = np.array(t["est_counts"])
    err = np.abs(got - want)
    print("quantify_single (ss %s): rounds %d (brute force %d), max absolute error %.3e, max relative error %.3e"
          % (ss, t["rounds"], rounds, float(err.max()), float((err[want > 0] / want[want > 0]).max())))
    assert t["rounds"] == rounds
    assert np.all(err <= ATOL + RTOL * np.abs(want))
    assert got[names.index("withN")] == 0.0 and got[names.index("short10")] == 0.0
    assert abs(sum(t["tpm"]) - 1e6) < 1e-3 and abs(got.sum() - t["mapped"]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- the command
def _write_reads(path, reads, fastq):
    path.write_text("".join(("@%d\n%s\n+\n%s\n" % (i, s, "I" * len(s))) if fastq else (">%d\n%s\n" % (i, s)) for i, s in enumerate(reads)))
    return str(path)


def _run(argv, capsys):
    from shannon_amd import quant
    capsys.readouterr()
    rc = quant.main(["quant"] + argv)
    out = capsys.readouterr()
    assert rc == 0, out.err
    return out.out


def test_command_single_end(ctx, isoforms, tmp_path, capsys):
    """synthetic isoforms, one transcript barely expressed: --cutoff drops exactly that one; filtered.fasta is abundance.decide on
    the written table; FASTQ and FASTA reads give the same table; the transcripts as a multi-line FASTA too"""
    from shannon_amd import abundance
    names, T, reads, rare, tables = isoforms
    B = tables[False]
    C = 3.0
    assert all(c < C * (1 - 1e-3) or c > C * (1 + 1e-3) for c in B["cov"])          # no cov near the cutoff: rounding cannot flip a decision
    assert [n for n, c in zip(names, B["cov"]) if c < C] == [rare]
    fa = tmp_path / "t.fasta"
    fa.write_text("".join(">%s some words\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in zip(names, T)))
    fq, rfa = _write_reads(tmp_path / "r.fastq", reads, True), _write_reads(tmp_path / "r.fa", reads, False)
    out = tmp_path / "Q1"
    printed = _run([str(fa), "-o", str(out), "--single", fq, "--cutoff", str(C)], capsys)
    assert "%d of %d reads mapped" % (B["mapped"], len(reads)) in printed and "%d of %d transcripts kept" % (len(names) - 1, len(names)) in printed
    tsv = (out / "abundance.tsv").read_text()
    assert tsv.startswith(abundance.HEADER)
    rows = [l.split("\t") for l in tsv.splitlines()[1:]]
    assert [r[0] for r in rows] == names and [int(r[1]) for r in rows] == [len(s) for s in T]
    assert [float(r[2]) for r in rows] == B["eff"].tolist()
    assert np.all(np.abs(np.array([float(r[3]) for r in rows]) - B["alpha"]) <= ATOL + RTOL * B["alpha"])
    filtered = (out / "filtered.fasta").read_text()
    assert filtered == abundance.decide(tsv, fa.read_text(), C, B["L"])
    assert [l[1:].split()[0] for l in filtered.splitlines() if l.startswith(">")] == [n for n in names if n != rare]
    log = (out / "quant_log.txt").read_text()
    assert "reads: %d of %d mapped, %d classes, %d EM rounds, L %r" % (B["mapped"], len(reads), len(B["classes"]), B["rounds"], B["L"]) in log
    assert "abundance.map" in log and "abundance.classes" in log and "abundance.index" in log and "abundance.em" in log
    # FASTA reads: the same table; without --cutoff no filtered.fasta
    out2 = tmp_path / "Q2"
    _run([str(fa), "-o", str(out2), "--single", rfa], capsys)
    assert (out2 / "abundance.tsv").read_text() == tsv and not (out2 / "filtered.fasta").exists()
    # ... and so does a multi-line FASTA of the reads, which the device ingest declines: read record by record
    out4 = tmp_path / "Q4"
    wrapped = tmp_path / "wrapped.fa"
    wrapped.write_text("".join(">%d\n%s\n%s\n" % (i, s[:40], s[40:]) for i, s in enumerate(reads)))
    _run([str(fa), "-o", str(out4), "--single", str(wrapped)], capsys)
    assert (out4 / "abundance.tsv").read_text() == tsv
    # -l / --sd move the effective lengths, and with them the table
    out3 = tmp_path / "Q3"
    _run([str(fa), "-o", str(out3), "--single", rfa, "-l", "150", "--sd", "10"], capsys)
    rows3 = [l.split("\t") for l in (out3 / "abundance.tsv").read_text().splitlines()[1:]]
    assert [float(r[2]) for r in rows3] == qc.brute_eff_model([len(s) for s in T], 150.0, 10.0).tolist()


def test_command_strand_specific_differs(ctx, tmp_path, capsys):
    """reads of B given as reverse complements: without -s both transcripts get their reads, with -s B gets none"""
    names, T, reads = qc.stranded_case()
    fa = tmp_path / "t.fasta"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in zip(names, T)))
    rf = _write_reads(tmp_path / "r.fq", reads, True)
    est = {}
    for ss in (False, True):
        out = tmp_path / ("S%d" % ss)
        _run([str(fa), "-o", str(out), "--single", rf] + (["-s"] if ss else []), capsys)
        est[ss] = [float(l.split("\t")[3]) for l in (out / "abundance.tsv").read_text().splitlines()[1:]]
        B = qc.brute_table(T, reads, ss)
        assert np.all(np.abs(np.array(est[ss]) - B["alpha"]) <= ATOL + RTOL * B["alpha"])
    assert est[False] == [150.0, 150.0] and est[True] == [150.0, 0.0]


def test_command_paired_is_quantify(ctx, tmp_path, capsys):
    """paired input: abundance.tsv is byte for byte abundance.abundance_tsv(abundance.quantify(...)) on the same inputs"""
    from shannon_amd import abundance, quant
    T, names, r1, r2 = fc.planted_case(n_pairs=400)
    fa = tmp_path / "t.fasta"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in zip(names, T)))
    f1, f2 = _write_reads(tmp_path / "r1.fq", r1, True), _write_reads(tmp_path / "r2.fq", r2, True)
    for ss in (True, False):
        d1, d2 = upload(ctx, r1), upload(ctx, r2)
        try:
            table = abundance.quantify(ctx, names, T, d1, d2, ss)
            L = abundance.fragment_bases(d1, d2)
        finally:
            d1.close()
            d2.close()
        want = abundance.abundance_tsv(table)
        out = tmp_path / ("P%d" % ss)
        _run([str(fa), "-o", str(out), "--left", f1, "--right", f2, "--cutoff", "2"] + (["-s"] if ss else []), capsys)
        assert (out / "abundance.tsv").read_bytes() == want.encode()
        assert (out / "filtered.fasta").read_text() == abundance.decide(want, fa.read_text(), 2.0, L)
        assert "pairs: %d of %d mapped" % (table["mapped"], len(r1)) in (out / "quant_log.txt").read_text()
    # mate files of different sizes are refused with a message
    short = _write_reads(tmp_path / "short.fq", r2[:-1], True)
    capsys.readouterr()
    assert quant.main(["quant", str(fa), "-o", str(tmp_path / "P9"), "--left", f1, "--right", short]) == 2
    assert "not mates" in capsys.readouterr().err
