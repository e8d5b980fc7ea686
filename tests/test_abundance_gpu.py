"""GPU: --kallisto_cutoff.  shn_abundance_classes and shn_abundance_em (csrc/abundance.hip) through shannon_amd.abundance against the
brute force of tests/abundance_cases.py (written from the rule): compatibility sets, span histogram and classes are
integers and compared exactly; the EM's alpha to a relative 1e-9 (absolute 1e-12) with the rounds used equal; then the flag through
the command line."""
import hashlib
import json
import os
import numpy as np
import pytest
import abundance_cases as ac
import filter_fp_cases as fc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def upload(ctx, reads):
    """reads of one length as a code matrix (the fixed-length read set), anything else as text + offsets (ragged)"""
    from shannon_amd import device
    if len(set(len(r) for r in reads)) != 1:
        return device.Reads.from_strings(ctx, reads)
    code = np.full(256, 4, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    return device.Reads.from_codes(ctx, code[np.frombuffer("".join(reads).encode(), np.uint8)].reshape(len(reads), len(reads[0])))


def gpu_classes(ctx, T, r1, r2, ss):
    from shannon_amd import abundance
    d1, d2 = upload(ctx, r1), upload(ctx, r2)
    try:
        return abundance.classes(ctx, T, d1, d2, ss)
    finally:
        d1.close()
        d2.close()


def merged(cl):
    """{member tuple: pairs} of an export, classes with the same members added up (a hash collision may have split one)"""
    out = {}
    off = [int(x) for x in cl["class_off"]]
    for c, n in enumerate(cl["n_c"]):
        M = tuple(int(j) for j in cl["members"][off[c]:off[c + 1]])
        assert list(M) == sorted(set(M)) and M, "members of a class ascending, distinct, at least one"
        out[M] = out.get(M, 0) + int(n)
    return out


def check_classes(ctx, T, r1, r2, ss):
    frags = ac.brute_fragments(T, r1, r2, ss)
    want, hist, mapped = ac.brute_classes(frags)
    cl = gpu_classes(ctx, T, r1, r2, ss)
    got = merged(cl)
    print("classes: brute force %s\n         device      %s" % (sorted(want.items())[:12], sorted(got.items())[:12]))
    assert got == want
    assert len(cl["n_c"]) == len(want)                        # equal sets collapse (no 64-bit collision at these sizes)
    assert cl["hist"].tolist() == hist and len(hist) == 501
    assert cl["mapped"] == mapped == int(cl["n_c"].sum()) and cl["fragments"] == len(r1)
    return frags, cl


# ------------------------------------------------------------------------------------------------ compatibility sets + histogram
@pytest.mark.parametrize("ss", [True, False])
def test_isoforms_ties_and_an_internal_repeat(ctx, ss):
    case = fc.isoform_case(ss=ss)
    rng = np.random.Generator(np.random.PCG64(5))
    r1, r2 = case["r1"] + [fc.rand_seq(rng, 100)], case["r2"] + [fc.rand_seq(rng, 100)]          # + a fragment that matches nothing
    frags, cl = check_classes(ctx, case["transcripts"], r1, r2, ss)
    assert frags[-1] == ((), 0, None) and cl["mapped"] == len(r1) - 1
    # ties: a fragment inside the shared exon is compatible with the six isoforms; the fragments inside the repeated segment have
    # several placements on ONE transcript: that transcript once in the set, nothing in the histogram
    assert any(len(C) == 6 for C, _n, _s in frags)
    twice = [f for f in frags if f[0] == (7,) and f[1] > 1]
    assert len(twice) >= 3
    assert int(cl["hist"].sum()) == sum(1 for _C, n, _s in frags if n == 1) < cl["mapped"]


def test_transcript_ends_pair_geometry_and_a_short_transcript(ctx):
    """edge_case: mates over an end or across two transcripts, u > v, span 500 / 501, reads of 14 / 15 bases, a transcript of 10 bases"""
    case = fc.edge_case()
    frags, cl = check_classes(ctx, case["transcripts"], case["r1"], case["r2"], True)
    assert len(case["transcripts"][4]) == 10 and not any(4 in C for C, _n, _s in frags)
    assert cl["hist"][500] >= 2 and sum(1 for C, _n, _s in frags if not C) >= 8
    # ... and a transcript with a base outside ACGT takes part in nothing, whatever else it holds
    T = list(case["transcripts"])
    T.append(T[2][:600] + "N" + T[2][600:])
    frags2, _cl = check_classes(ctx, T, case["r1"], case["r2"], True)
    assert frags2 == frags


def test_reads_with_n(ctx):
    case = fc.n_case()
    frags, _cl = check_classes(ctx, case["transcripts"], case["r1"], case["r2"], True)
    assert any(not C for C, _n, _s in frags) and any(C for C, _n, _s in frags)


def test_mismatch_budget(ctx):
    case = fc.mismatch_case()
    frags, cl = check_classes(ctx, case["transcripts"], case["r1"], case["r2"], True)
    assert any(len(C) == 2 for C, _n, _s in frags)            # (the two transcripts that share their text)
    assert 0 < cl["mapped"] < len(case["r1"])


@pytest.mark.parametrize("ss", [True, False])
def test_ragged_mates(ctx, ss):
    lens = [14, 15, 29, 30, 59, 60, 64, 100, 150, 250]
    case = fc.length_case(lens, lens, n_pairs=120, seed=8)
    r1, r2 = list(case["r1"]), list(case["r2"])
    if not ss:
        for i in range(1, len(r1), 2):                        # the second oriented pair is what places every second fragment
            r1[i], r2[i] = r2[i], r1[i]
    _frags, cl = check_classes(ctx, case["transcripts"], r1, r2, ss)
    assert 0 < cl["mapped"] < 120 and int(cl["hist"].sum()) > 0
    if not ss:
        one = gpu_classes(ctx, case["transcripts"], r1, r2, True)
        assert one["mapped"] < cl["mapped"]


def test_mates_of_two_fixed_lengths(ctx):
    case = fc.length_case(100, 60, seed=5)
    check_classes(ctx, case["transcripts"], case["r1"], case["r2"], True)


# ---------------------------------------------------------------------------------------------------------------- classes
def test_classes_of_1_2_64_and_65_transcripts(ctx):
    T, r1, r2, want = ac.shared_exon_case()
    _frags, cl = check_classes(ctx, T, r1, r2, True)
    off = cl["class_off"].astype(np.int64)
    sizes = {int(off[c + 1] - off[c]): int(cl["n_c"][c]) for c in range(len(cl["n_c"]))}
    assert sizes == want == {65: 5, 64: 4, 2: 3, 1: 6}
    assert cl["mapped"] == len(r1) - 1 and int(cl["n_c"].sum()) == cl["mapped"]
    again = gpu_classes(ctx, T, r1, r2, True)                 # the export is identical across two runs
    for k in ("class_off", "members", "n_c", "hist"):
        assert np.array_equal(cl[k], again[k]) and cl[k].dtype == again[k].dtype
    assert again["mapped"] == cl["mapped"]


@pytest.mark.parametrize("n_tr", [6, 32, 33, 70, 1001])
def test_a_list_that_arrives_unsorted(ctx, n_tr):
    """every pair's placements arrive as the odd transcripts, then the even ones: the list sorted by insertion (up to 32 ids) and
    by heapsort (33 and more) is the brute force's set; one class of all transcripts"""
    T, r1, r2 = ac.interleaved_case(n_tr)
    frags, cl = check_classes(ctx, T, r1, r2, True)
    assert all(f[0] == tuple(range(n_tr)) and f[1] == n_tr for f in frags)      # the case is what it says
    assert cl["members"].tolist() == list(range(n_tr)) and cl["n_c"].tolist() == [3] and cl["mapped"] == 3


def test_nothing_to_map_onto(ctx):
    _T, r1, r2, _want = ac.shared_exon_case()
    cl = gpu_classes(ctx, ["ACGTACGT", "ACGTNACGTACGTACGTACGTACGT"], r1, r2, True)
    assert cl["mapped"] == 0 and len(cl["n_c"]) == 0 and cl["class_off"].tolist() == [0] and int(cl["hist"].sum()) == 0


def test_classes_refuse_bad_arguments(ctx):
    from shannon_amd import abundance, _lib
    T, r1, r2, _want = ac.shared_exon_case()
    d1, d2, d3 = upload(ctx, r1), upload(ctx, r2), upload(ctx, r2[:-1])
    try:
        with pytest.raises(_lib.ShannonError, match="not mates"):
            abundance.classes(ctx, T, d1, d3, True)
        with pytest.raises(_lib.ShannonError, match="max_span"):
            abundance.classes(ctx, T, d1, d2, True, max_span=8192)
    finally:
        for d in (d1, d2, d3):
            d.close()


# ---------------------------------------------------------------------------------------------------------------- EM
@pytest.fixture(scope="module")
def em_reference():
    """the brute force's answer to every hand-made input, computed once"""
    return {name: ac.brute_em(lists, n_c, eff, m) for name, (lists, n_c, eff, m) in ac.em_cases().items()}


def gpu_em(ctx, lists, n_c, eff):
    from shannon_amd import abundance
    off, mem = ac.csr(lists)
    return abundance.em(ctx, off, mem, n_c, eff)


@pytest.mark.parametrize("name", sorted(ac.em_cases()))
def test_em_against_the_brute_force(ctx, em_reference, name):
    lists, n_c, eff, m = ac.em_cases()[name]
    want, rounds, tested = em_reference[name]
    # the stated condition: at no tested round does the largest relative change lie where rounding could move the stop by a block
    assert not any(0.5e-2 <= r <= 2e-2 for r in tested), tested
    assert rounds <= 200
    got, got_rounds = gpu_em(ctx, lists, n_c, eff)
    err = np.abs(got - want)
    nz = want > 0
    print("EM %s: rounds %d (brute force %d), max relative error %.3e, max absolute error %.3e"
          % (name, got_rounds, rounds, float((err[nz] / want[nz]).max()) if nz.any() else 0.0, float(err.max())))
    assert got_rounds == rounds
    assert np.all(err <= ATOL + RTOL * np.abs(want))
    again, again_rounds = gpu_em(ctx, lists, n_c, eff)        # determinism: the same call twice, the same bits
    assert again_rounds == got_rounds and got.tobytes() == again.tobytes()


@pytest.fixture(scope="module")
def em_bits():
    """tests/golden/abundance_em_bits.json: per case and row [label, rounds, SHA-256 of alpha.tobytes()], recorded from abundance.em while
    the single-replicate EM still had kernels of its own (tests/golden/make_abundance_em_golden.py)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abundance_em_bits.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", ac.em_golden_names())
def test_em_and_em_batch_give_the_recorded_bits(ctx, em_bits, name):
    """no tolerance: the one EM there is returns, row by row through em and all rows at once through em_batch (the budget's residency and
    one replicate at a time), the rounds and the bits recorded before the two were one implementation"""
    from shannon_amd import abundance
    lists, matrix, eff, labels = ac.em_golden_case(name)
    off, mem = ac.csr(lists)
    want = em_bits[name]
    assert [w[0] for w in want] == labels

    def rows(alpha, rounds):
        return [[label, int(r), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()] for label, a, r in zip(labels, alpha, rounds)]
    got = [abundance.em(ctx, off, mem, n_c, eff) for n_c in matrix]
    assert all(a.dtype == np.float64 and a.shape == (len(eff),) for a, _ in got)
    assert rows([a for a, _ in got], [r for _, r in got]) == want, "em"
    for max_live in (0, 1):
        alpha, rounds = abundance.em_batch(ctx, off, mem, matrix, eff, max_live=max_live)
        assert alpha.dtype == np.float64 and alpha.shape == (len(matrix), len(eff))
        assert rows(alpha, rounds) == want, "em_batch, max_live %d" % max_live


def test_em_closed_form_and_special_rows(ctx):
    lists, n_c, eff, _m = ac.em_cases()["shared pair"]
    alpha, rounds = gpu_em(ctx, lists, n_c, eff)
    assert rounds == 50 and np.allclose(alpha, [45.0, 15.0], rtol=1e-12, atol=0)         # equal eff: the shared 20 split 30 : 10
    lists, n_c, eff, _m = ac.em_cases()["a transcript in no class"]
    alpha, _rounds = gpu_em(ctx, lists, n_c, eff)
    assert alpha[2] == 0.0 and alpha[3] == 7.0 and abs(alpha.sum() - 62.0) < 1e-9
    # two classes with the same member list (what a hash collision may leave) change nothing but rounding
    a1, r1_ = gpu_em(ctx, [[0, 1], [0], [1]], [20, 30, 10], [200.0, 300.0])
    a2, r2_ = gpu_em(ctx, [[0, 1], [0], [0, 1], [1]], [12, 30, 8, 10], [200.0, 300.0])
    assert r1_ == r2_ and np.allclose(a1, a2, rtol=1e-12, atol=0)
    # no class at all: everything ends at 0 after the first test
    a0, r0 = gpu_em(ctx, [], [], [100.0, 50.0])
    assert a0.tolist() == [0.0, 0.0] and r0 == 50


def test_em_refuses_bad_arguments(ctx):
    from shannon_amd import abundance, _lib
    ok = dict(class_off=[0, 2, 3], members=[0, 1, 1], n_c=[5, 2], eff=[100.0, 50.0])

    def call(**kw):
        a = dict(ok, **kw)
        return abundance.em(ctx, np.array(a["class_off"], np.uint64), np.array(a["members"], np.uint32), np.array(a["n_c"], np.uint64),
                            np.array(a["eff"], np.float64))
    assert call()[1] % 50 == 0
    with pytest.raises(_lib.ShannonError, match="not monotone"):
        call(class_off=[0, 3, 2], members=[0, 1, 1])
    with pytest.raises(_lib.ShannonError, match="class_off\\[0\\]"):
        call(class_off=[1, 2, 3])
    with pytest.raises(_lib.ShannonError, match="names transcript 2 of 2"):
        call(members=[0, 2, 1])
    with pytest.raises(_lib.ShannonError, match="not above 0"):
        call(eff=[100.0, 0.0])
    with pytest.raises(_lib.ShannonError, match="not above 0"):
        call(eff=[-1.0, 50.0])
    with pytest.raises(_lib.ShannonError, match="not above 0"):
        call(eff=[float("nan"), 50.0])
    with pytest.raises(_lib.ShannonError, match="m is 0"):
        abundance.em(ctx, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.float64))
    with pytest.raises(ValueError):
        call(n_c=[5])
    with pytest.raises(ValueError):
        call(class_off=[0, 2, 4])


def test_quantify_against_the_brute_force(ctx):
    """classes, effective lengths and EM together on synth's pairs: the table the decision reads"""
    from shannon_amd import abundance
    T, names, r1, r2 = fc.planted_case(n_pairs=600)
    T, names = T + ["ACGTNACGTACGTACGTACGT" * 3], names + ["withN"]
    B = ac.brute_table(T, r1, r2, True)
    assert not any(0.5e-2 <= r <= 2e-2 for r in B["tested"]) and B["rounds"] <= 200, B["tested"]
    d1, d2 = upload(ctx, r1), upload(ctx, r2)
    try:
        t = abundance.quantify(ctx, names, T, d1, d2, True)
        assert abundance.fragment_bases(d1, d2) == B["L"] == 200.0
    finally:
        d1.close()
        d2.close()
    assert t["names"] == names and t["length"] == [len(s) for s in T]
    assert t["eff_length"] == B["eff"].tolist() and t["mapped"] == B["mapped"] and t["classes"] == len(B["classes"]) and t["rounds"] == B["rounds"]
    got = np.array(t["est_counts"])
    assert np.all(np.abs(got - B["alpha"]) <= ATOL + RTOL * B["alpha"])
    assert got[names.index("short40")] == 0.0 and got[names.index("withN")] == 0.0 and t["tpm"][names.index("withN")] == 0.0
    assert abs(sum(t["tpm"]) - 1e6) < 1e-3 and abs(got.sum() - t["mapped"]) < 1e-6
    rows = abundance.abundance_tsv(t).splitlines()[1:]
    assert [float(r.split("\t")[3]) for r in rows] == t["est_counts"] and [float(r.split("\t")[2]) for r in rows] == t["eff_length"]


# ---------------------------------------------------------------------------------------------------------------- end to end
def _run_cli(argv, capsys):
    """shannon.main in this process (one device context per run, closed at its end); returns what it printed"""
    import shannon
    capsys.readouterr()
    rc = shannon.main(["shannon.py"] + argv)
    out = capsys.readouterr().out
    assert rc == 0, out
    return out


def _records(text):
    lines = text.splitlines()
    assert len(lines) % 2 == 0 and all(l.startswith(">") for l in lines[0::2])
    return [l[1:] for l in lines[0::2]], lines[1::2]


def test_cli_drops_the_barely_expressed_transcript(ctx, tmp_path, capsys, monkeypatch):
    """synth's isoforms with 3,000 pairs + a spurious transcript that 14 pairs cover four deep (fully covered: --filter_FP would keep
    it): with FASTQ input `--kallisto_cutoff 10` removes it and nothing else; with FASTA input the flag changes nothing"""
    from shannon_amd import abundance
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    C = 10.0
    _T, S, r1, r2 = ac.spurious_case()
    files = {}
    for ext in ("fastq", "fasta"):
        for k, reads in enumerate((r1, r2)):
            p = tmp_path / ("r%d.%s" % (k + 1, ext))
            p.write_text("".join(("@%d\n%s\n+\n%s\n" % (i, s, "I" * len(s))) if ext == "fastq" else (">%d\n%s\n" % (i, s)) for i, s in enumerate(reads)))
            files[ext, k] = str(p)
    base = ["-s", "-K", "25"]
    out = tmp_path / "OUTK"
    printed = _run_cli(["-o", str(out), "--left", files["fastq", 0], "--right", files["fastq", 1], "--kallisto_cutoff", "10"] + base, capsys)
    assert "OPTIONS --kallisto_cutoff: Kallisto will be run to filter low expression transcripts below 10.0" in printed
    assert "ignored" not in printed
    alld = out / "TEMP" / "OUTK_allalgo_output"
    before, tsv, final = (alld / "rec_before_kallisto.fasta").read_text(), (alld / "kallisto" / "abundance.tsv").read_text(), (out / "shannon.fasta").read_text()
    assert tsv.startswith("target_id\tlength\teff_length\test_counts\ttpm\n")
    assert final == abundance.decide(tsv, before, C, 200.0)
    log = [l for l in (out / "log.txt").read_text().splitlines() if "--kallisto_cutoff" in l]
    names, seqs = _records(before)
    kept_names, kept_seqs = _records(final)
    assert len(log) == 1 and "fragments mapped" in log[0] and "EM rounds" in log[0] and "%d of %d transcripts kept" % (len(kept_names), len(names)) in log[0]
    assert [l.split("\t")[0] for l in tsv.splitlines()[1:]] == names
    # the spurious transcript was assembled, and it is the one that goes
    kmers = {S[i:i + 25] for i in range(len(S) - 24)}
    spurious = [n for n, s in zip(names, seqs) if any(s[i:i + 25] in kmers for i in range(len(s) - 24))]
    assert len(spurious) == 1 and len(names) >= 4
    assert kept_names == [n for n in names if n not in spurious] and kept_seqs == [s for n, s in zip(names, seqs) if n not in spurious]
    # the brute force on the same transcripts: no cov near the cutoff (rounding cannot flip a decision), the same decisions, the same table
    B = ac.brute_table(seqs, r1, r2, True)
    print("cov: %s" % {n: round(float(c), 3) for n, c in zip(names, B["cov"])})
    assert all(c < C * (1 - 1e-3) or c > C * (1 + 1e-3) for c in B["cov"])
    assert [n for n, c in zip(names, B["cov"]) if c >= C] == kept_names
    assert not any(0.5e-2 <= r <= 2e-2 for r in B["tested"])
    rows = [l.split("\t") for l in tsv.splitlines()[1:]]
    assert [float(r[2]) for r in rows] == B["eff"].tolist()
    assert np.all(np.abs(np.array([float(r[3]) for r in rows]) - B["alpha"]) <= ATOL + RTOL * B["alpha"])
    # FASTA copies of the same reads: the reference's gate leaves the flag off -- byte for byte the run without it, no kallisto/
    # (record names carry the sample, the output directory's base name: both runs write to an "OUTA")
    with_flag, without = tmp_path / "flag" / "OUTA", tmp_path / "noflag" / "OUTA"
    printed = _run_cli(["-o", str(with_flag), "--left", files["fasta", 0], "--right", files["fasta", 1], "--kallisto_cutoff", "10"] + base, capsys)
    assert "OPTIONS WARNING: --kallisto_cutoff NOT enabled. Option only works with fastq input." in printed
    assert "ignored: --kallisto_cutoff" in printed
    _run_cli(["-o", str(without), "--left", files["fasta", 0], "--right", files["fasta", 1]] + base, capsys)
    assert (with_flag / "shannon.fasta").read_bytes() == (without / "shannon.fasta").read_bytes()
    assert sorted(os.listdir(with_flag / "TEMP" / "OUTA_allalgo_output")) == sorted(os.listdir(without / "TEMP" / "OUTA_allalgo_output")) == ["all_reconstructed.fasta"]
    # ... which is what the FASTQ run held before the filter (the names carry the sample: compare the sequences)
    assert _records((without / "shannon.fasta").read_text())[1] == seqs


def test_pipeline_argument(ctx):
    """assemble(kallisto_cutoff=C): R.final filtered, R.final_before_kallisto, R.abundance, timings["abundance"]; None: nothing runs;
    together with filter_fp; single-end: a note"""
    from shannon_amd import abundance, pipeline
    _T, _S, r1, r2 = ac.spurious_case()
    kw = dict(K=25, sample="s", seed=0, double_stranded=False)
    plain = pipeline.assemble(ctx, r1, r2, **kw)
    off = pipeline.assemble(ctx, r1, r2, kallisto_cutoff=None, **kw)
    R = pipeline.assemble(ctx, r1, r2, kallisto_cutoff=10.0, **kw)
    assert dict(off.final) == dict(plain.final) and "abundance" not in off.timings and not hasattr(off, "abundance")
    assert dict(R.final_before_kallisto) == dict(plain.final) and "abundance" in R.timings
    before = "".join(">%s\n%s\n" % kv for kv in plain.final.items())
    assert R.abundance["before"] == before and R.abundance["L"] == 200.0
    assert "".join(">%s\n%s\n" % kv for kv in R.final.items()) == abundance.decide(R.abundance["tsv"], before, 10.0, 200.0)
    assert len(R.final) == len(plain.final) - 1 == R.abundance["kept"]
    both = pipeline.assemble(ctx, r1, r2, kallisto_cutoff=10.0, filter_fp=True, **kw)
    assert "filter_FP" in both.timings and "abundance" in both.timings and len(both.final) <= len(both.final_before_kallisto)
    se = pipeline.assemble(ctx, r1, None, kallisto_cutoff=10.0, **kw)
    assert "single-end" in se.kallisto_note and not hasattr(se, "abundance") and "abundance" not in se.timings
