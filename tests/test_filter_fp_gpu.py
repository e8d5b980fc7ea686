"""GPU: --filter_FP.  shn_filter_fp_hits (csrc/filter_fp.hip) through filter_fp.coverage_hits against the brute force of
tests/filter_fp_cases.py (written from the rule, DESIGN.md "filter_FP") -- hits are integers, every comparison is exact --, then
the flag through the pipeline, the reference's entry point and the command line."""
import os, subprocess, sys
import numpy as np
import pytest
from golden_util import *
import filter_fp_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def upload(ctx, reads, as_strings=False):
    """reads of one length as a code matrix (the fixed-length read set), anything else -- or as_strings -- as text + offsets (ragged)"""
    from shannon_amd import device
    if as_strings or len(set(len(r) for r in reads)) != 1:
        return device.Reads.from_strings(ctx, reads)
    code = np.full(256, 4, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    return device.Reads.from_codes(ctx, code[np.frombuffer("".join(reads).encode(), np.uint8)].reshape(len(reads), len(reads[0])))


def gpu_hits(ctx, case, as_strings=False, stats=None):
    from shannon_amd import filter_fp
    d1, d2 = upload(ctx, case["r1"], as_strings), upload(ctx, case["r2"], as_strings)
    try:
        return filter_fp.coverage_hits(ctx, case["transcripts"], case["part_of"], case["n_parts"], d1, d2, case["routes"], case["ss"],
                                       stats=stats).tolist()
    finally:
        d1.close()
        d2.close()


def check(ctx, case, **kw):
    want = fc.brute_hits(case)
    got = gpu_hits(ctx, case, **kw)
    print("hits: brute force %s\n      device      %s" % (want, got))
    assert got == want
    return want


@pytest.mark.parametrize("ss", [True, False])
def test_synthetic_pairs(ctx, ss):
    """300 of synth's pairs at L = 100 with 0.5 % errors on 13 isoforms in two partitions; not strand-specific: the mates of every
    second fragment swapped, so the second oriented pair is what places them"""
    case = fc.synth_case(ss)
    want, placed = fc.brute_hits(case, want_placed=True)
    st = {}
    assert gpu_hits(ctx, case, stats=st) == want
    assert st == {"routes": 600, "placed": placed} and placed >= 290
    assert sum(want) > 0.5 * sum(len(t) for t in case["transcripts"])
    if not ss:                                                # the swapped half is not found by the first oriented pair alone
        one = dict(case, ss=True, routes=(case["routes"][0], case["routes"][1] % 300))
        assert sum(fc.brute_hits(one)) < sum(want) and gpu_hits(ctx, one) == fc.brute_hits(one)


@pytest.mark.parametrize("L", [30, 59, 60, 64, 100, 150, 250])
def test_read_lengths(ctx, L):
    case = fc.length_case(L, L, seed=100 + L)
    want = check(ctx, case)
    assert sum(want) > 0
    assert gpu_hits(ctx, case, as_strings=True) == want          # the same reads as a ragged set


def test_mates_of_two_lengths_and_ragged_reads(ctx):
    check(ctx, fc.length_case(100, 60, seed=5))
    check(ctx, fc.length_case(64, 150, seed=6))
    lens = [14, 15, 29, 30, 59, 60, 64, 100, 150, 250]
    case = fc.length_case(lens, lens, n_pairs=120, seed=8)
    assert {len(r) for r in case["r1"] + case["r2"]} == set(lens)
    want, placed = fc.brute_hits(case, want_placed=True)
    assert gpu_hits(ctx, case) == want and 0 < placed < 120      # (the pairs with a 14-base mate never place)


def test_mismatch_budget_and_seeds(ctx):
    """exactly L // 30 mismatches with every seed but one hit: placed; L // 30 + 1 with a clean seed left, or with every seed hit: not"""
    case = fc.mismatch_case()
    want = check(ctx, case)
    assert 0 in want and max(want) > 0


def test_reads_with_n(ctx):
    case = fc.n_case()
    want = check(ctx, case)
    assert 0 in want and max(want) > 0
    # ... and in a set of one read length (the fixed-length layout's mask): an N in every third read of synth's pairs
    c2 = fc.synth_case(True, n_pairs=150, seed=9)
    for i in range(0, 150, 3):
        for r in (c2["r1"], c2["r2"]):
            s = list(r[i])
            for p in range(i % 4 + (r is c2["r2"])):
                s[(17 * i + 31 * p) % 100] = "N"
            r[i] = "".join(s)
    assert any("N" in r for r in c2["r1"]) and len({len(r) for r in c2["r1"]}) == 1
    check(ctx, c2)


def test_transcript_ends_and_pair_geometry(ctx):
    """a mate hanging over either end by one base or lying across two transcripts: never placed; u > v, a first mate that ends
    behind the second, span 501: not concordant; span 500, mates flush with the ends: placed; reads of 14 / 15 bases"""
    case = fc.edge_case()
    want = check(ctx, case)
    assert want == [400, 0, 500, 60, 0, 200]


def test_isoforms_ties_and_an_internal_repeat(ctx):
    for ss in (True, False):
        case = fc.isoform_case(ss=ss)
        want = check(ctx, case)
        assert want[0] == want[1] == 320 and want[6] == 320 and want[7] > 400


def test_partitions_are_kept_apart(ctx):
    """the same transcript in two partitions, fragments routed to one: the other's hits stay 0; a partition without transcripts;
    a partition without routes; a fragment routed twice"""
    case = fc.partition_case()
    want = check(ctx, case)
    assert want[0] > 0 and want[1] > 0 and want[2] == 0 and want[3] == 0
    # nothing to map onto, nothing to map
    from shannon_amd import filter_fp
    d1, d2 = upload(ctx, case["r1"]), upload(ctx, case["r2"])
    try:
        assert filter_fp.coverage_hits(ctx, [], [], 3, d1, d2, case["routes"], True).tolist() == []
        none = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        assert filter_fp.coverage_hits(ctx, case["transcripts"], case["part_of"], 4, d1, d2, none, True).tolist() == [0, 0, 0, 0]
    finally:
        d1.close()
        d2.close()


def test_bad_arguments_are_refused(ctx):
    from shannon_amd import filter_fp, _lib
    case = fc.partition_case()
    d1, d2 = upload(ctx, case["r1"]), upload(ctx, case["r2"])
    try:
        with pytest.raises(_lib.ShannonError, match="outside ACGT"):
            filter_fp.coverage_hits(ctx, ["ACGTACGTACGTACGTNACGT"], [0], 1, d1, d2, ([0], [0]), True)
        with pytest.raises(_lib.ShannonError, match="does not exist"):
            filter_fp.coverage_hits(ctx, case["transcripts"], case["part_of"], 4, d1, d2, ([0], [len(case["r1"])]), True)
        with pytest.raises(_lib.ShannonError, match="out of range"):
            filter_fp.coverage_hits(ctx, case["transcripts"], case["part_of"], 3, d1, d2, case["routes"], True)
    finally:
        d1.close()
        d2.close()


def _routed(ctx, r1, r2, ss):
    """count, extension, partitions and routing of a small input: (device reads, routing result)"""
    from shannon_amd import device, extension_correction as ec, kmers_for_component as kfc
    d1, d2 = device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2)
    t = device.count_k1mers_strand_specific(ctx, d1, d2, 26) if ss else device.count_k1mers(ctx, [d1, d2], 26, True)
    try:
        res = ec.run_correction(ctx, t, 3, 75, 500, want_allowed=False)
        part = kfc.kmers_for_component(ctx, res, d1, d2, 25, 500, want_rows=False, lazy_routes=True, strand_specific=ss)
    finally:
        t.close()
    return d1, d2, part


@pytest.mark.parametrize("ss", [True, False])
def test_routes_on_the_device_and_on_the_host(ctx, ss):
    """the routes of a real routing call as they lie on the device, and the same list downloaded and handed over from the host:
    the same hits -- and the brute force's on a part of them"""
    from shannon_amd import filter_fp, synth
    (r1, r2), iso = synth.make_dataset(4000, 6, seed=4, sigma=0.5)
    d1, d2, part = _routed(ctx, r1, r2, ss)
    try:
        routes, _starts = part["routes_dev"]
        names = list(part["new_components"])
        pid, ridx = routes.download()
        assert len(pid) > 1000 and len(names) >= 1
        T = synth.codes_to_strings(iso)
        seqs, part_of = T * len(names), [p for p in range(len(names)) for _ in T]          # every isoform offered to every partition
        dev = filter_fp.coverage_hits(ctx, seqs, part_of, len(names), d1, d2, routes, ss).tolist()
        host = filter_fp.coverage_hits(ctx, seqs, part_of, len(names), d1, d2, (pid, ridx), ss).tolist()
        assert dev == host and sum(dev) > 0
        sub = np.arange(0, len(pid), max(1, len(pid) // 300))
        case = fc.make_case(seqs, part_of, len(names), synth.codes_to_strings(r1), synth.codes_to_strings(r2), (pid[sub], ridx[sub]), ss)
        assert filter_fp.coverage_hits(ctx, seqs, part_of, len(names), d1, d2, case["routes"], ss).tolist() == fc.brute_hits(case)
    finally:
        d1.close()
        d2.close()


@pytest.mark.parametrize("name", ["syn_pe_ss_s69", "syn_pe_s0"])
def test_pipeline_with_the_filter(ctx, name):
    """assemble_resident(filter_fp=True): per partition the kept names are the brute force's on that partition's unfiltered text and
    routed fragments; R.final is the merge of single contigs + filtered texts; filter_fp=False returns what it returns without the
    argument"""
    from shannon_amd import device, pipeline, post, kmers_for_component as kfc
    m = MANIFEST[name]
    inp = load_inputs(name)
    ss = strand_specific(name)

    def run(**kw):
        d1, d2 = device.Reads.from_strings(ctx, inp[0]), device.Reads.from_strings(ctx, inp[1])
        try:
            return pipeline.assemble_resident(ctx, d1, d2, kfc.ReadStore(inp[0], inp[1]), K=m["K"], partition_size=m.get("partition_size", 500),
                                              sample="s", seed=m["sf_seed"], double_stranded=not ss, keep_partitioning=True, **kw)
        finally:
            d1.close()
            d2.close()
    plain, off, R = run(), run(filter_fp=False), run(filter_fp=True)
    assert dict(off.final) == dict(plain.final) and list(off.partitions) == list(plain.partitions)
    for p in plain.partitions:
        assert off.partitions[p]["reconstructed_fasta"] == plain.partitions[p]["reconstructed_fasta"]
        assert "filter_log" not in off.partitions[p] and "reconstructed_org_fasta" not in off.partitions[p]
    assert "filter_FP" in R.timings and "filter_FP" not in off.timings
    assert list(R.partitions) == list(plain.partitions)
    texts, dropped = [], 0
    for p, rec in R.partitions.items():
        org = plain.partitions[p]["reconstructed_fasta"]
        assert rec["reconstructed_org_fasta"] == org
        heads = [l for l in org.splitlines() if l.startswith(">")]
        seqs = [l for l in org.splitlines() if not l.startswith(">")]
        idx = np.asarray(R.partitioning["routes"][p], dtype=np.uint32)
        assert len(idx) == rec["n_reads_routed"]
        case = fc.make_case(seqs, [0] * len(seqs), 1, inp[0], inp[1], (np.zeros(len(idx), np.uint32), idx), ss)
        hits = fc.brute_hits(case)
        keep = fc.keep(hits, [len(s) for s in seqs])
        names = [h.split()[0][1:] for h in heads]
        assert rec["filter_log"] == "".join("%s\t%d\t%d\n" % (n, h, len(s)) for n, h, s in zip(names, hits, seqs))
        assert rec["reconstructed_fasta"] == "".join(">%s\n%s\n" % (n, s) for n, s, k in zip(names, seqs, keep) if k)
        dropped += len(keep) - sum(keep)
        assert sum(keep) > 0
        texts.append(rec["reconstructed_fasta"])
    assert dropped > 0                                        # (at the least the header record `Bases` of the single nodes)
    single = "".join(">Single_%d\n%s\n" % (i, c) for i, c in enumerate(R.extension.single_contigs))
    assert "".join(R.all_reconstructed) == single + "".join(texts)
    assert dict(R.final) == dict(post.finalize((single + "".join(texts)).splitlines(True), not ss))
    assert R.filter_fp_stats["transcripts"] == R.filter_fp_stats["kept"] + dropped and 0 < R.filter_fp_stats["placed"] <= R.filter_fp_stats["routes"]


def test_single_end_input_is_not_filtered(ctx):
    from shannon_amd import pipeline
    inp = load_inputs("syn_se_s5")
    m = MANIFEST["syn_se_s5"]
    kw = dict(K=m["K"], partition_size=m.get("partition_size", 500), sample="s", seed=m["sf_seed"])
    a = pipeline.assemble(ctx, inp[0], None, **kw)
    b = pipeline.assemble(ctx, inp[0], None, filter_fp=True, **kw)
    assert dict(a.final) == dict(b.final) and "single-end" in b.filter_fp_note
    assert all("filter_log" not in rec for rec in b.partitions.values())


def test_reference_entry_point_on_a_planted_case(ctx, tmp_path):
    """reference_api.filter_FP on files: the true isoforms and isoform 0 with a random tail of 8 % of the new length are kept, the
    one with 15 % and a 40-base transcript are dropped; the three files have the reference's format (filter_FP.py:22-25, 52-55)"""
    from shannon_amd import reference_api
    T, names, r1, r2 = fc.planted_case()
    # (a condition on the INPUT, confirmed with the brute force on all 3,000 pairs: 2,994 place, the true isoforms are covered to
    # 99.3-99.9 %, the 8 % tail leaves 0.917, the 15 % tail 0.848)
    rec = tmp_path / "reconstructed.fasta"
    text = "".join(">%s extra\tw=1.5\n%s\n" % (n, t) for n, t in zip(names, T))
    rec.write_text(text)
    f1, f2 = tmp_path / "reads_1.fasta", tmp_path / "reads_2.fasta"
    f1.write_text("".join(">%d\n%s\n" % (i, s) for i, s in enumerate(r1)))
    f2.write_text("".join(">%d\n%s\n" % (i, fc.rc(s)) for i, s in enumerate(r2)))          # as shannon.py:407-411 leaves reads_2: RC'd
    out = tmp_path / "algo_output"
    out.mkdir()
    reference_api.filter_FP(str(rec), str(f1), str(f2), str(out), ctx=ctx)
    assert sorted(os.listdir(out)) == ["rec.log", "reconstructed.fasta", "reconstructed_org.fasta"]
    assert (out / "reconstructed_org.fasta").read_text() == text
    log = [l.split("\t") for l in (out / "rec.log").read_text().splitlines()]
    assert [l[0] for l in log] == names and [int(l[2]) for l in log] == [len(t) for t in T]
    frac = {l[0]: int(l[1]) / int(l[2]) for l in log}
    print("covered fractions:", {k: round(v, 4) for k, v in frac.items()})
    kept = (out / "reconstructed.fasta").read_text()
    kept_names = [l[1:] for l in kept.splitlines() if l.startswith(">")]
    assert kept_names == [n for n in names if n not in ("tail15", "short40")]
    assert kept == "".join(">%s\n%s\n" % (n, t) for n, t in zip(names, T) if n in kept_names)
    assert all(frac[n] >= 0.9 for n in names if n.startswith("iso")) and frac["tail8"] >= 0.9 > frac["tail15"] and frac["short40"] == 0
    # the hits of the log are the brute force's on a tenth of the pairs (all of them: 19 s)
    sub = list(range(0, len(r1), 10))
    s1, s2 = tmp_path / "s1.fasta", tmp_path / "s2.fastq"
    s1.write_text("".join(">%d\n%s\n" % (i, r1[i]) for i in sub))
    s2.write_text("".join("@%d\n%s\n+\n%s\n" % (i, r2[i], "I" * len(r2[i])) for i in sub))   # second mates as sequenced, FASTQ: --fr
    out2 = tmp_path / "fr"
    out2.mkdir()
    reference_api.filter_FP(str(rec), str(s1), str(s2), str(out2), flags="-q --fr", ctx=ctx)
    case = fc.make_case(T, [0] * len(T), 1, [r1[i] for i in sub], [r2[i] for i in sub], (np.zeros(len(sub), np.uint32), np.arange(len(sub))), True)
    assert [int(l.split("\t")[1]) for l in (out2 / "rec.log").read_text().splitlines()] == fc.brute_hits(case)


def test_cli_writes_the_three_files(ctx, tmp_path):
    """shannon.py --left --right -s --filter_FP on a small synthetic input: per partition reconstructed.fasta (filtered),
    reconstructed_org.fasta and rec.log; shannon.fasta equal to the pipeline call's"""
    from conftest import ROOT
    from shannon_amd import pipeline, synth
    (r1, r2), _iso = synth.make_dataset(6000, 5, seed=12, sigma=0.5)
    files = []
    for k, m in enumerate((r1, r2)):
        fa = tmp_path / ("r%d.fasta" % (k + 1))
        synth.write_fasta(str(fa), m)
        files.append(str(fa))
    out = tmp_path / "OUTF"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", str(out), "--left", files[0], "--right", files[1], "-s", "-K", "25",
                        "--filter_FP"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "OPTIONS --filter_FP: False-positive filtering enabled" in p.stdout and "ignored" not in p.stdout
    assert "--filter_FP:" in (out / "log.txt").read_text()
    R = pipeline.assemble(ctx, r1, r2, K=25, sample="OUTF", seed=0, double_stranded=False, filter_fp=True)
    assert len(R.partitions) > 0
    for name, rec in R.partitions.items():
        d = out / "TEMP" / ("OUTF_%salgo_output" % name)
        assert (d / "reconstructed.fasta").read_text() == rec["reconstructed_fasta"]
        assert (d / "reconstructed_org.fasta").read_text() == rec["reconstructed_org_fasta"]
        assert (d / "rec.log").read_text() == rec["filter_log"]
        assert rec["reconstructed_fasta"].count(">") < rec["reconstructed_org_fasta"].count(">")
    got = dict((h[1:], s) for h, s in parse_fasta((out / "shannon.fasta").read_text()))
    assert got == dict(R.final) and len(got) > 0
