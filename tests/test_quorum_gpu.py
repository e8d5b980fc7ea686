"""GPU: --quorum.  shn_reads_quality_mask, shn_quorum_table and shn_quorum_correct (csrc/ingest.hip, csrc/quorum.hip) through
shannon_amd.quorum against the brute force of tests/quorum_cases.py (written from the rule); then the flag through
the command line.  Bases, counts and counters are integers: every comparison is exact."""
import re
import numpy as np
import pytest
import quorum_cases as qc

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def strings_of(host):
    """the host codes of a read set (matrix or RaggedCodes) as strings over ACGTN"""
    return [LETTERS[np.minimum(np.asarray(host[i]), 4)].tobytes().decode() for i in range(len(host))]


def resident_strings(d):
    from shannon_amd import quorum
    return strings_of(quorum.host_codes(d))


class Ingested(object):
    """the files of a case as FASTQ text through the device ingest: sets, host codes, texts"""

    def __init__(self, ctx, files):
        from shannon_amd import device
        self.texts = [qc.fastq_text(reads).encode() for reads in files]
        got = [device.Reads.ingest(ctx, t) for t in self.texts]
        self.sets, self.host = [g[0] for g in got], [g[1] for g in got]

    def close(self):
        for d in self.sets:
            d.close()


def key_str(key, k):
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def gpu_table(ctx, files, k=qc.K, q=qc.Q):
    """{canonical k-mer: count} and the number of windows, from the device"""
    from shannon_amd import quorum
    I = Ingested(ctx, files)
    masks = [quorum.hq_mask(ctx, d, t, q) for d, t in zip(I.sets, I.texts)]
    try:
        t = quorum.trusted_table(ctx, I.sets, masks, k)
        try:
            keys, cnts = t.download()
            assert t.k == k and t.canonical and len(t) == len(keys)
            return {key_str(x, k): int(c) for x, c in zip(keys, cnts)}, t.total
        finally:
            t.close()
    finally:
        for m in masks:
            m.close()
        I.close()


def gpu_apply(ctx, files, **kw):
    """(corrected files as strings, stats, the originals read back from the device afterwards)"""
    from shannon_amd import quorum
    I = Ingested(ctx, files)
    try:
        sets, codes, stats = quorum.apply(ctx, I.sets, I.texts, host=I.host, **kw)
        try:
            assert [len(s) for s in sets] == [len(s) for s in I.sets]
            from_host = [strings_of(c) for c in codes]
            assert [type(c) for c in codes] == [type(h) for h in I.host]
            assert from_host == [resident_strings(s) for s in sets]
            return from_host, stats, [resident_strings(d) for d in I.sets]
        finally:
            for s in sets:
                s.close()
    finally:
        I.close()


def check_apply(ctx, files, **kw):
    names = {"k": "k", "min_quality": "q", "anchor_count": "a", "window": "w", "max_subs": "e"}
    want, wstats, _table = qc.brute_apply(files, **{names[n]: v for n, v in kw.items()})
    got, stats, originals = gpu_apply(ctx, files, **kw)
    print("brute force %s\ndevice      %s" % (wstats, {n: stats[n] for n in wstats}))
    for f in range(len(files)):
        assert len(got[f]) == len(want[f])
        bad = [i for i in range(len(want[f])) if got[f][i] != want[f][i]]
        assert not bad, (f, bad[:5], [(files[f][i][0], want[f][i], got[f][i]) for i in bad[:2]])
    assert {n: stats[n] for n in wstats} == wstats
    # the originals are still resident and what they were
    assert originals == [[qc.norm(b) for b, _q in reads] for reads in files]
    return want, wstats


# ---------------------------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("ragged", [False, True])
def test_hq_mask_bits(ctx, ragged):
    """one bit per base in the layout of the set's own mask: 64 bases per word, first base in the highest bit, every read on a word of its own"""
    import random
    from shannon_amd import quorum
    rng = random.Random(3)
    lens = [1, 23, 63, 64, 65, 128, 129, 200] if ragged else [70] * 9
    reads = []
    for L in lens:
        b = "".join(rng.choice("ACGTacgtNR") for _ in range(L))
        reads.append((b, "".join(rng.choice("!%&'I#5") for _ in range(L))))
    I = Ingested(ctx, [reads])
    try:
        for q in (5, 20):
            m = quorum.hq_mask(ctx, I.sets[0], I.texts[0], q)
            words = m.download()
            want, n_hq = [], 0
            for b, ql in reads:
                bits = qc.hq_bits(b, ql, q)
                n_hq += sum(bits)
                for j0 in range(0, max(len(bits), 1), 64):
                    w = 0
                    for j, bit in enumerate(bits[j0:j0 + 64]):
                        w |= int(bit) << (63 - j)
                    want.append(w)
            assert [int(w) for w in words] == want and m.n_hq == n_hq
            m.close()
    finally:
        I.close()


# ---------------------------------------------------------------------------------------------------------------- the table
def table_reads(k):
    """(reads, facts): a low-quality base inside a window, a k-mer seen on the opposite strand only, a palindromic k-mer (even k), an
    N, reads of the lengths around the word boundaries"""
    import random
    rng = random.Random(100 + k)
    X, Y, Z = qc.rand_seq(rng, 70), qc.rand_seq(rng, 70), qc.rand_seq(rng, 66)
    half = qc.rand_seq(rng, k // 2)
    pal = half + qc.revcomp(half)                                       # (its own reverse complement when k is even)
    reads = [(X, "I" * 70), (qc.revcomp(X)[3:60], "I" * 57)]            # the second read: X's k-mers from the other strand
    low = list("I" * 70)
    low[k - 1] = "$"                                                    # quality 3: every window over base k - 1 is out
    reads.append((Y, "".join(low)))
    flank1, flank2 = qc.rand_seq(rng, 7), qc.rand_seq(rng, 9)
    reads.append((flank1 + pal + flank2, "I" * (len(pal) + 16)))
    n = list(Z)
    n[33] = "N"
    reads.append(("".join(n), "I" * 66))
    W = qc.rand_seq(rng, 80)
    for L in (23, 24, 25, 31, 32, 33, 64, 65):
        reads.append((W[5:5 + L], "I" * L))
    reads.append((W[:65].lower(), "&" * 65))                            # lower case, the lowest quality that still counts
    reads.append((W[:65], "%" * 65))                                    # one below it: nothing
    return reads, {"X": X, "Y": Y, "pal": pal, "Z": Z}


@pytest.mark.parametrize("k", [15, 24, 32])
def test_table_equals_brute_force(ctx, k):
    reads, F = table_reads(k)
    want = qc.brute_table([reads], k=k)
    # the input is what it is meant to be
    X, Y, Z, pal = F["X"], F["Y"], F["Z"], F["pal"]
    assert want[qc.can(X[10:10 + k])] == 2                              # once from X, once from the opposite strand
    assert want[qc.can(X[0:k])] == 1                                    # (the second read starts 10 bases into X's other end)
    assert all(qc.can(Y[i:i + k]) not in want for i in range(0, k))     # the windows over the low-quality base
    assert want[qc.can(Y[k:2 * k])] == 1
    if k % 2 == 0:
        assert qc.revcomp(pal) == pal and want[pal] == 1                # a palindrome counts once per window
    assert all(qc.can(Z[i:i + k]) not in want for i in range(max(0, 34 - k), 34)) and qc.can(Z[34:34 + k]) in want
    got, total = gpu_table(ctx, [reads], k=k)
    assert got == want and total == sum(want.values())


def test_table_over_two_files_and_another_quality(ctx):
    case = qc.scenario("mates_two_lengths")
    for q in (5, 3, 41):
        want = qc.brute_table(case["files"], q=q)
        got, total = gpu_table(ctx, case["files"], q=q)
        assert got == want and total == sum(want.values())
    assert not qc.brute_table(case["files"], q=41)                      # (I is 40: nothing is high quality, the table is empty)


# ---------------------------------------------------------------------------------------------------------------- the correction
@pytest.mark.parametrize("name", qc.SCENARIOS)
def test_correction_equals_brute_force(ctx, name):
    """one situation of the rule each (tests/test_quorum.py holds every input against its name on the CPU)"""
    case = qc.scenario(name)
    want, stats = check_apply(ctx, case["files"])
    f, i = case["probe"]
    if name == "n_base":
        # the N became a base, its mask bit is gone: the corrected set holds no base outside ACGT
        from shannon_amd import quorum
        I = Ingested(ctx, case["files"])
        try:
            sets, _codes, _st = quorum.apply(ctx, I.sets, I.texts, host=I.host)
            assert I.sets[0].n_invalid == 1 and sets[0].n_invalid == 0 and want[f][i] == case["clean"]
            sets[0].close()
        finally:
            I.close()


@pytest.mark.parametrize("kw", [dict(k=15), dict(k=32, anchor_count=2), dict(window=3, max_subs=2), dict(max_subs=0), dict(max_subs=4, window=40),
                                dict(min_quality=1)])
def test_other_parameters(ctx, kw):
    files = [qc.scenario("fourth_forward")["files"][0] + qc.scenario("fourth_backward")["files"][0] + qc.scenario("lookahead_settles")["files"][0]]
    check_apply(ctx, files, **kw)


def test_ragged_reads_across_blocks_and_words(ctx):
    files = qc.ragged_case()
    assert 4000 <= len(files[0]) <= 6000
    _want, stats = check_apply(ctx, files)
    assert stats["changed"] > 300 and stats["stopped"] > 0 and stats["anchored"] > 3000


def test_planted_errors(ctx):
    files, clean = qc.planted_case()
    want, stats = check_apply(ctx, files)
    altered = back = 0
    for f in range(2):
        for (bases, _q), c, o in zip(files[f], clean[f], want[f]):
            altered += bases != c
            back += bases != c and o == c
            assert bases != c or o == c                                 # no clean read is changed
    assert back >= 0.95 * altered and altered >= 150


def test_refusals(ctx):
    from shannon_amd import quorum, _lib
    case = qc.scenario("mid")
    I, J = Ingested(ctx, case["files"]), Ingested(ctx, case["files"])
    try:
        with pytest.raises(_lib.ShannonError, match="needs FASTQ text"):
            quorum.hq_mask(ctx, I.sets[0], qc.fasta_text([b for b, _q in case["files"][0]]).encode())
        with pytest.raises(_lib.ShannonError, match="records"):
            quorum.hq_mask(ctx, I.sets[0], qc.fastq_text(case["files"][0][:-1]).encode())
        with pytest.raises(_lib.ShannonError, match="quality line"):
            quorum.hq_mask(ctx, I.sets[0], qc.fastq_text([(b, ql[:-1]) for b, ql in case["files"][0]]).encode())
        m = quorum.hq_mask(ctx, I.sets[0], I.texts[0])
        for k in (14, 33):
            with pytest.raises(_lib.ShannonError, match="k outside 15 .. 32"):
                quorum.trusted_table(ctx, I.sets, [m], k)
        with pytest.raises(_lib.ShannonError, match="does not belong"):
            quorum.trusted_table(ctx, J.sets, [m])                      # the same reads, but another set
        t = quorum.trusted_table(ctx, I.sets, [m])
        for kw, msg in ((dict(k=14), "k outside"), (dict(k=33), "k outside"), (dict(k=25), "not a canonical table of k-mers of this k"),
                        (dict(anchor_count=0), "anchor_count is 0"), (dict(max_subs=5), "max_subs above 4")):
            with pytest.raises(_lib.ShannonError, match=msg):
                quorum.correct(ctx, I.sets[0], t, **kw)
        # a ragged set and a text with the same records, words and bases in all, two lengths exchanged
        ragged = [("ACGT" * 10, "I" * 40), ("TTGCA" * 6, "I" * 30), ("GATTACA" * 10, "I" * 70)]
        R = Ingested(ctx, [ragged])
        try:
            with pytest.raises(_lib.ShannonError, match="record 0 has 30 bases, the set's read 40"):
                quorum.hq_mask(ctx, R.sets[0], qc.fastq_text([ragged[1], ragged[0], ragged[2]]).encode())
            quorum.hq_mask(ctx, R.sets[0], R.texts[0]).close()
        finally:
            R.close()
        c, st = quorum.correct(ctx, I.sets[0], t)                       # and what is not refused works
        assert st["changed"] == 1 and resident_strings(c)[0] == case["clean"]
        c.close()
        t.close()
        m.close()
    finally:
        I.close()
        J.close()


# ---------------------------------------------------------------------------------------------------------------- command line
def _run_cli(argv, capsys):
    """shannon.main in this process (one device context per run, closed at its end); returns what it printed"""
    import shannon
    capsys.readouterr()
    rc = shannon.main(["shannon.py"] + argv)
    out = capsys.readouterr().out
    assert rc == 0, out
    return out


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted-error pairs as FASTQ and as FASTA files, the brute force's corrected reads as FASTA files"""
    files, _clean = qc.planted_case()
    want, stats, _t = qc.brute_apply(files)
    d = tmp_path_factory.mktemp("quorum_cli")
    paths = {}
    for m in (0, 1):
        for kind, text in (("fastq", qc.fastq_text(files[m])), ("fasta", qc.fasta_text([b for b, _q in files[m]])), ("fixed.fasta", qc.fasta_text(want[m]))):
            p = d / ("r%d.%s" % (m + 1, kind))
            p.write_text(text)
            paths[kind, m] = str(p)
    return {"dir": d, "paths": paths, "want": want, "stats": stats, "files": files}


LOG = re.compile(r"--quorum: .*: (\d+) of (\d+) reads anchored, (\d+) changed, (\d+) substitutions, (\d+) stopped directions, (\d+) window reverts; "
                 r"table of (\d+) k-mers from (\d+) high-quality windows")


def test_cli_corrects_fastq_input(ctx, planted, capsys, monkeypatch):
    """corrected_reads*.fa and the log's counters are the brute force's; shannon.fasta is that of a run given the brute force's
    corrected reads as plain FASTA"""
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    P, d = planted["paths"], planted["dir"]
    out, ref = d / "q" / "OUT", d / "fixed" / "OUT"
    printed = _run_cli(["-o", str(out), "--left", P["fastq", 0], "--right", P["fastq", 1], "--quorum"], capsys)
    assert "OPTIONS --quorum: read error correction with quality scores enabled" in printed and "ignored" not in printed
    for m in (0, 1):
        text = (out / "TEMP" / ("corrected_reads_%d.fa" % (m + 1))).read_text()
        assert text == "".join(">%d_%d\n%s\n" % (i, m + 1, s) for i, s in enumerate(planted["want"][m]))
    log = (out / "log.txt").read_text().splitlines()
    hits = [LOG.search(l) for l in log if "--quorum: " in l]
    assert len(hits) == 1 and hits[0]
    st = planted["stats"]
    assert [int(x) for x in hits[0].groups()] == [st["anchored"], 2 * len(planted["files"][0]), st["changed"], st["substitutions"], st["stopped"],
                                                   st["reverts"], st["table"], st["windows"]]
    kern = [l for l in log if "quorum kernels: " in l]
    assert len(kern) == 1 and all(('"%s"' % g) in kern[0] for g in ("quorum.count", "quorum.table", "quorum.correct"))
    _run_cli(["-o", str(ref), "--left", P["fixed.fasta", 0], "--right", P["fixed.fasta", 1]], capsys)
    final = (out / "shannon.fasta").read_bytes()
    assert final == (ref / "shannon.fasta").read_bytes() and final.count(b">") >= 4


def test_cli_fasta_input_is_left_alone(ctx, planted, capsys, monkeypatch):
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    P, d = planted["paths"], planted["dir"]
    flag, plain = d / "fa_flag" / "OUT", d / "fa_plain" / "OUT"
    printed = _run_cli(["-o", str(flag), "--left", P["fasta", 0], "--right", P["fasta", 1], "--quorum"], capsys)
    assert "OPTIONS WARNING: --quorum NOT enabled. Option only works with fastq input." in printed and "ignored: --quorum" in printed
    printed = _run_cli(["-o", str(plain), "--left", P["fasta", 0], "--right", P["fasta", 1]], capsys)
    assert "quorum" not in printed
    assert (flag / "shannon.fasta").read_bytes() == (plain / "shannon.fasta").read_bytes()
    assert not list((flag / "TEMP").glob("corrected_reads*")) and "quorum" not in (plain / "log.txt").read_text()


def test_cli_single_end(ctx, planted, capsys, monkeypatch):
    """--single: ONE file's table, corrected_reads.fa with the headers >i, the counters of the brute force over that file alone;
    shannon.fasta is that of a run given the brute force's corrected reads as plain FASTA"""
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    P, d = planted["paths"], planted["dir"]
    reads = planted["files"][0]
    want, st, _t = qc.brute_apply([reads])
    assert want[0] != planted["want"][0]                                # (the table of one file is not the table of the two)
    fixed = d / "single.fixed.fasta"
    fixed.write_text(qc.fasta_text(want[0]))
    out, ref = d / "single_q" / "OUT", d / "single_fixed" / "OUT"
    printed = _run_cli(["-o", str(out), "--single", P["fastq", 0], "--quorum"], capsys)
    assert "OPTIONS --quorum: read error correction with quality scores enabled" in printed and "ignored" not in printed
    assert sorted(p.name for p in (out / "TEMP").glob("corrected_reads*")) == ["corrected_reads.fa"]
    assert (out / "TEMP" / "corrected_reads.fa").read_text() == "".join(">%d\n%s\n" % (i, s) for i, s in enumerate(want[0]))
    hits = [LOG.search(l) for l in (out / "log.txt").read_text().splitlines() if "--quorum: " in l]
    assert len(hits) == 1 and hits[0]
    assert [int(x) for x in hits[0].groups()] == [st["anchored"], len(reads), st["changed"], st["substitutions"], st["stopped"], st["reverts"],
                                                   st["table"], st["windows"]]
    _run_cli(["-o", str(ref), "--single", str(fixed)], capsys)
    final = (out / "shannon.fasta").read_bytes()
    assert final == (ref / "shannon.fasta").read_bytes() and final.count(b">") >= 1


def test_pipeline_quantifies_the_sets_it_is_told_to(ctx, planted):
    """assemble(kallisto_reads=...): the abundance step sees THOSE sets -- told by their number of pairs -- and the sets passed in by default"""
    from shannon_amd import pipeline
    r1, r2 = ([b for b, _q in f] for f in planted["files"])
    I = Ingested(ctx, [f[:100] for f in planted["files"]])
    try:
        kw = dict(K=24, sample="s", seed=0, kallisto_cutoff=1.0)
        plain = pipeline.assemble(ctx, r1, r2, **kw)
        told = pipeline.assemble(ctx, r1, r2, kallisto_reads=(I.sets[0], I.sets[1]), **kw)
    finally:
        I.close()
    assert plain.abundance["fragments"] == len(r1) == 480 and told.abundance["fragments"] == 100
    assert dict(told.final_before_kallisto) == dict(plain.final_before_kallisto) and len(plain.final_before_kallisto) >= 4
    assert 0 < told.abundance["mapped"] <= 100 < plain.abundance["mapped"]
    assert told.abundance["L"] == plain.abundance["L"] == 100.0


def test_cli_kallisto_sees_the_original_reads(ctx, tmp_path, capsys, monkeypatch):
    """--quorum --kallisto_cutoff on pairs of which twelve have a mate with two errors: as they stand those pairs cannot be placed
    (one mismatch a 50-base mate at the most), corrected they can.  The transcripts come from the corrected reads, the abundances
    from the ORIGINAL ones: the log's mapped is what abundance.quantify gives for the original sets on the run's transcripts, twelve
    below what it gives for the corrected sets, and abundance.tsv is the originals'.  Where the transcripts of a run without
    --quorum coincide, its fragments and mapped are the same."""
    from shannon_amd import abundance
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    files, _clean, double = qc.kallisto_case()
    want, _stats, _t = qc.brute_apply(files)
    P = []
    for m in (0, 1):
        p = tmp_path / ("r%d.fastq" % (m + 1))
        p.write_text(qc.fastq_text(files[m]))
        P.append(str(p))
    both, only = tmp_path / "qk" / "OUT", tmp_path / "k" / "OUT"
    args = ["--left", P[0], "--right", P[1], "--kallisto_cutoff", "1"]
    _run_cli(["-o", str(both)] + args + ["--quorum"], capsys)
    _run_cli(["-o", str(only)] + args, capsys)
    pat = re.compile(r"--kallisto_cutoff 1.0: (\d+) of (\d+) fragments mapped")

    def mapped(o):
        hits = [pat.search(l) for l in (o / "log.txt").read_text().splitlines() if "fragments mapped" in l]
        assert len(hits) == 1 and hits[0]
        return int(hits[0].group(1)), int(hits[0].group(2))
    before = [(o / "TEMP" / "OUT_allalgo_output" / "rec_before_kallisto.fasta").read_text() for o in (both, only)]
    got = mapped(both)
    lines = before[0].splitlines()
    names, seqs = [l[1:] for l in lines[0::2]], lines[1::2]
    I = Ingested(ctx, files)
    C = Ingested(ctx, [[(s, "I" * len(s)) for s in f] for f in want])
    try:
        orig = abundance.quantify(ctx, names, seqs, I.sets[0], I.sets[1], False)
        fixed = abundance.quantify(ctx, names, seqs, C.sets[0], C.sets[1], False)
    finally:
        I.close()
        C.close()
    print("mapped, fragments: with --quorum %s, without %s; transcripts coincide: %s; quantify: originals %d, corrected %d"
          % (got, mapped(only), before[0] == before[1], orig["mapped"], fixed["mapped"]))
    assert len(names) >= 4 and got[1] == len(files[0]) == orig["fragments"]
    assert fixed["mapped"] == orig["mapped"] + len(double) and len(double) == 12         # the two sets do quantify differently ...
    assert got[0] == orig["mapped"]                                                      # ... and the run saw the original one
    tsv = (both / "TEMP" / "OUT_allalgo_output" / "kallisto" / "abundance.tsv").read_text()
    assert tsv == abundance.abundance_tsv(orig) and tsv != abundance.abundance_tsv(fixed)
    if before[0] == before[1]:
        assert got == mapped(only)
