"""GPU parity, end to end: shannon_amd.pipeline (HIP kernels + host mirrors) vs the oracle
pipeline on the golden inputs: identical transcript sequences, abundances within 1e-6 rel."""
import pytest
from golden_util import *

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def cmp_fasta(a, b):
    ra, rb = parse_fasta(a), parse_fasta(b)
    assert len(ra) == len(rb)
    for (h1, s1), (h2, s2) in zip(ra, rb):
        assert s1 == s2
        t1, t2 = h1.split("\t"), h2.split("\t")
        assert t1[0] == t2[0] and t1[2:] == t2[2:]
        if "Copycount" in t1[1]:
            assert t1[1] == t2[1]
        else:
            assert abs(float(t1[1]) - float(t2[1])) <= 1e-6 * max(1.0, abs(float(t1[1])))


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_end_to_end_vs_oracle(ctx, name):
    from shannon_amd import pipeline
    from oracle import pipeline as opipe
    m = MANIFEST[name]
    g = load_case(name)
    inp = load_inputs(name)
    psize = m.get("partition_size", 500)
    pv = [part_vectors(len(b["contigs"]), psize) for b in g["big_components"]] or None
    ds = not strand_specific(name)                          # -s / --ss cases: shannon.py:407-411
    R = pipeline.assemble(ctx, inp[0], inp[1] if m["paired"] else None, K=m["K"], partition_size=psize, sample="s",
                          seed=m["sf_seed"], part_vectors=pv, double_stranded=ds)
    O = opipe.assemble(inp[0], inp[1] if m["paired"] else None, K=m["K"], partition_size=psize, sample="s",
                       seed=m["sf_seed"], part_vectors=pv, double_stranded=ds)
    assert R.extension.contigs == O["contigs"] == g["contigs"]
    assert list(R.partitions) == list(O["partitions"]) == list(g["partitions"])
    for p in R.partitions:
        cmp_fasta(R.partitions[p]["reconstructed_fasta"], O["partitions"][p]["reconstructed_fasta"])
        # and the reference's own graph for that partition (canonical form)
        from shannon_amd import mbgraph
        can = mbgraph.canonical(R.partitions[p]["singles"], R.partitions[p]["components"])
        for k in can:
            assert approx_eq(can[k], g["partitions"][p]["graph"][k])
    assert R.final == O["final"]                 # final shannon.fasta as {name: sequence}
    # ... and the reference's own final file (process_concatenated_fasta -> perl sort -> faster_reps -d on the reference run's
    # concatenation, ref_harness.run_final): the sequences -- the names carry the reference's address-ordered component numbers
    # Sparse flow visits nodes in id order and the reference numbers them in address order (one fixture, syn_pe_hairpin_K31, decomposes
    # a node differently for that: the reference itself is not reproducible there without setarch -R), so the comparison holds
    # wherever the partitions' transcripts equal the reference's; test_lp_gpu.py runs the reference's own tables to the final file.
    key = "ds" if ds else "ss"
    same = all(sorted(sq for _h, sq in parse_fasta(R.partitions[p]["reconstructed_fasta"])) ==
               sorted(sq for _h, sq in parse_fasta(g["partitions"][p]["reconstructed_fasta"])) for p in R.partitions)
    assert same or name == "syn_pe_hairpin_K31"
    if same:
        assert sorted(R.final.values()) == sorted(g["final"][key].values())
    # the device merge on the reference's own concatenation: names too
    from shannon_amd import post
    for k2, d2 in (("ds", True), ("ss", False)):
        assert post.finalize_texts([g["all_reconstructed"]], d2, ctx=ctx) == g["final"][k2]


@pytest.mark.parametrize("name", ["se_K24", "syn_part_s33", "syn_pe_hairpin_K31"])
def test_end_to_end_vs_oracle_under_the_unitig_check(ctx, name, monkeypatch):
    """the same once more with SHN_GRAPH_CHECK=1 (a single-end case, a paired one that goes through the gpmetis branch, one at
    K = 31): every real partition's GPU unitigs are held against load_k1mers + condense_all by the graph stage's own
    order-sensitive comparison, in rows mode, where the byte rows are made on demand; a difference is an error return"""
    monkeypatch.setenv("SHN_GRAPH_CHECK", "1")
    test_end_to_end_vs_oracle(ctx, name)


def test_cli_config1_samples_se(tmp_path):
    """BASELINE configs[0]: Samples/SE_read.fasta, single-end, -K 25, through the shannon.py CLI."""
    import gzip, subprocess, sys, os
    from conftest import ROOT
    from oracle import pipeline as opipe
    fa = tmp_path / "SE_read.fasta"
    with gzip.open(os.path.join(GOLD, "data", "SE_read.fasta.gz"), "rt") as f:
        fa.write_text(f.read())
    out = tmp_path / "OUT"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", str(out), "--single", str(fa), "-K", "25"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    assert (out / "shannon.fasta").exists() and (out / "log.txt").exists() and (out / "TEMP").is_dir()
    got = dict((h[1:], s) for h, s in parse_fasta((out / "shannon.fasta").read_text()))
    ref = opipe.assemble(load_inputs("se_K25")[0], None, K=25, sample="OUT", seed=0)
    assert got == ref["final"]
    g = load_case("se_K25")
    assert (out / "TEMP" / "OUT_algo_input" / "k1mer.dict_contig").read_text().split() == g["contigs"]
    # reads of 48-51 bases: the device ingest takes them as codes + offsets (shn_reads_ingest_ragged), no Python read loop
    assert "through the device ingest" in (out / "log.txt").read_text()
    # a second run into the same non-empty directory is refused, as in shannon.py:255-257
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", str(out), "--single", str(fa)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode != 0 and "not empty" in p.stdout


@pytest.mark.parametrize("flag", ["-s", "--strand_specific"])
def test_cli_strand_specific_pe(tmp_path, flag):
    """-s / --ss / --strand_specific (shannon.py:407-411) through the CLI on a paired case whose reference run was made with
    double_stranded = False: the contig file equals the reference's, the final FASTA the oracle's run of the same mode."""
    import subprocess, sys, os
    from conftest import ROOT
    from oracle import pipeline as opipe
    name = "syn_pe_ss_s69"
    inp = load_inputs(name)
    files = []
    for m, reads in enumerate(inp):
        fa = tmp_path / ("r%d.fasta" % (m + 1))
        fa.write_text("".join(">%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
        files.append(str(fa))
    out = tmp_path / "OUTSS"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", str(out), "--left", files[0], "--right", files[1], "-K", "25", flag],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    got = dict((h[1:], s) for h, s in parse_fasta((out / "shannon.fasta").read_text()))
    ref = opipe.assemble(inp[0], inp[1], K=25, sample="OUTSS", seed=0, double_stranded=False)
    assert got == ref["final"] and len(got) > 0
    assert (out / "TEMP" / "OUTSS_algo_input" / "k1mer.dict_contig").read_text().split() == load_case(name)["contigs"]


def test_cli_samples_pe(tmp_path):
    """Samples/PE_read_1.fasta + PE_read_2.fasta through the shannon.py CLI (--left / --right, -K 25): the final FASTA and the
    contig file equal the oracle's run and the reference's golden contigs; the TEMP tree has the reference's layout."""
    import gzip, subprocess, sys, os
    from conftest import ROOT
    from oracle import pipeline as opipe
    files = []
    for nm in ("PE_read_1.fasta", "PE_read_2.fasta"):
        fa = tmp_path / nm
        with gzip.open(os.path.join(GOLD, "data", nm + ".gz"), "rt") as f:
            fa.write_text(f.read())
        files.append(str(fa))
    out = tmp_path / "OUTPE"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", str(out), "--left", files[0], "--right", files[1], "-K", "25"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    got = dict((h[1:], s) for h, s in parse_fasta((out / "shannon.fasta").read_text()))
    inp = load_inputs("pe_K25")
    ref = opipe.assemble(inp[0], inp[1], K=25, sample="OUTPE", seed=0)
    assert got == ref["final"] and len(got) > 0
    g = load_case("pe_K25")
    assert (out / "TEMP" / "OUTPE_algo_input" / "k1mer.dict_contig").read_text().split() == g["contigs"]
    # the files went through the device ingest although 1,098 / 1,552 of their reads hold an N (kept and marked, not refused)
    assert "through the device ingest" in (out / "log.txt").read_text()


@pytest.mark.parametrize("K", [25, 31])
def test_graph_reads_gathered_on_the_device_equal_uploaded_text(ctx, monkeypatch, K):
    """With code-matrix input the graph stage builds the device copy of a partition's distinct reads by gathering rows of the
    resident packed input (shn_reads_gather, reverse complements on chip) instead of uploading their text: same graphs, same
    transcripts -- paired and single-end, several partitions."""
    import numpy as np
    from shannon_amd import pipeline, synth
    (r1, r2), _ = synth.make_dataset(30000, 40, seed=31)
    for paired in (True, False):
        outs = []
        # rows named on the device (shn_mbgraph_run_rows) / rows gathered on the host + device copy gathered / text uploaded /
        # rows gathered on the host, distinct reads found on the device
        for env in ({}, {"SHN_GRAPH_ROWS": "0"}, {"SHN_GRAPH_ROWS": "0", "SHN_GRAPH_RESIDENT_READS": "0"},
                    {"SHN_GRAPH_ROWS": "0", "SHN_GRAPH_BULK_MIN": "64"}, {"SHN_GRAPH_ROWS": "0", "SHN_GRAPH_BULK_MIN": "64", "SHN_GRAPH_DEVICE_DEDUP": "0"},
                    {"SHN_GRAPH_KP_GPU": "0"},                       # known_paths' in-node test on host threads instead of the device
                    {"SHN_GRAPH_LAZY_TEXT": "0"},                    # the text of every distinct read decoded up front
                    {"SHN_GRAPH_DEV_ATTRS": "0"},                    # copies / mates / path states per read in host arrays (the form before graph_dev.h)
                    {"SHN_GRAPH_DEV_ATTRS": "0", "SHN_GRAPH_KP_SEARCH": "0"},
                    {"SHN_SFLOW_BESIDE": "0"}):                      # one sparse-flow call over all partitions after the graph stage (default: beside it)
            for k in ("SHN_GRAPH_ROWS", "SHN_GRAPH_RESIDENT_READS", "SHN_GRAPH_BULK_MIN", "SHN_GRAPH_DEVICE_DEDUP", "SHN_GRAPH_KP_GPU", "SHN_GRAPH_LAZY_TEXT",
                      "SHN_GRAPH_DEV_ATTRS", "SHN_GRAPH_KP_SEARCH", "SHN_SFLOW_BESIDE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            R = pipeline.assemble(ctx, r1, r2 if paired else None, K=K, partition_size=8, sample="s", seed=2)
            outs.append(R)
        a = outs[0]
        for b in outs[1:]:
            assert len(a.partitions) > 1 and list(a.partitions) == list(b.partitions)
            for p in a.partitions:
                assert a.partitions[p]["reconstructed_fasta"] == b.partitions[p]["reconstructed_fasta"]
                assert a.partitions[p]["components"] == b.partitions[p]["components"] and a.partitions[p]["singles"] == b.partitions[p]["singles"]
            assert a.final == b.final and len(a.final) > 10


def _dedup_vs_read_dictionary(ctx, paired, L, seed):
    import numpy as np
    from shannon_amd import device, mbgraph_native
    rng = np.random.RandomState(seed)
    n = 3000
    pool = rng.randint(0, 4, size=(40, L)).astype(np.uint8)
    pool[7] = (3 - pool[6][::-1])                                   # a read and its reverse complement, and a palindrome-free pool otherwise
    if L % 2 == 0:                                                  # (even lengths: one read that is its own reverse complement)
        pool[8][L // 2:] = 3 - pool[8][:L // 2][::-1]
    m1 = pool[rng.randint(0, 40, size=n)].copy()
    m2 = pool[rng.randint(0, 40, size=n)].copy()
    d1 = device.Reads.from_codes(ctx, m1)
    d2 = device.Reads.from_codes(ctx, m2) if paired else None
    didx = np.sort(rng.choice(2 * n, size=2500, replace=False)).astype(np.uint32)
    slot, cnt, mate, role = mbgraph_native.reads_dedup(ctx, d1, d2, didx)
    rc = lambda r: (3 - r[::-1])
    def text(d, mt):
        second = d >= n
        i = d - n if second else d
        if not paired:
            r = rc(m1[i]) if second else m1[i]
        elif mt == 0:
            r = rc(m2[i]) if second else m1[i]
        else:
            r = m2[i] if second else rc(m1[i])
        return r.tobytes()
    ids, first, counts, mates, roles = {}, [], [], [], []
    for i, d in enumerate(didx):
        got = []
        for mt in range(2 if paired else 1):
            t = text(int(d), mt)
            if t not in ids:
                ids[t] = len(ids); first.append(i * (2 if paired else 1) + mt); counts.append(0); mates.append(-1); roles.append(0)
            counts[ids[t]] += 1
            got.append(ids[t])
        if paired:
            a, b = got
            roles[a] = 1; roles[b] = 2; mates[a] = b; mates[b] = a
    assert len(ids) < len(didx) and len(slot) == len(ids)
    assert slot.tolist() == first and cnt.tolist() == counts and mate.tolist() == mates and role.tolist() == roles
    d1.close()
    if d2 is not None:
        d2.close()


@pytest.mark.parametrize("paired", [False, True])
def test_distinct_reads_found_on_the_device_equal_the_read_dictionary(ctx, paired):
    """shn_reads_dedup against Read.reads filled one read (pair) at a time (mbgraph.py:56-70, multibridging.py:185-236): ids in
    order of first occurrence, copy counts, and for pairs the role and mate of each read's LAST occurrence."""
    _dedup_vs_read_dictionary(ctx, paired, 77, 5 + paired)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("L", [31, 32, 64, 96, 128, 129, 150, 250, 512, 513, 600])
def test_distinct_reads_found_on_the_device_at_read_lengths(ctx, paired, L):
    """The same at the edges of the word geometry (32 bases per word, 2 * ceil(L / 64) words per read): one word, exact words, a
    whole padding word; dd_insert<4> up to 128 bases, dd_insert<16> at 129-512, dd_insert_wide beyond (reads of more than 512
    bases used to be refused, which failed the graph stage of any run on such reads)."""
    _dedup_vs_read_dictionary(ctx, paired, L, 11 * L + paired)


def _lengths_case(case):
    """inputs of test_end_to_end_at_read_lengths: (reads for the pipeline, reads for the oracle) -- code matrices where the reads
    have one length per mate file (the graph stage then names them by rows of the resident sets), strings otherwise"""
    import numpy as np
    from shannon_amd import synth
    A = np.frombuffer(b"ACGT", np.uint8)
    txt = lambda rows: [A[r].tobytes().decode() for r in rows]
    iso, _ = synth.make_transcriptome(5, seed=61)
    L = {"L513": 513, "L600": 600}.get(case, 150)
    iso = [t for t in iso if len(t) >= L + 150]
    r1, r2 = synth.sample_pairs(iso, 1200, 62, read_len=L, frag_len=L + 150, err=0.003)
    if case in ("L513", "L600"):
        return (r1, r2), (txt(r1), txt(r2))
    if case == "mates_differ":
        a, b = np.ascontiguousarray(r1[:, :100]), np.ascontiguousarray(r2[:, :80])
        return (a, b), (txt(a), txt(b))
    rng = np.random.RandomState(63)                                   # ragged: 30-150 bases, the mates of a pair of different lengths
    s1 = [t[:rng.randint(30, 151)] for t in txt(r1)]
    s2 = [t[:rng.randint(30, 151)] for t in txt(r2)]
    return (s1, s2), (s1, s2)


@pytest.mark.parametrize("case", ["L513", "L600", "ragged", "mates_differ"])
def test_end_to_end_at_read_lengths(ctx, case):
    """Reads the device duplicate search took no part in before, or must be kept away from: longer than 512 bases (one word
    more than its register bound), a ragged set, mates of different fixed lengths -- pipeline.assemble against the oracle."""
    from shannon_amd import pipeline
    from oracle import pipeline as opipe
    (p1, p2), (o1, o2) = _lengths_case(case)
    R = pipeline.assemble(ctx, p1, p2, K=25, sample="s", seed=7)
    O = opipe.assemble(o1, o2, K=25, sample="s", seed=7)
    assert R.extension.contigs == O["contigs"]
    assert list(R.partitions) == list(O["partitions"]) and len(R.partitions) > 0
    for p in R.partitions:
        cmp_fasta(R.partitions[p]["reconstructed_fasta"], O["partitions"][p]["reconstructed_fasta"])
    assert R.final == O["final"] and len(R.final) > 0


def test_two_batches_in_flight_give_the_sequential_results(ctx):
    """pipeline.assemble_resident(defer_back=True): the host-bound half of a step (graph stage, sparse flow, merge) runs on a second
    thread and context while the next batch's counting / extension runs on the first -- bench.py --overlap-steps.  Every batch's
    output equals the one-batch-at-a-time run."""
    from concurrent.futures import ThreadPoolExecutor
    from shannon_amd import device, pipeline, synth, kmers_for_component as kfc
    batches = []
    for seed in (31, 32):
        (r1, r2), _ = synth.make_dataset(30000, 40, seed=seed)
        batches.append((device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2), kfc.ReadStore(r1, r2)))
    want = [pipeline.assemble_resident(ctx, d1, d2, st, K=25, partition_size=8, sample="s", seed=2) for d1, d2, st in batches]
    ctx_b = device.Context(0)
    pool = ThreadPoolExecutor(max_workers=1)
    try:
        got, prev = [], None
        for rep in range(3):
            for d1, d2, st in batches:
                fin = pipeline.assemble_resident(ctx, d1, d2, st, K=25, partition_size=8, sample="s", seed=2, defer_back=True)
                if prev is not None:
                    got.append(prev.result())
                prev = pool.submit(fin, ctx_b)
        got.append(prev.result())
    finally:
        pool.shutdown(wait=True)
        ctx_b.close()
    assert len(got) == 6
    for i, R in enumerate(got):
        W = want[i % 2]
        assert R.final == W.final and R.extension.contigs == W.extension.contigs and list(R.partitions) == list(W.partitions)
        for p in W.partitions:
            assert R.partitions[p]["reconstructed_fasta"] == W.partitions[p]["reconstructed_fasta"]
    for d1, d2, _st in batches:
        d1.close(); d2.close()


@pytest.mark.parametrize("name", ["se_K24", "pe_K25", "syn_pe_s0", "syn_pe_hairpin_K31", "syn_pe_ss_s71", "syn_part_s33"])
def test_end_to_end_on_a_minimizer_bucketed_table(ctx, name, monkeypatch):
    """The counting path of large inputs (super-k-mers, csrc/count_sk.hip) hands the extension a table whose buckets are buckets of
    minimizers (shn_table layout 1: a k1-mer and its neighbours mostly share a bucket); forced here on the golden inputs: the same
    contigs, partitions, transcripts and final file as the reference / the oracle."""
    from shannon_amd import pipeline
    from oracle import pipeline as opipe
    monkeypatch.setenv("SHN_COUNT_DIRECT", "0")
    monkeypatch.setenv("SHN_COUNT_SK", "2")
    m = MANIFEST[name]
    g = load_case(name)
    inp = load_inputs(name)
    psize = m.get("partition_size", 500)
    pv = [part_vectors(len(b["contigs"]), psize) for b in g["big_components"]] or None
    ds = not strand_specific(name)
    ctx.timer_reset()
    R = pipeline.assemble(ctx, inp[0], inp[1] if m["paired"] else None, K=m["K"], partition_size=psize, sample="s",
                          seed=m["sf_seed"], part_vectors=pv, double_stranded=ds)
    assert "count.sk_buckets" in ctx.timers() or not ds          # (strand-specific runs merge two tables through the pairs path)
    assert R.extension.contigs == g["contigs"]
    assert list(R.partitions) == list(g["partitions"])
    O = opipe.assemble(inp[0], inp[1] if m["paired"] else None, K=m["K"], partition_size=psize, sample="s",
                       seed=m["sf_seed"], part_vectors=pv, double_stranded=ds)
    for p in R.partitions:
        cmp_fasta(R.partitions[p]["reconstructed_fasta"], O["partitions"][p]["reconstructed_fasta"])
    assert R.final == O["final"]


def test_own_partitioner_through_the_pipeline(ctx):
    """a8 with the partition COMPUTED (no gpmetis output to replay): 60 genes sharing three repeated elements give two contig
    components of ~120 contigs (the strands' twins); with --partition 10 they go through the product's multilevel partitioner, twice
    (the second time on the penalised graph, kmers_for_component.py:207-237).  The oracle pipeline given exactly those partition
    vectors produces the same partitions, transcripts and final file -- and every part is non-empty and within gpmetis' balance
    bound."""
    import numpy as np
    from shannon_amd import pipeline, synth, kmers_for_component as kfc
    from oracle import pipeline as opipe
    rng = np.random.Generator(np.random.PCG64(17))
    S = [rng.integers(0, 4, 120, dtype=np.uint8) for _ in range(3)]
    iso = []
    for i in range(60):
        iso.append(np.concatenate([rng.integers(0, 4, int(rng.integers(200, 400)), dtype=np.uint8), S[i % 3],
                                   rng.integers(0, 4, int(rng.integers(200, 400)), dtype=np.uint8),
                                   S[(i + 1) % 3] if i % 4 == 0 else rng.integers(0, 4, 5, dtype=np.uint8), rng.integers(0, 4, 150, dtype=np.uint8)]))
    r1, r2 = synth.sample_pairs(iso, 40000, 5, err=0.003)
    A = np.frombuffer(b"ACGT", np.uint8)
    s1, s2 = [A[r].tobytes().decode() for r in r1], [A[r].tobytes().decode() for r in r2]
    psize = 10
    R = pipeline.assemble(ctx, s1, s2, K=25, partition_size=psize, sample="s", seed=3)
    big = R.extension.big_components
    assert len(big) == 2 and min(len(c) for c, _m in big) > 100
    pv = []
    for contigs, metis in big:
        P = kfc.n_partitions(len(contigs), psize)
        p1 = kfc.partition_graph(metis, P, 1000)
        pv.append((p1, kfc.partition_graph(kfc.weight_updated_graph(metis, p1, 5), P, 1000)))
        assert set(p1) == set(range(P)) and max(np.bincount(p1)) <= 2.0 * len(contigs) / P + 1
    O = opipe.assemble(s1, s2, K=25, partition_size=psize, sample="s", seed=3, part_vectors=pv)
    assert list(R.partitions) == list(O["partitions"]) and sum(1 for p in R.partitions if p.startswith("r2_c")) >= 10
    for p in R.partitions:
        cmp_fasta(R.partitions[p]["reconstructed_fasta"], O["partitions"][p]["reconstructed_fasta"])
    assert R.final == O["final"] and len(R.final) >= 40


def test_repeat_linked_genes_through_the_partitioner(ctx, monkeypatch):
    """the input shape of `bench.py --config 2p` at test size: 70 genes linked by three shared repeats (synth.make_repeat_family)
    give contig components far above --partition; they are cut by the library's partitioner (shn_partition_metis, twice:
    kmers_for_component.py:207-237) -- the same vectors as its Python mirror -- and the oracle pipeline given exactly those vectors
    produces the same partitions, transcripts and final file."""
    import numpy as np
    from shannon_amd import pipeline, synth, kmers_for_component as kfc
    from oracle import pipeline as opipe
    iso = synth.make_repeat_family(70, seed=29)
    r1, r2 = synth.sample_pairs(iso, 32000, 9, err=0.003, sigma=0.5)
    A = np.frombuffer(b"ACGT", np.uint8)
    s1, s2 = [A[r].tobytes().decode() for r in r1], [A[r].tobytes().decode() for r in r2]
    psize = 20
    monkeypatch.setenv("SHN_PROBE_GPU", "1")        # k1mers2component on the device: every k1-mer of these components lies in two partitions (pg_pair_kernel)
    R = pipeline.assemble(ctx, s1, s2, K=25, partition_size=psize, sample="s", seed=3)
    big = R.extension.big_components
    assert big and max(len(c) for c, _m in big) >= 110, [len(c) for c, _m in big]
    pv = []
    for contigs, metis in big:
        P = kfc.n_partitions(len(contigs), psize)
        p1 = kfc.partition_graph(metis, P, 1000)
        assert p1 == kfc.partition_graph_py(metis, P, 1000)                       # the library's partitioner = its readable mirror
        pv.append((p1, kfc.partition_graph(kfc.weight_updated_graph(metis, p1, 5), P, 1000)))
        assert set(p1) == set(range(P)) and max(np.bincount(p1)) <= 2.0 * len(contigs) / P + 1
    O = opipe.assemble(s1, s2, K=25, partition_size=psize, sample="s", seed=3, part_vectors=pv)
    assert list(R.partitions) == list(O["partitions"]) and sum(1 for p in R.partitions if p.startswith("r2_c")) >= 10
    for p in R.partitions:
        cmp_fasta(R.partitions[p]["reconstructed_fasta"], O["partitions"][p]["reconstructed_fasta"])
    assert R.final == O["final"] and len(R.final) >= 40
