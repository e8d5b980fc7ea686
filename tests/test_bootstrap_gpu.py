"""GPU: the bootstrap replicates of `python -m shannon_amd.quant -b B --seed S` (csrc/abundance.hip).
shn_abundance_resample against the brute force of tests/bootstrap_cases.py (integers: compared exactly); shn_abundance_em_batch against
the unchanged shn_abundance_em one replicate at a time (np.array_equal on alpha, equal rounds: no tolerance -- that call is held to
its own brute force by tests/test_abundance_gpu.py); shn_abundance_bootstrap against the two; then the command."""
import numpy as np
import pytest
import abundance_cases as ac
import bootstrap_cases as bc
import filter_fp_cases as fc
import quant_cases as qc
from test_abundance_gpu import upload

pytestmark = pytest.mark.gpu

SEEDS = (0, 7, (1 << 64) - 1)
REPLICATES = (1, 3, 65)


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("name", sorted(bc.resample_cases()))
def test_resample_equals_the_brute_force(ctx, name):
    from shannon_amd import abundance
    n_c = bc.resample_cases()[name]
    N = sum(n_c)
    for seed in SEEDS:
        want = bc.brute_counts_np(n_c, max(REPLICATES), seed)            # (replicate b does not depend on B: test_bootstrap.py)
        for B in REPLICATES:
            got = abundance.resample(ctx, n_c, B, seed)
            assert got.dtype == np.uint64 and got.shape == (B, len(n_c))
            assert np.array_equal(got, want[:B]), (name, seed, B)
            assert (got.sum(axis=1) == N).all() and not got[:, np.array(n_c) == 0].any()


def test_resample_refuses_2_to_the_32_fragments_without_a_launch(ctx):
    from shannon_amd import abundance, _lib
    for n_c in ([1 << 32], [1 << 31, 5, 1 << 31], [(1 << 64) - 1, 1]):
        ctx.timer_reset()
        with pytest.raises(_lib.ShannonError, match="shn_abundance_resample: 2\\^32 or more fragments"):
            abundance.resample(ctx, n_c, 1, 0)
        assert not any(k.startswith("abundance.") for k in ctx.timers()), "nothing launched"
    with pytest.raises(ValueError):
        abundance.resample(ctx, [3], 0, 0)
    with pytest.raises(ValueError):
        abundance.resample(ctx, [3], 1 << 32, 0)
    with pytest.raises(ValueError):
        abundance.resample(ctx, [3], 1, 1 << 64)
    assert abundance.resample(ctx, [], 2, 0).shape == (2, 0)


# ---------------------------------------------------------------------------------------------------------------- EM
def oracle(ctx, off, mem, matrix, eff):
    """abundance.em, one row at a time -> (alpha[B][m], rounds[B])"""
    from shannon_amd import abundance
    out = [abundance.em(ctx, off, mem, row, eff) for row in matrix]
    return np.array([a for a, _ in out]).reshape(len(matrix), len(eff)), np.array([r for _, r in out], dtype=np.uint32)


def check_batch(ctx, off, mem, matrix, eff, want, label):
    """em_batch over the first 1, 2 and all rows, resident 0 (the budget), 1 and 2 at once, against the oracle's rows"""
    from shannon_amd import abundance
    alpha, rounds = want
    for B in sorted(set((1, 2, len(matrix)))):
        if B > len(matrix):
            continue
        for max_live in (0, 1, 2):
            got, got_rounds = abundance.em_batch(ctx, off, mem, matrix[:B], eff, max_live=max_live)
            assert got.shape == (B, len(eff)) and got_rounds.shape == (B,)
            assert got_rounds.tolist() == rounds[:B].tolist(), (label, B, max_live)
            assert np.array_equal(got, alpha[:B]), (label, B, max_live)


@pytest.mark.parametrize("name", sorted(ac.em_cases()))
def test_em_batch_equals_em_per_replicate(ctx, name):
    lists, n_c, eff, m = ac.em_cases()[name]
    off, mem = ac.csr(lists)
    matrix = bc.brute_counts_np(n_c, 65, 7)
    want = oracle(ctx, off, mem, matrix, eff)
    print("em_batch %s: rounds of the 65 replicates %s" % (name, sorted(set(want[1].tolist()))))
    check_batch(ctx, off, mem, matrix, eff, want, name)


def test_em_batch_replicates_that_stop_at_different_rounds(ctx):
    """the replicates leave the launches at their own rounds (DESIGN.md 3.10 records 50, 100 and 150 rounds for the three inputs), one of
    them with all-zero counts, and the ones still running are not disturbed"""
    lists, matrix, eff, m = ac.union_case()
    off, mem = ac.csr(lists)
    want = oracle(ctx, off, mem, matrix, eff)
    print("rounds of the hand-made replicates: %s" % want[1].tolist())
    assert len(set(want[1].tolist())) >= 2
    assert not want[0][4].any() and want[1][4] == 50                     # the replicate without counts: all zeros after the first test
    check_batch(ctx, off, mem, matrix, eff, want, "union")
    order = [3, 4, 0, 2, 1]                                              # ... in another order: a slot's answer does not depend on its neighbours
    check_batch(ctx, off, mem, matrix[order], eff, (want[0][order], want[1][order]), "union, reordered")


def test_em_batch_one_transcript_and_no_classes(ctx):
    from shannon_amd import abundance
    off, mem = ac.csr([[0]])
    matrix = np.array([[5], [0], [7]], dtype=np.uint64)
    want = oracle(ctx, off, mem, matrix, [100.0])
    assert want[0].tolist() == [[5.0], [0.0], [7.0]]
    check_batch(ctx, off, mem, matrix, [100.0], want, "m = 1")
    alpha, rounds = abundance.em_batch(ctx, [0], [], np.zeros((3, 0), np.uint64), [100.0, 50.0])      # no class at all
    assert alpha.tolist() == [[0.0, 0.0]] * 3 and rounds.tolist() == [50] * 3


def test_em_batch_refuses_bad_arguments(ctx):
    from shannon_amd import abundance, _lib
    ok = dict(class_off=[0, 2, 3], members=[0, 1, 1], n_c=[[5, 2], [1, 0]], eff=[100.0, 50.0])

    def call(**kw):
        a = dict(ok, **kw)
        return abundance.em_batch(ctx, np.array(a["class_off"], np.uint64), np.array(a["members"], np.uint32), np.array(a["n_c"], np.uint64),
                                  np.array(a["eff"], np.float64))
    assert (call()[1] % 50 == 0).all()
    for kw, msg in ((dict(class_off=[0, 3, 2]), "class_off not monotone"), (dict(class_off=[1, 2, 3]), "class_off\\[0\\] is not 0"),
                    (dict(members=[0, 2, 1]), "a class names transcript 2 of 2"), (dict(eff=[100.0, 0.0]), "eff of transcript 1 is not above 0"),
                    (dict(eff=[float("nan"), 50.0]), "eff of transcript 0 is not above 0")):
        ctx.timer_reset()
        with pytest.raises(_lib.ShannonError, match="shn_abundance_em_batch: " + msg):
            call(**kw)
        assert not any(k.startswith("abundance.") for k in ctx.timers()), "nothing launched"
    with pytest.raises(_lib.ShannonError, match="shn_abundance_em_batch: no transcripts \\(m is 0\\)"):
        abundance.em_batch(ctx, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((1, 0), np.uint64), np.zeros(0, np.float64))
    with pytest.raises(ValueError):
        call(n_c=[[5], [1]])
    with pytest.raises(ValueError):
        call(n_c=[5, 2])
    with pytest.raises(ValueError):
        call(class_off=[0, 2, 4])
    with pytest.raises(ValueError):
        call(n_c=np.zeros((0, 2)))


# ---------------------------------------------------------------------------------------------------------------- both
@pytest.mark.parametrize("name", ["shared pair", "a class of 65", "random, 300 transcripts"])
def test_bootstrap_is_resample_then_em_batch(ctx, name):
    from shannon_amd import abundance, _lib
    lists, n_c, eff, m = ac.em_cases()[name]
    off, mem = ac.csr(lists)
    for B, seed, max_live in ((1, 0, 0), (65, 7, 0), (5, (1 << 64) - 1, 2)):
        counts = abundance.resample(ctx, n_c, B, seed)
        assert np.array_equal(counts, bc.brute_counts_np(n_c, B, seed))
        alpha, rounds = abundance.em_batch(ctx, off, mem, counts, eff)
        a1, r1, c1 = abundance.bootstrap(ctx, off, mem, n_c, eff, B, seed, max_live=max_live, want_counts=True)
        a0, r0, c0 = abundance.bootstrap(ctx, off, mem, n_c, eff, B, seed, max_live=max_live)
        assert c0 is None and np.array_equal(c1, counts) and c1.dtype == np.uint64
        assert np.array_equal(a1, alpha) and np.array_equal(a0, alpha) and r1.tolist() == rounds.tolist() == r0.tolist()
    ctx.timer_reset()
    with pytest.raises(_lib.ShannonError, match="shn_abundance_bootstrap: 2\\^32 or more fragments"):
        abundance.bootstrap(ctx, [0, 1], [0], [1 << 32], [100.0], 2, 0)
    with pytest.raises(_lib.ShannonError, match="shn_abundance_bootstrap: a class names transcript 1 of 1"):
        abundance.bootstrap(ctx, [0, 1], [1], [4], [100.0], 2, 0)
    assert not any(k.startswith("abundance.") for k in ctx.timers()), "nothing launched"


# ---------------------------------------------------------------------------------------------------------------- the command
def _write_reads(path, reads):
    path.write_text("".join("@%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    return str(path)


def _run(argv, capsys):
    from shannon_amd import quant
    capsys.readouterr()
    rc = quant.main(["quant"] + argv)
    out = capsys.readouterr()
    assert rc == 0, out.err
    return out.out


def _check_command(ctx, tmp_path, capsys, names, T, read_args, cl, eff):
    """the files of a run with -b 4 --seed 7 against the brute force's counts -> abundance.em -> tpm_of -> abundance_tsv, for the classes
    cl and effective lengths eff the same inputs give"""
    from shannon_amd import abundance
    fa = tmp_path / "t.fasta"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in zip(names, T)))
    B = 4
    plain, out, again, other = (tmp_path / d for d in ("plain", "b4", "b4_again", "b4_seed8"))
    _run([str(fa), "-o", str(plain)] + read_args + ["--cutoff", "2"], capsys)
    _run([str(fa), "-o", str(out)] + read_args + ["--cutoff", "2", "-b", str(B), "--seed", "7"], capsys)
    assert (out / "abundance.tsv").read_bytes() == (plain / "abundance.tsv").read_bytes()
    assert (out / "filtered.fasta").read_bytes() == (plain / "filtered.fasta").read_bytes()
    assert sorted(p.name for p in plain.iterdir()) == ["abundance.tsv", "filtered.fasta", "quant_log.txt"]
    assert sorted(p.name for p in out.iterdir()) == sorted(["abundance.tsv", "filtered.fasta", "quant_log.txt", "bootstrap_summary.tsv"]
                                                           + ["bs_abundance_%d.tsv" % b for b in range(B)])
    counts = bc.brute_counts_np([int(x) for x in cl["n_c"]], B, 7)
    rows, rounds = [], []
    for b in range(B):
        alpha, r = abundance.em(ctx, cl["class_off"], cl["members"], counts[b], eff)
        table = {"names": names, "length": [len(s) for s in T], "eff_length": eff.tolist(), "est_counts": alpha.tolist(), "tpm": abundance.tpm_of(alpha, eff)}
        assert (out / ("bs_abundance_%d.tsv" % b)).read_text() == abundance.abundance_tsv(table), b
        rows.append(alpha.tolist())
        rounds.append(r)
    est = [float(l.split("\t")[3]) for l in (out / "abundance.tsv").read_text().splitlines()[1:]]
    summary = dict(abundance.bootstrap_summary(rows), names=names, est_counts=est)
    assert (out / "bootstrap_summary.tsv").read_text() == abundance.bootstrap_summary_tsv(summary)
    head = (out / "bootstrap_summary.tsv").read_text().splitlines()[0]
    assert head == "target_id\test_counts\tbs_mean\tbs_sd\tbs_min\tbs_max"
    log = (out / "quant_log.txt").read_text()
    assert "-b 4 --seed 7: EM rounds of the replicates %d .. %d" % (min(rounds), max(rounds)) in log
    assert "abundance.resample" in log and "abundance.em_batch" in log
    plain_log = (plain / "quant_log.txt").read_text()
    assert "abundance.resample" not in plain_log and "abundance.em_batch" not in plain_log and "EM rounds of the replicates" not in plain_log
    # a second run: identical files (the log holds times)
    _run([str(fa), "-o", str(again)] + read_args + ["--cutoff", "2", "-b", str(B), "--seed", "7"], capsys)
    for p in out.iterdir():
        if p.name != "quant_log.txt":
            assert (again / p.name).read_bytes() == p.read_bytes(), p.name
    # another seed: other counts (asserted on the brute force first), so another replicate 0
    assert not np.array_equal(bc.brute_counts_np([int(x) for x in cl["n_c"]], 1, 8)[0], counts[0])
    _run([str(fa), "-o", str(other)] + read_args + ["-b", str(B), "--seed", "8"], capsys)
    assert (other / "bs_abundance_0.tsv").read_bytes() != (out / "bs_abundance_0.tsv").read_bytes()
    assert (other / "abundance.tsv").read_bytes() == (plain / "abundance.tsv").read_bytes()


def test_command_paired(ctx, tmp_path, capsys):
    from shannon_amd import abundance
    T, names, r1, r2 = fc.planted_case(n_pairs=400)
    d1, d2 = upload(ctx, r1), upload(ctx, r2)
    try:
        cl = abundance.classes(ctx, T, d1, d2, False)
    finally:
        d1.close()
        d2.close()
    eff = abundance.eff_lengths([len(s) for s in T], cl["hist"])
    read_args = ["--left", _write_reads(tmp_path / "r1.fq", r1), "--right", _write_reads(tmp_path / "r2.fq", r2)]
    _check_command(ctx, tmp_path, capsys, names, T, read_args, cl, eff)


def test_command_single_end(ctx, tmp_path, capsys):
    from shannon_amd import abundance
    names, T, reads, _rare = qc.isoform_case()
    d = upload(ctx, reads)
    try:
        cl = abundance.classes_single(ctx, T, d, False)
    finally:
        d.close()
    eff = abundance.eff_lengths_model([len(s) for s in T])
    _check_command(ctx, tmp_path, capsys, names, T, ["--single", _write_reads(tmp_path / "r.fq", reads)], cl, eff)


def test_quantify_without_bootstraps_is_unchanged(ctx):
    """bootstraps=None: the table of before, key for key; with a number, the same columns and the new ones beside them"""
    from shannon_amd import abundance
    names, T, reads, _rare = qc.isoform_case()
    d = upload(ctx, reads)
    try:
        plain = abundance.quantify_single(ctx, names, T, d, False)
        with_b = abundance.quantify_single(ctx, names, T, d, False, bootstraps=3, seed=7)
    finally:
        d.close()
    assert sorted(plain) == ["classes", "eff_length", "est_counts", "fragments", "hist", "length", "mapped", "names", "rounds", "tpm"]
    for k in plain:
        assert np.array_equal(plain[k], with_b[k]), k
    assert len(with_b["bs_est_counts"]) == len(with_b["bs_tpm"]) == len(with_b["bs_rounds"]) == 3
    assert all(len(with_b[k]) == len(names) for k in ("bs_mean", "bs_sd", "bs_min", "bs_max"))
    assert all(abs(sum(row) - plain["mapped"]) < 1e-6 for row in with_b["bs_est_counts"])
