"""GPU: --filter_FP on N ranks (distributed.filter_owned_texts between the owners' sparse flow and the gather).  Ranks share cuda:0
and meet over gloo, as in tests/test_distributed_gpu.py; what they produce is held against pipeline.assemble_resident(filter_fp=True)
of one process on the same reads: texts, logs (the integer hits of every transcript) and counters are EQUAL, there is no tolerance --
the union over the ranks of what each rank's pairs cover is the one-process bitmap.  Then the command line: -p 2 against one process."""
import json, os, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,n_genes,seed,port,big,ss", [(2, 12, 4, 29671, False, False), (3, 12, 4, 29672, False, True),
                                                            (2, 40, 8, 29673, True, False)])
def test_filtered_ranks_equal_the_filtered_single_process(world, n_genes, seed, port, big, ss, tmp_path):
    from shannon_amd import device, synth, pipeline, kmers_for_component as kfc
    n_pairs = 12000
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    if big:
        env["SHN_CONTIG_GPU"] = "1"
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_filter_fp_worker.py"),
                        str(n_genes), str(seed), str(n_pairs), out] + (["ss"] if ss else []),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    got = json.load(open(out))
    (q1, q2), _ = synth.make_dataset(n_pairs, n_genes, seed=seed)
    ctx = device.Context(0)
    d1, d2 = device.Reads.from_codes(ctx, q1), device.Reads.from_codes(ctx, q2)
    try:
        ref = pipeline.assemble_resident(ctx, d1, d2, kfc.ReadStore(q1, q2), K=25, sample="t", seed=1, double_stranded=not ss, filter_fp=True)
    finally:
        d1.close()
        d2.close()
        ctx.close()
    assert list(got["partitions"]) == list(ref.partitions) and len(ref.partitions) > 0
    for name, rec in ref.partitions.items():
        assert got["filter_logs"][name] == rec["filter_log"], name                # name, hits, length of every transcript
        assert got["partitions_org"][name] == rec["reconstructed_org_fasta"], name
        assert got["partitions"][name] == rec["reconstructed_fasta"], name
    assert got["final"] == ref.final
    assert got["filter_fp_stats"] == ref.filter_fp_stats
    # ... and none of this is vacuous
    st = got["filter_fp_stats"]
    print("filter_fp_stats %s; per rank %s" % (st, got["local"]))
    assert sum(1 for l in got["local"] if l and l.get("placed", 0) > 0) >= 2
    assert sum(l["placed"] for l in got["local"]) == st["placed"] and sum(l["routes"] for l in got["local"]) == st["routes"]
    assert 0 < st["kept"] < st["transcripts"]
    assert {"filter_FP", "x:filter_FP texts", "x:filter_FP coverage"} <= set(got["timings"])


def _cli(tmp_path, tag, args, env_extra=None):
    os.makedirs(str(tmp_path / tag))
    out = str(tmp_path / tag / "OUT")                      # (the records are named after the output directory: one name for both runs)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", out] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=dict(os.environ, **(env_extra or {})), timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return out, p.stdout


def test_cli_filter_on_two_ranks_equals_the_one_process_cli(tmp_path):
    """shannon.py --left --right --filter_FP, once plain and once with -p 2: shannon.fasta, the three files of every partition and
    the summary line are the same"""
    from golden_util import GOLD, meta
    from shannon_amd import synth
    z = np.load(os.path.join(GOLD, "data", meta("syn_pe_s0")["inputs"][0]))
    f1, f2 = str(tmp_path / "r1.fasta"), str(tmp_path / "r2.fasta")
    synth.write_fasta(f1, z["r1"], "/1")
    synth.write_fasta(f2, z["r2"], "/2")
    args = ["-K", "25", "--left", f1, "--right", f2, "--filter_FP"]
    one, log_one = _cli(tmp_path, "one", args)
    ranks, log_ranks = _cli(tmp_path, "ranks", args + ["-p", "2"], {"SHN_CLI_BACKEND": "gloo"})
    assert "2 ranks" in log_ranks and "NOT filtered" not in log_ranks
    assert open(os.path.join(one, "shannon.fasta")).read() == open(os.path.join(ranks, "shannon.fasta")).read() != ""

    def partition_dirs(out):
        return {d: os.path.join(out, "TEMP", d) for d in os.listdir(os.path.join(out, "TEMP"))
                if d.endswith("algo_output") and not d.endswith("_allalgo_output")}
    a, b = partition_dirs(one), partition_dirs(ranks)
    assert sorted(a) == sorted(b) and len(a) > 0
    dropped = 0
    for d in a:
        texts = [[open(os.path.join(out, f)).read() for f in ("reconstructed.fasta", "reconstructed_org.fasta", "rec.log")] for out in (a[d], b[d])]
        assert texts[0] == texts[1], d
        dropped += texts[0][1].count(">") - texts[0][0].count(">")
    assert dropped > 0

    def summary(log):                                      # the line behind its timestamp
        lines = [l for l in log.splitlines() if "--filter_FP:" in l and "routed fragments placed" in l]
        assert len(lines) == 1, lines
        return lines[0][lines[0].index("--filter_FP:"):]
    assert summary(log_one) == summary(log_ranks)
