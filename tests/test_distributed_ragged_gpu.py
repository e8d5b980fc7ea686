"""GPU: shannon.py -p N on reads of different lengths and on mates of two lengths -- the ranks (sharing cuda:0, collectives over
gloo: SHN_CLI_BACKEND=gloo) against the one-process CLI on the same files, which test_e2e_gpu.py::test_end_to_end_at_read_lengths
holds to the oracle.  The inputs are that test's (_lengths_case): 5 transcripts of synth.make_transcriptome(seed=61), 1,200 pairs,
read lengths drawn from 30-150, or 100 / 80 for the mates; -K 25 --partition 2: the inputs give 16 contigs (8 with -s) in components
of at most 10, so --partition 8 or 4 would leave 1 or 2 partitions; --partition 2 gives 9 (5 with -s), and more than one rank owns
some -- every case asserts that there are at least 4.  The reads of a partition then travel with their lengths (exchange.RaggedPiece), collected from the
resident sets by shn_reads_collect ("collect path": "device") or, with SHN_COLLECT_DEVICE=0, on the host."""
import os, re, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

COMMON = ["-K", "25", "--partition", "2"]


def _write(path, seqs, suffix):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">read_%d%s\n%s\n" % (i, suffix, s))
    return path


def _cli(base, tag, args, env_extra=None):
    os.makedirs(os.path.join(base, tag))
    out = os.path.join(base, tag, "OUT")                   # (the records are named after the output directory: one name for all runs)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", out] + COMMON + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=dict(os.environ, **(env_extra or {})), timeout=600)
    return p.returncode, out, p.stdout


def _products(out):
    recs = open(os.path.join(out, "shannon.fasta")).read().split(">")[1:]
    contigs = open(os.path.join(out, "TEMP", "OUT_algo_input", "k1mer.dict_contig")).read()
    return sorted(r.split("\n", 1)[1] for r in recs), contigs


def _partition_files(out):
    dirs = sorted(d for d in os.listdir(os.path.join(out, "TEMP")) if d.endswith("algo_output") and not d.endswith("_allalgo_output"))
    return {d: [open(os.path.join(out, "TEMP", d, f)).read() for f in ("reconstructed.fasta", "reconstructed_org.fasta", "rec.log")] for d in dirs}


class _Inputs(object):
    """the read files, and the one-process run of every (input, flags) a case asks for -- run once, kept for the module"""

    def __init__(self, base):
        from shannon_amd import synth
        self.base = base
        A = np.frombuffer(b"ACGT", np.uint8)
        txt = lambda rows: [A[r].tobytes().decode() for r in rows]
        iso, _ = synth.make_transcriptome(5, seed=61)
        iso = [t for t in iso if len(t) >= 300]
        r1, r2 = synth.sample_pairs(iso, 1200, 62, read_len=150, frag_len=300, err=0.003)
        rng = np.random.RandomState(63)                                   # ragged: 30-150 bases, the mates of a pair of different lengths
        s1 = [t[:rng.randint(30, 151)] for t in txt(r1)]
        s2 = [t[:rng.randint(30, 151)] for t in txt(r2)]
        f = lambda name: os.path.join(base, name)
        self.files = {
            "ragged": ["--left", _write(f("rag1.fasta"), s1, "/1"), "--right", _write(f("rag2.fasta"), s2, "/2")],
            "ragged_single": ["--single", _write(f("rag.fasta"), s1 + s2, "")],
            "mates_differ": ["--left", _write(f("md1.fasta"), txt(r1[:, :100]), "/1"), "--right", _write(f("md2.fasta"), txt(r2[:, :80]), "/2")],
        }
        (q1, q2), _ = synth.make_dataset(12000, 12, seed=4)             # the input of test_cli_ranks_equal_the_one_process_cli
        f1, f2 = f("fix1.fasta"), f("fix2.fasta")
        synth.write_fasta(f1, q1, "/1")
        synth.write_fasta(f2, q2, "/2")
        self.files["fixed"] = ["--left", f1, "--right", f2]
        self._one, self._n = {}, 0

    def run(self, name, flags, ranks=0, env=None):
        """(exit code, OUT, log) of one launch"""
        self._n += 1
        extra = ["-p", str(ranks)] if ranks else []
        return _cli(self.base, "run%d" % self._n, self.files[name] + list(flags) + extra, dict(env or {}, SHN_CLI_BACKEND="gloo") if ranks else env)

    def one_process(self, name, flags):
        key = (name, tuple(flags))
        if key not in self._one:
            rc, out, log = self.run(name, flags)
            assert rc == 0, log[-3000:]
            self._one[key] = (out, log)
        return self._one[key]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return _Inputs(str(tmp_path_factory.mktemp("ragged_ranks")))


def _n_partitions(log):
    m = re.search(r"(\d+) contigs; (\d+) partitions", log)
    assert m, log[-2000:]
    return int(m.group(2))


def _ranks_equal_one_process(inputs, name, flags, world, env=None, path="device"):
    one, _log = inputs.one_process(name, flags)
    rc, out, log = inputs.run(name, flags, ranks=world, env=env)
    assert rc == 0, log[-3000:]
    assert "%d ranks" % world in log
    assert _n_partitions(log) >= 4, "the job must have partitions for more than one rank"
    want, got = _products(one), _products(out)
    assert got[1] == want[1]
    assert got[0] == want[0] and len(want[0]) > 0
    assert '"collect path": "%s"' % path in log, log[-1500:]
    return one, out, log


@pytest.mark.parametrize("name,flags,world", [("ragged", [], 2), ("ragged_single", [], 3), ("ragged", ["-s"], 2), ("mates_differ", [], 2),
                                              ("mates_differ", ["-s"], 2)],
                         ids=["ragged-p2", "ragged-single-p3", "ragged-s-p2", "mates_differ-p2", "mates_differ-s-p2"])
def test_ranks_take_reads_of_any_lengths(inputs, name, flags, world):
    _ranks_equal_one_process(inputs, name, flags, world)


def test_filter_fp_on_ranks_with_reads_of_different_lengths(inputs):
    """--filter_FP -p 2 on the ragged pairs: beside the products, every partition's reconstructed.fasta, reconstructed_org.fasta and
    rec.log are the one-process run's, byte for byte"""
    one, out, log = _ranks_equal_one_process(inputs, "ragged", ["--filter_FP"], 2)
    assert "NOT filtered" not in log
    a, b = _partition_files(one), _partition_files(out)
    assert sorted(a) == sorted(b) and len(a) >= 4
    for d in a:
        assert a[d] == b[d], d


def test_the_host_collect_gives_the_same(inputs):
    """SHN_COLLECT_DEVICE=0: the pieces with lengths gathered from the host copies (ReadStore.gather_codes)"""
    _ranks_equal_one_process(inputs, "ragged", [], 2, env={"SHN_COLLECT_DEVICE": "0"}, path="host")


def test_the_device_collect_gives_the_same_rows_for_reads_of_one_length(inputs):
    """SHN_COLLECT_DEVICE=1 on reads of one length: the rows come from the resident sets instead of the host matrices, the run's
    products are those of the switch unset (the host gather, as ever)"""
    runs = {}
    for tag, env, path in (("unset", {}, "host"), ("device", {"SHN_COLLECT_DEVICE": "1"}, "device")):
        env = dict({k: v for k, v in os.environ.items() if k != "SHN_COLLECT_DEVICE"}, SHN_CLI_BACKEND="gloo", **env)
        os.makedirs(os.path.join(inputs.base, "fixed_" + tag))
        out = os.path.join(inputs.base, "fixed_" + tag, "OUT")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "shannon.py"), "-o", out, "-K", "25"] + inputs.files["fixed"] + ["-p", "2"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        assert '"collect path": "%s"' % path in p.stdout
        runs[tag] = _products(out)
    assert runs["unset"] == runs["device"] and len(runs["unset"][0]) > 0
