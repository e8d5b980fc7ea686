"""CPU, world 4 (gloo): the N-rank CLI's ingest by BYTES of the read files for reads of different lengths
(distributed.ingest_rank_slice(..., ragged=True)) -- every rank holds the records [n r / W, n (r + 1) / W) of each file as
device.RaggedCodes, looks at no more than its share of the bytes, and a file that is ragged in one rank's share only still gives
every rank the same kind of store."""
import json, os, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT

W = 4


def _write(path, lens, fastq, seed):
    rng = np.random.default_rng(seed)
    A = np.frombuffer(b"ACGTN", np.uint8)
    with open(path, "w") as f:
        for i, L in enumerate(lens):
            codes = rng.integers(0, 4, L, dtype=np.uint8)
            codes[rng.random(L) < 0.001] = 4                                 # a few N
            name = "read_%d%s" % (i, "_x" * int(rng.integers(0, 6)))             # names of different lengths
            s = A[codes].tobytes().decode()
            if fastq:
                q = "".join("@+I#"[int(v)] for v in rng.integers(0, 4, L))       # quality lines that start with '@' or '+'
                f.write("@%s\n%s\n+\n%s\n" % (name, s, q))
            else:
                f.write(">%s\n%s\n" % (name, s))
    return path


def _run(out, paths, port):
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(W), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "ingest_ragged_worker.py"), out] + paths,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]


def _check_slices(out, paths, n, bound=True):
    from shannon_amd import device
    whole = [device.Reads.ingest(None, p)[1] for p in paths]
    assert all(isinstance(w, device.RaggedCodes) and len(w) == n for w in whole)
    total = sum(os.path.getsize(p) for p in paths)
    for r in range(W):
        st = json.load(open("%s.rank%d.json" % (out, r)))
        assert not st.get("declined") and st["n"] == n and st["file_bytes"] == total
        assert st["kinds"] == ["ragged"] * len(paths), (r, st)
        z = np.load("%s.rank%d.npz" % (out, r))
        lo, hi = r * n // W, (r + 1) * n // W
        for i, w in enumerate(whole):
            codes, off = z["codes%d" % i], z["off%d" % i]
            assert off.dtype == np.uint64 and len(off) == hi - lo + 1 and int(off[0]) == 0
            assert np.array_equal(off, w.off[lo:hi + 1] - w.off[lo]), (r, i)     # the records [n r / W, n (r + 1) / W) of the file, in order
            assert np.array_equal(codes[:int(off[-1])], w.codes[int(w.off[lo]):int(w.off[hi])]), (r, i)
        if bound:
            # its share of the bytes once to count and once to parse (+ the records between a share's start and its slice's)
            assert st["bytes_scanned"] <= 1.2 * 2 * total / W, (r, st)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_ranks_keep_their_share_of_reads_of_different_lengths(tmp_path, fastq):
    n = 4001
    lens = [80 + 4 * (i % 3) for i in range(n)]
    paths = [_write(str(tmp_path / ("r%d.%s" % (m, "fastq" if fastq else "fasta"))), lens if m == 1 else lens[::-1], fastq, 10 * m + fastq) for m in (1, 2)]
    out = str(tmp_path / "o")
    _run(out, paths, 29661 + int(fastq))
    _check_slices(out, paths, n)


def test_a_file_that_is_ragged_in_one_share_only(tmp_path):
    """the first 3,000 records have one length: three ranks parse a matrix, the last one does not -- every rank ends with RaggedCodes"""
    n = 4001
    lens = [84] * 3000 + [80 + 4 * (i % 3) for i in range(n - 3000)]
    paths = [_write(str(tmp_path / "r.fasta"), lens, False, 5)]
    out = str(tmp_path / "o")
    _run(out, paths, 29663)
    _check_slices(out, paths, n)


def test_two_lengths_that_meet_on_a_share_boundary(tmp_path):
    """every rank parses a matrix, of 80 bases on two ranks and of 100 on the others: still one ragged store on every rank; and the plain
    call (ragged=False) goes on declining such a file (tests/test_ingest_ranks.py holds that for the ragged file)"""
    n = 4000
    # (records of one name length: the byte shares then fall where the record shares do, up to a few records either way)
    lens = [80] * 2000 + [100] * 2000
    p = str(tmp_path / "r.fasta")
    rng = np.random.default_rng(9)
    with open(p, "w") as f:
        for i, L in enumerate(lens):
            f.write(">r%05d\n%s\n" % (i, "".join("ACGT"[c] for c in rng.integers(0, 4, L))))
    out = str(tmp_path / "o")
    _run(out, [p], 29664)
    _check_slices(out, [p], n, bound=False)
