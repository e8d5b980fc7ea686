"""bench.py --dump-outputs: the final transcripts of the last timed step as .npy arrays (float32 / float64, at most 64 MB; a fixed,
seeded sample where the whole output would not fit), the same arrays from run to run; and a plain run (no --full) prints the
headline line without the extra measurements."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("transcript_lengths", "transcript_name_lengths", "sample_index", "sample_bases", "sample_names")


def _load(d):
    return {nm: np.load(os.path.join(d, nm + ".npy")) for nm in NAMES}


def _transcripts(A):
    """the sampled transcripts back as {name: sequence}"""
    idx = A["sample_index"].astype(np.int64)
    so = np.concatenate([[0], np.cumsum(A["transcript_lengths"][idx])]).astype(np.int64)
    no = np.concatenate([[0], np.cumsum(A["transcript_name_lengths"][idx])]).astype(np.int64)
    seqs = np.frombuffer(b"ACGTN", np.uint8)[A["sample_bases"].astype(np.int64)].tobytes().decode()
    names = A["sample_names"].astype(np.uint8).tobytes().decode()
    return {names[no[i]:no[i + 1]]: seqs[so[i]:so[i + 1]] for i in range(len(idx))}


def test_dump_holds_the_transcripts_and_a_fixed_sample_within_the_cap(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    final = {"comp%d_%d_0" % (i, i % 7): "".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(100, 3000)))) for i in range(300)}
    bench.dump_outputs(final, str(tmp_path / "all"))
    A = _load(str(tmp_path / "all"))
    assert all(A[nm].dtype in (np.float32, np.float64) for nm in NAMES)
    assert np.array_equal(A["sample_index"], np.arange(300)) and _transcripts(A) == final
    cap = bench.DUMP_BYTES
    try:
        bench.DUMP_BYTES = 200_000
        bench.dump_outputs(final, str(tmp_path / "a"))
        bench.dump_outputs(final, str(tmp_path / "b"))
    finally:
        bench.DUMP_BYTES = cap
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / (nm + ".npy"))) for nm in NAMES) <= 200_000
    assert 0 < len(a["sample_index"]) < 300 and all(np.array_equal(a[nm], b[nm]) for nm in NAMES)
    assert np.array_equal(a["transcript_lengths"], A["transcript_lengths"])
    got = _transcripts(a)
    assert got == {k: final[k] for k in got}


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genes", "200", "--reads", "1000000", "--K", "25",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", out_dir],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_computed(tmp_path):
    one = _bench(str(tmp_path / "one"))
    assert one["steps"] == 2 and one["warmup"] == 1 and one["ms_per_step"] > 0
    assert not any(k in one for k in ("cpu_baseline", "ingest", "value_with_ingest", "overlap"))
    A = _load(str(tmp_path / "one"))
    assert len(A["transcript_lengths"]) == one["config"]["transcripts"] > 0
    assert len(A["sample_index"]) == len(A["transcript_lengths"])              # a small output is written out whole
    seqs = sorted(_transcripts(A).values())                                     # bench._final_sha of the dumped transcripts
    h = hashlib.sha256()
    for sq in seqs:
        h.update(sq.encode() + b"\n")
    assert h.hexdigest()[:16] == one["config"]["transcripts_sha256_16"]
    two = _bench(str(tmp_path / "two"))
    B = _load(str(tmp_path / "two"))
    assert all(np.array_equal(A[nm], B[nm]) for nm in NAMES)
