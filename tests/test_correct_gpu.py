"""GPU: python -m shannon_amd.correct.  shn_reads_slice against numpy; the spans of shn_quorum_correct_spans, the
trimming and the command against the brute force of tests/correct_cases.py; tables added up against the table of all sets resident;
lanes and ranks against the one-process run on the concatenated files; the untrimmed command against `shannon.py --quorum`.
Everything is integers or bytes and compared exactly."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT
import quorum_cases as qc
import correct_cases as cc

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", np.uint8)
CODE = {c: i for i, c in enumerate("ACGTN")}


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def collect_strings(d):
    """the reads of a resident set as strings over ACGTN (Reads.collect: codes and lengths)"""
    from shannon_amd import device
    n = len(d)
    codes, off = device.Reads.collect(d, None, np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
    return [LETTERS[np.minimum(codes[int(off[i]):int(off[i + 1])], 4)].tobytes().decode() for i in range(n)]


def ragged_set(ctx, strings):
    from shannon_amd import device
    codes = np.array([CODE[c] for s in strings for c in s], dtype=np.uint8)
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return device.Reads.from_ragged(ctx, codes, off)


def fixed_set(ctx, strings):
    from shannon_amd import device
    return device.Reads.from_codes(ctx, np.array([[CODE[c] for c in s] for s in strings], dtype=np.uint8).reshape(len(strings), len(strings[0])))


def table_pairs(t):
    keys, cnts = t.download()
    order = np.argsort(keys)
    return keys[order].tolist(), cnts[order].tolist()


def counted(ctx, d):
    from shannon_amd import device
    t = device.count_k1mers(ctx, [d], 24)
    try:
        return table_pairs(t), t.total
    finally:
        t.close()


def check_slice(ctx, src, strings, spans, keep_min=None):
    """shn_reads_slice of `src` (whose reads are `strings`) under `spans` -- with keep_min, of the reads rule 7 keeps at that M --
    against Python slices: collected codes and lengths, the reads with a base outside ACGT, the counted 24-mers (stray bits behind
    a read's end would show there), and the source afterwards"""
    from shannon_amd import quorum, _lib
    sp = quorum.QSpans.from_array(ctx, spans)
    try:
        if keep_min is None:
            want = [s[lo:hi] for s, (lo, hi) in zip(strings, spans)]
            got = quorum.slice_reads(ctx, src, sp)
        else:
            want = [s[lo:hi] for s, (lo, hi) in zip(strings, spans) if hi - lo >= keep_min]
            out, st = quorum.trim(ctx, [src], [sp], keep_min)
            got = out[0]
            assert st["kept"] == len(want) and st["below_min"] == len(strings) - len(want) and st["pairs_dropped"] == 0
            assert st["bases_cut"] == sum(len(s) - (hi - lo) for s, (lo, hi) in zip(strings, spans) if hi - lo >= keep_min)
        try:
            assert len(got) == len(want)
            assert collect_strings(got) == want
            assert got.n_invalid == sum(1 for w in want if "N" in w)
            assert got.max_len == max([len(w) for w in want] + [0])
            assert int(_lib.lib().shn_reads_total_bases(got.h)) == sum(len(w) for w in want)
            if want:                                              # (a set of 0 reads has nothing to count)
                ref = ragged_set(ctx, want)
                try:
                    assert counted(ctx, got) == counted(ctx, ref)
                finally:
                    ref.close()
        finally:
            got.close()
        assert collect_strings(src) == strings
    finally:
        sp.close()


# ---------------------------------------------------------------------------------------------------------------- 1. the slice
SRC_LENS = (1, 31, 32, 33, 63, 64, 65, 96, 129, 200)
OUT_LENS = (1, 31, 32, 33, 63, 64, 65)


def _with_n(rng, L, lo, hi):
    """a random read of L bases with an N at lo - 1, lo, hi - 1, hi and inside the span, where those exist"""
    s = [rng.choice("ACGT") for _ in range(L)]
    for p in (lo - 1, lo, hi - 1, hi, (lo + hi) // 2):
        if 0 <= p < L and rng.random() < 0.6:
            s[p] = "N"
    return "".join(s)


def slice_cases():
    """(strings, spans) of a ragged source: every source length with every lo of 0 .. 65 and every output length that fits"""
    rng = random.Random(11)
    strings, spans = [], []
    for L in SRC_LENS:
        for lo in range(0, 66):
            for n in OUT_LENS:
                if lo + n <= L:
                    strings.append(_with_n(rng, L, lo, lo + n))
                    spans.append((lo, lo + n))
    return strings, spans


def test_slice_ragged_source_every_offset_and_length(ctx):
    strings, spans = slice_cases()
    assert {lo % 32 for lo, _h in spans} >= {0, 1, 31} and {lo % 64 for lo, _h in spans} >= {0, 1, 33, 63} and len(strings) > 1000
    src = ragged_set(ctx, strings)
    try:
        check_slice(ctx, src, strings, spans)
    finally:
        src.close()


@pytest.mark.parametrize("L", SRC_LENS)
def test_slice_fixed_length_source(ctx, L):
    rng = random.Random(L)
    strings, spans = [], []
    for lo in range(0, min(L, 66)):
        for n in OUT_LENS + (L - lo,):
            if 0 < n and lo + n <= L:
                strings.append(_with_n(rng, L, lo, lo + n))
                spans.append((lo, lo + n))
    src = fixed_set(ctx, strings)
    try:
        check_slice(ctx, src, strings, spans)
    finally:
        src.close()


def test_slice_random_reads_some_not_kept(ctx):
    """about 2,000 reads: reads and output words cross the blocks; the first read, the last read and a run of neighbours are not kept"""
    rng = random.Random(12)
    strings, spans = [], []
    for i in range(2000):
        L = rng.randrange(30, 260)
        lo = rng.randrange(0, L - 24)
        hi = rng.randrange(lo + 24, L + 1)
        if i in (0, 1999) or 700 <= i < 740 or rng.random() < 0.1:
            hi = lo + rng.randrange(0, 24)                          # below M = 24: not kept
        strings.append(_with_n(rng, L, lo, hi))
        spans.append((lo, hi))
    src = ragged_set(ctx, strings)
    try:
        check_slice(ctx, src, strings, spans, keep_min=24)
        check_slice(ctx, src, strings, [(lo, lo + min(hi - lo, 23)) for lo, hi in spans], keep_min=24)      # the empty selection: a set of 0 reads
    finally:
        src.close()


def test_slice_refusals(ctx):
    from shannon_amd import quorum, _lib
    strings = ["ACGT" * 10, "TTGCA" * 6]
    src, fix = ragged_set(ctx, strings), fixed_set(ctx, ["ACGT" * 10] * 2)
    try:
        with pytest.raises(_lib.ShannonError, match="lo > hi"):
            quorum.QSpans.from_array(ctx, [(5, 4), (0, 1)])
        three = quorum.QSpans.from_array(ctx, [(0, 1)] * 3)
        with pytest.raises(_lib.ShannonError, match="spans of 3 reads, a set of 2"):
            quorum.slice_reads(ctx, src, three)
        with pytest.raises(_lib.ShannonError, match="not of their set's read count"):
            quorum.trim(ctx, [src], [three], 1)
        beyond = quorum.QSpans.from_array(ctx, [(0, 41), (0, 1)])
        for d in (src, fix):
            with pytest.raises(_lib.ShannonError, match="hi 41 beyond the reads' length 40"):
                quorum.slice_reads(ctx, d, beyond)
        ok = quorum.QSpans.from_array(ctx, [(0, 40), (0, 30)])
        with pytest.raises(_lib.ShannonError, match="min_len is 0"):
            quorum.trim(ctx, [src], [ok], 0)
        # a span that ends inside the set's longest read but beyond its own: the host cannot know, the kernel holds it inside the read
        inside = quorum.QSpans.from_array(ctx, [(0, 40), (10, 40)])
        got = quorum.slice_reads(ctx, src, inside)
        assert collect_strings(got) == [strings[0], strings[1][10:30]]
        got.close()
        for s in (three, beyond, ok, inside):
            s.close()
        assert collect_strings(src) == strings
    finally:
        src.close()
        fix.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the spans
class Ingested(object):
    def __init__(self, ctx, files, q=qc.Q):
        from shannon_amd import device, quorum
        self.texts = [qc.fastq_text(reads).encode() for reads in files]
        self.sets = [device.Reads.ingest(ctx, t, want_codes=False)[0] for t in self.texts]
        self.masks = [quorum.hq_mask(ctx, d, t, q) for d, t in zip(self.sets, self.texts)]

    def close(self):
        for x in self.masks + self.sets:
            x.close()


def check_spans(ctx, files):
    from shannon_amd import quorum
    want = cc.brute_run(files)
    I = Ingested(ctx, files)
    try:
        t = quorum.trusted_table(ctx, I.sets, I.masks)
        stats = dict.fromkeys(qc.STAT_NAMES, 0)
        for f, d in enumerate(I.sets):
            c, st, sp = quorum.correct(ctx, d, t, spans=True)
            plain, st0 = quorum.correct(ctx, d, t)
            try:
                got = sp.download()
                assert [tuple(int(v) for v in row) for row in got] == [(r["lo"], r["hi"]) for r in want["reads"][f]]
                assert collect_strings(c) == want["files"][f] == collect_strings(plain) and st == st0
                for n in qc.STAT_NAMES:
                    stats[n] += st[n]
            finally:
                c.close(); plain.close(); sp.close()
        assert stats == {n: want["stats"][n] for n in qc.STAT_NAMES}
        t.close()
    finally:
        I.close()
    return want


@pytest.mark.parametrize("name", qc.SCENARIOS)
def test_spans_of_every_scenario(ctx, name):
    check_spans(ctx, qc.scenario(name)["files"])


def test_spans_ragged_and_planted(ctx):
    check_spans(ctx, qc.ragged_case())
    check_spans(ctx, qc.planted_case()[0])
    check_spans(ctx, cc.trim_case()[0])


# ---------------------------------------------------------------------------------------------------------------- 3. tables added
def check_added(ctx, parts):
    """the tables of `parts` (lists of files) added up hold what the table over all their sets resident holds; no part's table does"""
    from shannon_amd import quorum
    I = [Ingested(ctx, files) for files in parts]
    try:
        whole = quorum.trusted_table(ctx, [s for i in I for s in i.sets], [m for i in I for m in i.masks])
        singles = [quorum.trusted_table(ctx, i.sets, i.masks) for i in I]
        total = singles[0]
        for t in singles[1:]:
            both = quorum.add_tables(ctx, total, t)
            if total is not singles[0]:
                total.close()
            total = both
        assert table_pairs(total) == table_pairs(whole) and total.total == whole.total and total.k == whole.k and total.canonical
        keys = np.array(table_pairs(whole)[0], dtype=np.uint64)
        assert total.lookup(keys).tolist() == whole.lookup(keys).tolist()
        for t in singles:
            assert table_pairs(t) != table_pairs(whole)
        want = qc.brute_table([f for files in parts for f in files])
        assert len(want) == len(whole) and sum(want.values()) == total.total
        for t in singles + [whole] + ([total] if total is not singles[0] else []):
            t.close()
    finally:
        for i in I:
            i.close()


def test_tables_added_up(ctx):
    lanes, _probe, _clean = cc.lane_effect_case()
    check_added(ctx, [[lanes[0]], [lanes[1]]])
    f = qc.scenario("mates_two_lengths")["files"]
    check_added(ctx, [[f[0]], [f[1]]])


# ---------------------------------------------------------------------------------------------------------------- the command
def run_correct(argv, capsys=None):
    """the command in this process; (exit code, stdout, stderr)"""
    from shannon_amd import correct
    if capsys is not None:
        capsys.readouterr()
    rc = correct.main(["correct"] + [str(a) for a in argv])
    cap = capsys.readouterr() if capsys is not None else None
    return rc, (cap.out if cap else ""), (cap.err if cap else "")


def files_under(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


def log_lines(d, skip=("quorum kernels: ",)):
    return [l for l in open(os.path.join(str(d), "correct_log.txt")).read().splitlines() if not l.startswith(skip)]


def same_outputs(a, b, lanes_differ=False):
    """every file under a and b byte for byte, but the log's kernel line (and, where the lanes differ, its lane lines)"""
    fa, fb = files_under(a), files_under(b)
    assert sorted(fa) == sorted(fb)
    for f in fa:
        if f != "correct_log.txt":
            assert fa[f] == fb[f], f
    drop = ("quorum kernels: ", "lane ") if lanes_differ else ("quorum kernels: ",)
    assert log_lines(a, drop) == log_lines(b, drop)


CORRECTED = re.compile(r"corrected: (\d+) of (\d+) reads anchored, (\d+) changed, (\d+) substitutions, (\d+) stopped directions, (\d+) window reverts")
QUORUM = re.compile(r"--quorum: .*: (\d+) of (\d+) reads anchored, (\d+) changed, (\d+) substitutions, (\d+) stopped directions, (\d+) window reverts; "
                    r"table of (\d+) k-mers from (\d+) high-quality windows")
TABLE = re.compile(r"table: (\d+) k-mers from (\d+) high-quality windows")
TRIMMED = re.compile(r"trimmed: (\d+) reads kept, (\d+) of them trimmed, (\d+) bases cut from kept reads, (\d+) reads with a span below (\d+), (\d+) pairs dropped")


def log_counters(d):
    text = open(os.path.join(str(d), "correct_log.txt")).read()
    return [int(x) for x in CORRECTED.search(text).groups()] + [int(x) for x in TABLE.search(text).groups()]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted pairs as FASTQ files, whole and in 3 lanes of unequal size, and `shannon.py --quorum` on the whole files (paired
    and single-end)"""
    import shannon
    files, _clean = qc.planted_case()
    d = tmp_path_factory.mktemp("correct_cli")
    lanes, whole = cc.write_lanes(str(d), "planted", files, (50, 330))
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SHN_MALLOC_TUNE", "0")
        for name, argv in (("paired", ["--left", whole[0], "--right", whole[1]]), ("single", ["--single", whole[0]])):
            out = d / ("shannon_" + name)
            assert shannon.main(["shannon.py", "-o", str(out), "--quorum"] + argv) == 0
            hit = [QUORUM.search(l) for l in (out / "log.txt").read_text().splitlines() if "--quorum: " in l][0]
            runs[name] = {"out": out, "counters": [int(x) for x in hit.groups()]}
    noisy_lanes, noisy_whole = cc.write_lanes(str(d), "noisy", cc.noisy_tail_pairs(), (200,))
    return {"dir": d, "files": files, "lanes": lanes, "whole": whole, "runs": runs, "noisy_lanes": noisy_lanes, "noisy_whole": noisy_whole}


def test_command_one_lane_is_shannon_quorum(ctx, planted, capsys):
    """4. one lane, no trim: the files are TEMP/corrected_reads*.fa of `shannon.py --quorum` on the same files, the counters its log line's"""
    d, whole = planted["dir"], planted["whole"]
    for name, argv in (("paired", ["--left", whole[0], "--right", whole[1]]), ("single", ["--single", whole[0]])):
        out = d / ("one_" + name)
        rc, printed, err = run_correct(["-o", out] + argv, capsys)
        assert rc == 0, err
        temp = planted["runs"][name]["out"] / "TEMP"
        names = sorted(p.name for p in temp.glob("corrected_reads*"))
        assert names == (["corrected_reads_1.fa", "corrected_reads_2.fa"] if name == "paired" else ["corrected_reads.fa"])
        assert sorted(os.listdir(str(out))) == sorted(names + ["correct_log.txt"])
        for f in names:
            assert (out / f).read_bytes() == (temp / f).read_bytes(), f
        assert log_counters(out) == planted["runs"][name]["counters"]
        log = (out / "correct_log.txt").read_text()
        assert "parameters: k 24, quality 5, anchor count 3, 3 substitutions in a window of 10\n" in log and "lane 1: " in log
        assert all(('"%s"' % g) in log for g in ("quorum.count", "quorum.table", "quorum.correct"))


def test_command_lanes(ctx, planted, capsys, tmp_path):
    """5. lanes: every file is that of the run on the concatenated files (the test that fails when tables are not added up)"""
    lanes = planted["lanes"]
    rc, _o, err = run_correct(["-o", tmp_path / "lanes", "--left", ",".join(lanes[0]), "--right", ",".join(lanes[1])], capsys)
    assert rc == 0, err
    same_outputs(tmp_path / "lanes", _one(planted, capsys, tmp_path), lanes_differ=True)
    assert len([l for l in log_lines(tmp_path / "lanes") if l.startswith("lane ")]) == 3
    # ragged reads in 2 lanes
    rl, rw = cc.write_lanes(str(tmp_path / "in"), "ragged", qc.ragged_case(), (1700,))
    assert run_correct(["-o", tmp_path / "r2", "--single", ",".join(rl[0])], capsys)[0] == 0
    assert run_correct(["-o", tmp_path / "r1", "--single", rw[0]], capsys)[0] == 0
    same_outputs(tmp_path / "r2", tmp_path / "r1", lanes_differ=True)
    # the lane effect: the brute force over both lanes, which is not the brute force lane by lane
    le, probe, clean = cc.lane_effect_case()
    paths = [cc.write_fastq(str(tmp_path / ("le%d.fq" % i)), l) for i, l in enumerate(le)]
    assert run_correct(["-o", tmp_path / "le", "--single", ",".join(paths)], capsys)[0] == 0
    want = cc.brute_run([le[0] + le[1]])
    apart = [cc.brute_run([l]) for l in le]
    got = (tmp_path / "le" / "corrected_reads.fa").read_text()
    assert got == cc.expected_texts(want)["corrected_reads.fa"] != cc.fasta_of(apart[0]["files"][0] + apart[1]["files"][0])
    assert got.splitlines()[2 * len(le[0]) + 1] == clean
    st = want["stats"]
    assert log_counters(tmp_path / "le") == [st["anchored"], len(le[0]) + len(le[1]), st["changed"], st["substitutions"], st["stopped"], st["reverts"],
                                             st["table"], st["windows"]]


def _one(planted, capsys, tmp_path):
    whole = planted["whole"]
    assert run_correct(["-o", tmp_path / "one", "--left", whole[0], "--right", whole[1]], capsys)[0] == 0
    return tmp_path / "one"


def test_command_refuses(ctx, planted, capsys, tmp_path):
    """FASTA text, mates of different counts, a non-empty directory: exit code 2, a message, nothing written"""
    whole, lanes = planted["whole"], planted["lanes"]
    fa = tmp_path / "reads.fa"
    fa.write_text(qc.fasta_text([b for b, _q in planted["files"][0][:20]]))
    rc, _o, err = run_correct(["-o", tmp_path / "fa", "--single", fa], capsys)
    assert rc == 2 and "needs FASTQ text" in err and not (tmp_path / "fa").exists()
    rc, _o, err = run_correct(["-o", tmp_path / "mates", "--left", lanes[0][0] + "," + lanes[0][1], "--right", lanes[1][0] + "," + lanes[1][2]], capsys)
    assert rc == 2 and err.startswith("lane 2: ") and "not mates of each other" in err and not (tmp_path / "mates").exists()
    (tmp_path / "full").mkdir()
    (tmp_path / "full" / "x").write_text("x")
    rc, _o, err = run_correct(["-o", tmp_path / "full", "--single", whole[0]], capsys)
    assert rc == 2 and "not empty" in err
    gz = tmp_path / "r.fastq.gz"
    import gzip
    with gzip.open(str(gz), "wb") as f:
        f.write(open(whole[0], "rb").read())
    assert run_correct(["-o", tmp_path / "gz", "--single", gz], capsys)[0] == 0
    assert run_correct(["-o", tmp_path / "plain", "--single", whole[0]], capsys)[0] == 0
    same_outputs(tmp_path / "gz", tmp_path / "plain", lanes_differ=True)


# ---------------------------------------------------------------------------------------------------------------- 7. --trim
@pytest.fixture(scope="module")
def trim_files(tmp_path_factory):
    files, idx = cc.trim_case()
    d = tmp_path_factory.mktemp("correct_trim")
    return {"dir": d, "files": files, "idx": idx, "paths": [cc.write_fastq(str(d / ("t%d.fq" % (m + 1))), f) for m, f in enumerate(files)]}


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("min_len", [None, cc.TRIM_M, cc.TRIM_M - 1])
def test_command_trim(ctx, trim_files, capsys, tmp_path, paired, min_len):
    """the files and the five counters of rule 7 are the brute force's: the default M = k, the M of the boundary pair, and one below it"""
    P, files = trim_files["paths"], trim_files["files"] if paired else trim_files["files"][:1]
    argv = (["--left", P[0], "--right", P[1]] if paired else ["--single", P[0]]) + ["--trim"] + (["--min_len", min_len] if min_len else [])
    rc, _o, err = run_correct(["-o", tmp_path / "t"] + argv, capsys)
    assert rc == 0, err
    want = cc.brute_run(files, trim=True, min_len=min_len)
    for name, text in cc.expected_texts(want).items():
        assert (tmp_path / "t" / name).read_text() == text, name
    log = (tmp_path / "t" / "correct_log.txt").read_text()
    tr = want["trim"]
    assert [int(x) for x in TRIMMED.search(log).groups()] == [tr["kept"], tr["trimmed"], tr["bases_cut"], tr["below_min"], min_len or 24, tr["pairs_dropped"]]
    st = want["stats"]
    assert log_counters(tmp_path / "t") == [st["anchored"], sum(len(f) for f in files), st["changed"], st["substitutions"], st["stopped"], st["reverts"],
                                            st["table"], st["windows"]]
    i, j = trim_files["idx"]["span_m_minus_1"], trim_files["idx"]["span_m"]
    assert (i in want["kept"], j in want["kept"]) == ((False, True) if min_len == cc.TRIM_M else (True, True))
    if not paired and min_len is None:
        # a kept read whose span is the whole read is written as the run without --trim writes it
        assert run_correct(["-o", tmp_path / "u", "--single", P[0]], capsys)[0] == 0
        plain = (tmp_path / "u" / "corrected_reads.fa").read_text().splitlines()[1::2]
        whole = [i for i in want["kept"] if want["reads"][0][i]["hi"] - want["reads"][0][i]["lo"] == len(want["reads"][0][i]["text"])]
        assert len(whole) > 10 and all(want["files"][0][want["kept"].index(i)] == plain[i] for i in whole)


# ---------------------------------------------------------------------------------------------------------------- 6. ranks
def _ranks(argv, gpus, cwd):
    """the command with --gpus N as a fresh process: N ranks on GPU 0, collectives through host memory"""
    env = dict(os.environ, SHN_CLI_BACKEND="gloo", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SHN_CLI_LAUNCH_PROBE", None)
    return subprocess.run([sys.executable, "-m", "shannon_amd.correct"] + [str(a) for a in argv] + ["--gpus", str(gpus)], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, env=env, cwd=str(cwd), timeout=300)


@pytest.mark.parametrize("gpus,trim", [(2, False), (3, True)])
def test_ranks_planted_pairs_in_two_lanes(ctx, planted, capsys, tmp_path, gpus, trim):
    lanes = planted["noisy_lanes"] if trim else planted["lanes"]             # (with --trim: pairs of which some are cut and some dropped)
    argv = ["--left", lanes[0][0] + "," + lanes[0][1], "--right", lanes[1][0] + "," + lanes[1][1]] + (["--trim"] if trim else [])
    p = _ranks(["-o", tmp_path / "ranks"] + argv, gpus, tmp_path)
    assert p.returncode == 0, p.stdout
    assert run_correct(["-o", tmp_path / "one"] + argv, capsys)[0] == 0
    same_outputs(tmp_path / "ranks", tmp_path / "one")
    assert (tmp_path / "one" / "corrected_reads_1.fa").stat().st_size > 1000
    if trim:
        hit = [int(x) for x in TRIMMED.search((tmp_path / "ranks" / "correct_log.txt").read_text()).groups()]
        assert hit[1] > 10 and hit[5] > 5                              # (reads trimmed, pairs dropped)


@pytest.mark.parametrize("gpus,trim", [(3, False), (2, True)])
def test_ranks_ragged_reads(ctx, capsys, tmp_path, gpus, trim):
    path = cc.write_fastq(str(tmp_path / "ragged.fq"), qc.ragged_case(n=500)[0])
    argv = ["--single", path] + (["--trim"] if trim else [])
    p = _ranks(["-o", tmp_path / "ranks"] + argv, gpus, tmp_path)
    assert p.returncode == 0, p.stdout
    assert run_correct(["-o", tmp_path / "one"] + argv, capsys)[0] == 0
    same_outputs(tmp_path / "ranks", tmp_path / "one")


def test_ranks_more_ranks_than_reads_and_mates_that_differ(ctx, planted, capsys, tmp_path):
    """2 reads on 3 ranks: one rank holds none.  Mate files of different read counts: all ranks end with 2, one message."""
    reads = qc.scenario("mid")["files"][0][:2]
    path = cc.write_fastq(str(tmp_path / "two.fq"), reads)
    argv = ["--single", path, "--anchor", "1", "--trim", "--min_len", "30"]      # (A = 1: a read's own windows anchor it)
    p = _ranks(["-o", tmp_path / "ranks"] + argv, 3, tmp_path)
    assert p.returncode == 0, p.stdout
    assert run_correct(["-o", tmp_path / "one"] + argv, capsys)[0] == 0
    same_outputs(tmp_path / "ranks", tmp_path / "one")
    assert (tmp_path / "one" / "corrected_reads.fa").read_text().count(">") == 2
    lanes = planted["lanes"]
    p = _ranks(["-o", tmp_path / "bad", "--left", lanes[0][0] + "," + lanes[0][1], "--right", lanes[1][0] + "," + lanes[1][2]], 2, tmp_path)
    assert p.returncode != 0 and p.stdout.count("lane 2: ") == 1 and "not mates of each other" in p.stdout
    assert not (tmp_path / "bad").exists()


# ---------------------------------------------------------------------------------------------------------------- 8. downstream
def test_downstream_assembly(ctx, planted, capsys, tmp_path, monkeypatch):
    """shannon.py on the command's FASTA files writes the shannon.fasta of `shannon.py --quorum` on the FASTQ files; on the --trim
    output (ragged mates) it runs to the end"""
    import shannon
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")
    for tag, extra in (("u", []), ("t", ["--trim"])):
        whole = planted["noisy_whole"] if extra else planted["whole"]
        out = tmp_path / ("c" + tag)
        assert run_correct(["-o", out, "--left", whole[0], "--right", whole[1]] + extra, capsys)[0] == 0
        asm = tmp_path / ("asm" + tag)
        assert shannon.main(["shannon.py", "-o", str(asm), "--left", str(out / "corrected_reads_1.fa"), "--right", str(out / "corrected_reads_2.fa")]) == 0
        final = (asm / "shannon.fasta").read_bytes()
        assert final.count(b">") >= 1
        if not extra:
            assert final == (planted["runs"]["paired"]["out"] / "shannon.fasta").read_bytes()
        else:
            lens = {len(l) for l in (out / "corrected_reads_1.fa").read_text().splitlines()[1::2]}
            assert len(lens) > 1                                      # (trimmed mates are ragged)
