"""GPU: the merge of class sets.  shn_abundance_merge (csrc/abundance.hip) through the C ABI against the brute force of
tests/merge_cases.py; abundance.merge_classes of the classes of parts of the reads against abundance.classes / classes_single of all the
reads; `python -m shannon_amd.quant` on lane files and on N ranks against the one-process run on the concatenated files.  Everything is
integers or bytes and compared exactly."""
import ctypes as C
import os, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT
import abundance_cases as ac
import filter_fp_cases as fc
import merge_cases as mc
from test_abundance_gpu import upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def merge_abi(ctx, lists, weights, m, hash_bits=63):
    """shn_abundance_merge on lists and weights -> (sizes[6], class_off, members, n_c)"""
    from shannon_amd import _lib
    L = _lib.lib()
    off, mem = mc.csr(lists)
    w = np.array([int(x) for x in weights], dtype=np.uint64)
    h = C.c_void_p()
    _lib.check(L.shn_abundance_merge(ctx.h, off.ctypes.data, mem.ctypes.data if len(mem) else None, w.ctypes.data if len(w) else None, len(lists), m, hash_bits,
                                     C.byref(h)))
    try:
        sizes = np.zeros(6, dtype=np.uint64)
        _lib.check(L.shn_abundance_sizes(h, sizes.ctypes.data))
        n_classes, n_entries = int(sizes[3]), int(sizes[4])
        class_off, members, n_c = np.zeros(n_classes + 1, np.uint64), np.zeros(max(n_entries, 1), np.uint32), np.zeros(max(n_classes, 1), np.uint64)
        _lib.check(L.shn_abundance_export(h, class_off.ctypes.data, members.ctypes.data, n_c.ctypes.data, None))
    finally:
        L.shn_abundance_destroy(h)
    return [int(x) for x in sizes], class_off, members[:n_entries], n_c[:n_classes]


def check_against_brute(ctx, lists, weights, m):
    sizes, off, mem, n_c = merge_abi(ctx, lists, weights, m)
    w_off, w_mem, w_nc = mc.brute_arrays(lists, weights)
    assert off.tolist() == w_off.tolist() and mem.tolist() == w_mem.tolist() and n_c.tolist() == w_nc.tolist()
    total = sum(int(x) for x in weights)
    assert sizes == [m, total, total, len(w_nc), len(w_mem), 0]
    return off, mem, n_c


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_no_lists_one_list_and_one_list_twice(ctx):
    sizes, off, mem, n_c = merge_abi(ctx, [], [], 5)
    assert sizes == [5, 0, 0, 0, 0, 0] and off.tolist() == [0] and len(mem) == 0 and len(n_c) == 0
    off, mem, n_c = check_against_brute(ctx, [[2, 4]], [7], 5)
    assert off.tolist() == [0, 2] and mem.tolist() == [2, 4] and n_c.tolist() == [7]
    off, mem, n_c = check_against_brute(ctx, [[2, 4], [2, 4]], [3000000000, 3000000000], 5)
    assert off.tolist() == [0, 2] and mem.tolist() == [2, 4] and n_c.tolist() == [6000000000]        # exact beyond 2^32
    off, mem, n_c = check_against_brute(ctx, [[1], [1], [3]], [0, 0, 0], 5)                          # weights of 0 are kept
    assert sorted(n_c.tolist()) == [0, 0] and len(off) == 3


@pytest.mark.parametrize("n", [1, 2, 32, 33, 64, 65, 1001])
def test_list_lengths_last_members_and_prefixes(ctx, n):
    """lists of n members: the same list in three parts; a list that differs from it in the last member only; its proper prefix (n > 1)
    and the list it is a proper prefix of"""
    m = 1100
    A = list(range(3, 3 + n))
    B = A[:-1] + [A[-1] + 1]
    longer = A + [A[-1] + 2]
    lists, weights = [A, B, A, longer, B, A], [5, 7, 11, 13, 17, 19]
    if n > 1:
        lists, weights = lists + [A[:-1], A[:-1]], weights + [23, 29]
    off, mem, n_c = check_against_brute(ctx, lists, weights, m)
    got = dict(mc.lists_of({"class_off": off, "members": mem, "n_c": n_c}))
    assert got[tuple(A)] == 35 and got[tuple(B)] == 24 and got[tuple(longer)] == 13 and len(got) == (4 if n > 1 else 3)
    if n > 1:
        assert got[tuple(A[:-1])] == 52


def test_a_class_of_many_lists(ctx):
    """one list 300 times among 299 others, each twice: a class's weights are summed over any number of lists (the wave's strided loop
    runs five times), the others over two"""
    lists, weights = [], []
    for k in range(300):
        lists += [[0, 9], [k + 10], [k + 10]] if k < 299 else [[0, 9]]
        weights += [k + 1, 2 * k, 1] if k < 299 else [k + 1]
    off, mem, n_c = check_against_brute(ctx, lists, weights, 400)
    got = dict(mc.lists_of({"class_off": off, "members": mem, "n_c": n_c}))
    assert got[(0, 9)] == 300 * 301 // 2 and len(got) == 300


@pytest.mark.parametrize("hash_bits", [1, 2])
def test_lists_that_share_a_key_are_told_apart_by_their_members(ctx, hash_bits):
    """three distinct lists arriving as A, B, A, B, C under keys of 1 or 2 bits: some share a key, so the heads are found by comparing the
    lists; a list's class may be split in two (DESIGN.md 3.10 rule 3), never mixed with another list's"""
    from shannon_amd import abundance
    A, B, Cl = [1, 2, 3], [1, 2, 4], [1, 2]
    lists, weights = [A, B, A, B, Cl], [3, 5, 7, 11, 13]
    mask = (1 << hash_bits) - 1
    keys = [abundance.list_key(M) & mask for M in (A, B, Cl)]
    if hash_bits == 1:
        assert len(set(keys)) < 3                                                     # at least two of the three share a key
    sizes, off, mem, n_c = merge_abi(ctx, lists, weights, 6, hash_bits)
    got = mc.lists_of({"class_off": off, "members": mem, "n_c": n_c})
    assert all(list(M) in (A, B, Cl) for M, _n in got)
    per_list = {}
    for M, n in got:
        per_list[M] = per_list.get(M, 0) + n
    assert per_list == dict(mc.brute_merge(lists, weights)) == {(1, 2, 3): 10, (1, 2, 4): 16, (1, 2): 13}
    assert 3 <= len(got) <= 5 and sizes[1] == sizes[2] == 39
    # the masked keys ascend along the output
    out_keys = [abundance.list_key(M) & mask for M, _n in got]
    assert out_keys == sorted(out_keys)
    # ... and with all 63 bits the arrays are the brute force's
    check_against_brute(ctx, lists, weights, 6)


def test_refusals_before_any_launch(ctx):
    from shannon_amd import _lib
    L = _lib.lib()
    u64, u32 = (lambda x: np.array(x, dtype=np.uint64)), (lambda x: np.array(x, dtype=np.uint32))
    good_off, good_mem, good_w = u64([0, 2, 3]), u32([1, 4, 2]), u64([5, 6])
    h = C.c_void_p()

    def call(off=good_off, mem=good_mem, w=good_w, n=2, m=5, bits=63, out=True):
        return L.shn_abundance_merge(ctx.h, off.ctypes.data if off is not None else None, mem.ctypes.data if mem is not None else None,
                                     w.ctypes.data if w is not None else None, n, m, bits, C.byref(h) if out else None)
    ARG, OVERFLOW = -1, -4                                                           # SHN_ERR_ARG, SHN_ERR_OVERFLOW of include/shannon_hip.h
    cases = [(dict(m=0), "no transcripts", ARG),
             (dict(bits=0), "hash_bits 0 outside 1 .. 63", ARG),
             (dict(bits=64), "hash_bits 64 outside 1 .. 63", ARG),
             (dict(off=u64([1, 2, 3])), r"class_off\[0\] is not 0", ARG),
             (dict(off=u64([0, 3, 2])), "class_off not monotone", ARG),
             (dict(off=u64([0, 2, 2])), "list 1 is empty", ARG),
             (dict(mem=u32([1, 5, 2])), "a list names transcript 5 of 5", ARG),
             (dict(mem=u32([4, 1, 2])), "list 0 is not strictly ascending", ARG),
             (dict(mem=u32([1, 1, 2])), "list 0 is not strictly ascending", ARG),
             (dict(n=1 << 32), "2\\^32 or more lists", OVERFLOW),
             (dict(w=u64([1 << 63, 1 << 63])), "the weights' sum does not fit in 64 bits", OVERFLOW),
             (dict(off=None), "NULL argument", ARG),
             (dict(w=None), "NULL argument", ARG),
             (dict(out=False), "NULL argument", ARG)]
    for kw, msg, code in cases:
        ctx.timer_reset()
        with pytest.raises(_lib.ShannonError, match="shn_abundance_merge: " + msg) as ei:
            _lib.check(call(**kw))
        assert "(code %d)" % code in str(ei.value)
        assert not any(k.startswith("abundance.") for k in ctx.timers()), "nothing launched"
        assert not h.value
    # the largest sum that fits is taken
    sizes, off, mem, n_c = merge_abi(ctx, [[1], [1]], [(1 << 63), (1 << 63) - 1], 3)
    assert n_c.tolist() == [(1 << 64) - 1] and sizes[1] == (1 << 64) - 1
    ctx.timer_reset()
    merge_abi(ctx, [[1], [2]], [1, 1], 3)
    assert [k for k in ctx.timers() if k.startswith("abundance.")] == ["abundance.merge"] and ctx.timer_bytes()["abundance.merge"] > 0


# ---------------------------------------------------------------------------------------------------------------- parts of reads
def _cut(reads, cuts):
    return [reads[a:b] for a, b in zip(cuts, cuts[1:])]


def _same(got, want):
    for k in ("class_off", "members", "n_c", "hist"):
        assert got[k].dtype == want[k].dtype and got[k].tolist() == want[k].tolist(), k
    assert got["mapped"] == want["mapped"] and got["fragments"] == want["fragments"]


@pytest.fixture(scope="module")
def read_cases():
    """(transcripts, r1, r2, the cuts of the reads into parts) -- shared_exon_case's last pair matches nothing: a part of its own, all
    unmapped; a part without reads in both"""
    T, r1, r2, _want = ac.shared_exon_case()
    assert len(r1) == 19
    T2, s1, s2 = ac.interleaved_case(33)
    return {"shared exon": (T, r1, r2, [[0, 19], [0, 0, 5, 12, 18, 19], [0, 1, 2, 3, 18, 18, 19], [0, 10, 19]]),
            "interleaved 33": (T2, s1, s2, [[0, 3], [0, 1, 1, 3], [0, 2, 3], [0, 0, 3, 3]])}


@pytest.mark.parametrize("name", ["shared exon", "interleaved 33"])
@pytest.mark.parametrize("ss", [True, False])
def test_merged_classes_of_the_parts_are_the_classes_of_all_reads(ctx, read_cases, name, ss):
    from shannon_amd import abundance
    T, r1, r2, all_cuts = read_cases[name]

    def paired(a, b):
        d1, d2 = upload(ctx, a), upload(ctx, b)
        try:
            return abundance.classes(ctx, T, d1, d2, ss)
        finally:
            d1.close()
            d2.close()

    def single(a):
        d = upload(ctx, a)
        try:
            return abundance.classes_single(ctx, T, d, ss)
        finally:
            d.close()
    whole, whole_single = paired(r1, r2), single(r1)
    assert len(whole["n_c"]) >= 1 and len(whole["hist"]) == abundance.MAX_SPAN + 1 and len(whole_single["hist"]) == 0
    # (no two of these lists share a 63-bit key: the classes arrive one per distinct list in ascending key order)
    keys = [abundance.list_key(M) for M, _n in mc.lists_of(whole)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for cuts in all_cuts:
        parts = [paired(a, b) for a, b in zip(_cut(r1, cuts), _cut(r2, cuts))]
        assert [p["fragments"] for p in parts] == [b - a for a, b in zip(cuts, cuts[1:])]
        _same(abundance.merge_classes(ctx, parts, len(T)), whole)
        _same(abundance.merge_classes(ctx, [single(a) for a in _cut(r1, cuts)], len(T)), whole_single)
        if cuts == [0, 0, 5, 12, 18, 19]:                     # a part without reads; a part whose only pair maps nowhere
            assert (parts[0]["fragments"], parts[0]["mapped"]) == (0, 0) and (parts[-1]["fragments"], parts[-1]["mapped"]) == (1, 0)
            assert len(parts[0]["n_c"]) == 0 and len(parts[-1]["n_c"]) == 0 and all(len(p["n_c"]) for p in parts[1:-1])
    _same(abundance.merge_classes(ctx, [whole], len(T)), whole)                       # merging one part is the identity
    with pytest.raises(ValueError, match="histograms"):
        abundance.merge_classes(ctx, [whole, whole_single], len(T))


# ---------------------------------------------------------------------------------------------------------------- the command
def _fastq(path, reads):
    path.write_text("".join("@%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    return str(path)


def _main(argv, capsys, want_rc=0):
    from shannon_amd import quant
    capsys.readouterr()
    rc = quant.main(["quant"] + argv)
    out = capsys.readouterr()
    assert rc == want_rc, out.err
    return out


def _files_of(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(str(d))) if n != "quant_log.txt"}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """planted_case's transcripts and 300 pairs, the second mates of the last 100 pairs cut to 60 bases (mates of two lengths, so L is
    no whole number), as files: all reads, and three lanes of 120 / 0 / 180 pairs"""
    T, names, r1, r2 = fc.planted_case(n_pairs=300)
    r2 = r2[:200] + [r[:60] for r in r2[200:]]
    d = tmp_path_factory.mktemp("planted")
    fa = d / "t.fasta"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in zip(names, T)))
    f = {"fa": str(fa), "r1": _fastq(d / "r1.fq", r1), "r2": _fastq(d / "r2.fq", r2), "dir": d}
    for k, (a, b) in enumerate(((0, 120), (120, 120), (120, 300))):
        f["l1_%d" % k], f["l2_%d" % k] = _fastq(d / ("a%d.fq" % k), r1[a:b]), _fastq(d / ("b%d.fq" % k), r2[a:b])
    f["bases"], f["pairs"] = sum(len(r) for r in r1) + sum(len(r) for r in r2), len(r1)
    return f


def test_command_on_lane_files_paired(planted, tmp_path, capsys):
    f = planted
    extra = ["--cutoff", "2", "-b", "3", "--seed", "7"]
    _main([f["fa"], "-o", str(tmp_path / "one"), "--left", f["r1"], "--right", f["r2"]] + extra, capsys)
    _main([f["fa"], "-o", str(tmp_path / "lanes"), "--left", ",".join(f["l1_%d" % k] for k in range(3)), "--right", ",".join(f["l2_%d" % k] for k in range(3))]
          + extra, capsys)
    one, lanes = _files_of(tmp_path / "one"), _files_of(tmp_path / "lanes")
    assert sorted(one) == ["abundance.tsv", "bootstrap_summary.tsv", "bs_abundance_0.tsv", "bs_abundance_1.tsv", "bs_abundance_2.tsv", "filtered.fasta"]
    assert lanes == one
    assert 0 < one["filtered.fasta"].count(b">") < one["abundance.tsv"].count(b"\n") - 1          # the cutoff dropped some, kept some
    log1, log = (tmp_path / "one" / "quant_log.txt").read_text(), (tmp_path / "lanes" / "quant_log.txt").read_text()
    assert "merge" not in log1                                                                   # one pair of files: the run it always was
    assert log.splitlines()[0] == log1.splitlines()[0]                                           # pairs, mapped, classes, rounds, L as repr
    want_L = f["bases"] / f["pairs"]
    assert want_L != int(want_L) and ("L %r" % want_L) in log.splitlines()[0]
    line = [l for l in log.splitlines() if l.startswith("merge: ")]
    assert len(line) == 1 and line[0].startswith("merge: 3 parts, ") and "classes out; abundance.merge {" in line[0] and '"bytes"' in line[0]
    # a lane whose mates differ in count is refused by name
    err = _main([f["fa"], "-o", str(tmp_path / "bad"), "--left", f["l1_0"] + "," + f["l1_2"], "--right", f["l2_0"] + "," + f["l2_0"]], capsys, want_rc=2).err
    assert "lane 2" in err and "not mates" in err


def test_command_on_lane_files_single_end(planted, tmp_path, capsys):
    f = planted
    extra = ["--cutoff", "2", "-b", "3", "--seed", "7", "-s"]
    _main([f["fa"], "-o", str(tmp_path / "one"), "--single", f["r2"]] + extra, capsys)
    _main([f["fa"], "-o", str(tmp_path / "lanes"), "--single", ",".join(f["l2_%d" % k] for k in range(3))] + extra, capsys)
    assert _files_of(tmp_path / "lanes") == _files_of(tmp_path / "one") and len(_files_of(tmp_path / "one")) == 6
    first = lambda d: (tmp_path / d / "quant_log.txt").read_text().splitlines()[0]
    assert first("lanes") == first("one") and "merge: 3 parts" in (tmp_path / "lanes" / "quant_log.txt").read_text()


# ---------------------------------------------------------------------------------------------------------------- N ranks
def _ranks(argv, gpus, tmp_path):
    """the command with --gpus N as a fresh process: N ranks on GPU 0, collectives through host memory"""
    env = dict(os.environ, SHN_CLI_BACKEND="gloo", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SHN_CLI_LAUNCH_PROBE", None)
    return subprocess.run([sys.executable, "-m", "shannon_amd.quant"] + argv + ["--gpus", str(gpus)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, env=env, cwd=str(tmp_path), timeout=300)


@pytest.fixture(scope="module")
def two_pairs(planted, tmp_path_factory):
    """two read pairs in one lane -- on 3 ranks one rank holds none -- and the one-process run on them"""
    from shannon_amd import quant
    T, names, r1, r2 = fc.planted_case(n_pairs=300)
    d = tmp_path_factory.mktemp("two")
    f = {"fa": planted["fa"], "r1": _fastq(d / "r1.fq", r1[:2]), "r2": _fastq(d / "r2.fq", r2[:2]), "r2_short": _fastq(d / "r2s.fq", r2[:1]), "dir": d}
    f["extra"] = ["--cutoff", "0.001", "-b", "3", "--seed", "7"]
    assert quant.main(["quant", f["fa"], "-o", str(d / "one"), "--left", f["r1"], "--right", f["r2"]] + f["extra"]) == 0
    f["one"] = _files_of(d / "one")
    return f


@pytest.mark.parametrize("gpus", [2, 3])
def test_ranks_write_the_files_of_one_process(two_pairs, tmp_path, gpus):
    f = two_pairs
    p = _ranks([f["fa"], "-o", str(tmp_path / "out"), "--left", f["r1"], "--right", f["r2"]] + f["extra"], gpus, tmp_path)
    assert p.returncode == 0, p.stdout[-3000:]
    assert _files_of(tmp_path / "out") == f["one"] and len(f["one"]) == 6
    log = (tmp_path / "out" / "quant_log.txt").read_text()
    assert log.splitlines()[0] == (f["dir"] / "one" / "quant_log.txt").read_text().splitlines()[0]
    assert "merge: %d parts (%d ranks), " % (gpus, gpus) in log


def test_ranks_on_lane_files(planted, tmp_path):
    f = planted
    argv = [f["fa"], "-o", str(tmp_path / "out"), "--left", ",".join(f["l1_%d" % k] for k in (0, 2)), "--right", ",".join(f["l2_%d" % k] for k in (0, 2))]
    p = _ranks(argv, 2, tmp_path)
    assert p.returncode == 0, p.stdout[-3000:]
    from shannon_amd import quant
    assert quant.main(["quant", f["fa"], "-o", str(tmp_path / "one"), "--left", f["r1"], "--right", f["r2"]]) == 0
    assert _files_of(tmp_path / "out") == _files_of(tmp_path / "one")
    assert "merge: 4 parts (2 ranks), " in (tmp_path / "out" / "quant_log.txt").read_text()


def test_ranks_slice_whole_files_the_byte_shares_decline(planted, tmp_path):
    """single-end reads as a multi-line FASTA and as a .gz: no rank can take a share of the bytes, so every rank reads the whole file
    and takes its records by index"""
    import gzip
    from shannon_amd import quant
    reads = [l for l in open(planted["r1"]).read().splitlines()[1::4]][:41]
    wrapped = tmp_path / "wrapped.fa"
    wrapped.write_text("".join(">%d\n%s\n%s\n" % (i, s[:40], s[40:]) for i, s in enumerate(reads[:20])))
    gz = tmp_path / "rest.fq.gz"
    with gzip.open(str(gz), "wt") as f:
        f.write("".join("@%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads[20:])))
    p = _ranks([planted["fa"], "-o", str(tmp_path / "out"), "--single", "%s,%s" % (wrapped, gz)], 2, tmp_path)
    assert p.returncode == 0, p.stdout[-3000:]
    assert quant.main(["quant", planted["fa"], "-o", str(tmp_path / "one"), "--single", _fastq(tmp_path / "all.fq", reads)]) == 0
    assert _files_of(tmp_path / "out") == _files_of(tmp_path / "one")
    assert "reads: " in (tmp_path / "out" / "quant_log.txt").read_text() and "merge: 4 parts (2 ranks), " in (tmp_path / "out" / "quant_log.txt").read_text()


def test_a_refused_lane_ends_every_rank(two_pairs, tmp_path):
    """mates that differ in count: every rank ends with a message and a non-zero code inside the time limit -- nobody waits in a
    collective"""
    f = two_pairs
    p = _ranks([f["fa"], "-o", str(tmp_path / "out"), "--left", f["r1"], "--right", f["r2_short"]], 3, tmp_path)
    assert p.returncode != 0 and "lane 1" in p.stdout and "not mates" in p.stdout, p.stdout[-3000:]
    assert not (tmp_path / "out" / "abundance.tsv").exists()
