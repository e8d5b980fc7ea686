"""GPU: the --inDisk formatters (csrc/reads_text.hip) -- shn_reads_fasta, shn_k1mers_dict_text and their file drivers -- byte
for byte against the text a Python join gives over the strings of kmers_for_component.ReadStore.mate1 / mate2 (the reads) and over
the windows of the contigs (the dictionary).  Every comparison is byte equality."""
import ctypes as C
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100]
DOUBLED, SS = 0, 1


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def _strings(rng, lengths):
    return ["".join("ACGT"[c] for c in rng.integers(0, 4, size=int(L))) for L in lengths]


def _fixed(ctx, strs):
    from shannon_amd import device
    code = np.full(256, 4, np.uint8)
    for j, c in enumerate(b"ACGT"):
        code[c] = j
    return device.Reads.from_codes(ctx, np.stack([code[np.frombuffer(s.encode(), np.uint8)] for s in strs]))


def _ragged(ctx, strs):
    from shannon_amd import device
    return device.Reads.from_strings(ctx, strs)


def _routes(ctx, idx, reads):
    from shannon_amd import kmers_for_component as kfc
    return kfc.Routes.from_arrays(ctx, np.zeros(len(idx), np.uint32), np.asarray(idx, np.uint32), reads=reads)


def _expect(store, idx, mode, mate, e0=0):
    """the text of the reference's writer: '>e' + suffix, then the read ReadStore gives for the index"""
    n = store.n
    out = []
    for i, d in enumerate(idx):
        d = int(d)
        if mode == DOUBLED:
            s = store.mate2(d) if mate == 2 else store.mate1(d)
        else:                                   # -s: a[d] / RC(b[d]) = mate1 of the strand-doubled numbering at d / d + N
            s = store.mate1(d + n) if mate == 2 else store.mate1(d)
        out.append(">%d%s\n%s\n" % (e0 + i, "_%d" % mate if mate else "", s))
    return "".join(out).encode()


def _raw_fasta(ctx, routes, a, b, lo, n, mode, mate, e0, out, cap):
    """shn_reads_fasta itself: (return code, *total_out)"""
    from shannon_amd import _lib
    total = C.c_uint64(12345)
    rc = _lib.lib().shn_reads_fasta(ctx.h, a.h, b.h if b is not None else None, routes.h, lo, n, mode, mate, e0,
                                    out.ctypes.data if out is not None else None, cap, C.byref(total))
    return rc, int(total.value)


@pytest.mark.parametrize("L", LENGTHS)
def test_fixed_length_sets(ctx, L):
    """word edges (32 bases a word) and the 16-byte chunk edge inside header, bases and newline"""
    from shannon_amd import kmers_for_component as kfc
    rng = np.random.default_rng(L)
    n = 37
    s1, s2 = _strings(rng, [L] * n), _strings(rng, [L] * n)
    a, b = _fixed(ctx, s1), _fixed(ctx, s2)
    idx = np.arange(2 * n)                                      # both sides of N
    se, pe = kfc.ReadStore(s1), kfc.ReadStore(s1, s2)
    r_se, r_pe = _routes(ctx, idx, (a, None)), _routes(ctx, idx, (a, b))
    assert r_se.fasta(0, 2 * n, DOUBLED, 0) == _expect(se, idx, DOUBLED, 0)
    for mate in (1, 2):
        assert r_pe.fasta(0, 2 * n, DOUBLED, mate) == _expect(pe, idx, DOUBLED, mate)
    # a slice in the middle, names from 7 on
    assert r_pe.fasta(5, 40, DOUBLED, 2, e0=7) == _expect(pe, idx[5:45], DOUBLED, 2, e0=7)


def test_ragged_set_and_mates_of_different_geometry(ctx):
    from shannon_amd import kmers_for_component as kfc
    rng = np.random.default_rng(5)
    lens = LENGTHS * 3 + [0, 129, 250]
    rng.shuffle(lens)
    s1 = _strings(rng, lens)
    a = _ragged(ctx, s1)
    n = len(s1)
    idx = np.sort(rng.choice(2 * n, size=2 * n - 5, replace=False))
    assert _routes(ctx, idx, (a, None)).fasta(0, len(idx), DOUBLED, 0) == _expect(kfc.ReadStore(s1), idx, DOUBLED, 0)
    # a pair: fixed a (33 bases), ragged b
    f1 = _strings(rng, [33] * n)
    fa = _fixed(ctx, f1)
    pe = kfc.ReadStore(f1, s1)
    r = _routes(ctx, idx, (fa, a))
    for mate in (1, 2):
        assert r.fasta(0, len(idx), DOUBLED, mate) == _expect(pe, idx, DOUBLED, mate)
    half = idx[idx < n]
    r = _routes(ctx, half, (fa, a))
    for mate in (1, 2):
        assert r.fasta(0, len(half), SS, mate) == _expect(pe, half, SS, mate)


@pytest.mark.parametrize("mode,paired,mate", [(DOUBLED, False, 0), (DOUBLED, True, 1), (DOUBLED, True, 2), (SS, False, 0), (SS, True, 1), (SS, True, 2)])
def test_the_six_rows_of_the_table(ctx, mode, paired, mate):
    from shannon_amd import kmers_for_component as kfc
    rng = np.random.default_rng(11)
    n = 24
    s1, s2 = _strings(rng, [48] * n), _strings(rng, [48] * n)
    h = "ACGGTCATTGACCTAGGATCCAAG"
    pal = h + kfc.ReadStore._rc(h)                              # its own reverse complement
    assert kfc.ReadStore._rc(pal) == pal and kfc.ReadStore._rc(s1[1]) != s1[1]
    s1[0], s2[3] = pal, pal
    a, b = _fixed(ctx, s1), (_fixed(ctx, s2) if paired else None)
    store = kfc.ReadStore(s1, s2 if paired else None)
    idx = np.array([0, 1, 3, 5, n - 1] + ([n, n + 1, n + 3, 2 * n - 1] if mode == DOUBLED else []))
    got = _routes(ctx, idx, (a, b)).fasta(0, len(idx), mode, mate)
    assert got == _expect(store, idx, mode, mate)
    # the reverse-complemented rows show in the text: the palindrome's record reads the same on both strands, its neighbour's does not
    recs = got.decode().split("\n")[1::2]
    if mate == 2 and mode == SS:
        assert recs[2] == pal and recs[1] == kfc.ReadStore._rc(s2[1]) != s2[1]
    if mode == DOUBLED and mate == 0:
        assert recs[5] == pal and recs[6] == kfc.ReadStore._rc(s1[1]) != s1[1]


def test_a_masked_base_is_written_as_N(ctx):
    from shannon_amd import kmers_for_component as kfc
    s1 = ["ACGTNACGTTTGACCA" * 5, "N" + "C" * 70, "G" * 64 + "N", "ACGT" * 8]
    a = _ragged(ctx, s1)
    idx = np.arange(8)
    assert _routes(ctx, idx, (a, None)).fasta(0, 8, DOUBLED, 0) == _expect(kfc.ReadStore(s1), idx, DOUBLED, 0)


@pytest.fixture(scope="module")
def partition_1001(ctx):
    """a partition of 1,001 routes over a pair of 100-base sets: (routes, store, idx)"""
    from shannon_amd import kmers_for_component as kfc
    rng = np.random.default_rng(1001)
    n = 600
    s1, s2 = _strings(rng, [100] * n), _strings(rng, [100] * n)
    a, b = _fixed(ctx, s1), _fixed(ctx, s2)
    idx = np.sort(rng.choice(2 * n, size=1001, replace=False))
    return _routes(ctx, idx, (a, b)), kfc.ReadStore(s1, s2), idx


def test_names(ctx, partition_1001):
    routes, store, idx = partition_1001
    want = _expect(store, idx, DOUBLED, 1)
    assert want.count(b">9_1\n") == 1 and want.count(b">10_1\n") == 1 and want.count(b">1000_1\n") == 1      # 1, 2, 3, 4 digits
    assert routes.fasta(0, 1001, DOUBLED, 1) == want
    for e0 in (0, 9, 99, 999999999):                            # the last crosses into 10 digits
        assert routes.fasta(17, 3, DOUBLED, 2, e0=e0) == _expect(store, idx[17:20], DOUBLED, 2, e0=e0)
    assert b">1000000000_2\n" in routes.fasta(17, 3, DOUBLED, 2, e0=999999999)


def test_sizes_sizing_call_and_cap(ctx):
    from shannon_amd import kmers_for_component as kfc
    rng = np.random.default_rng(3)
    # names of four digits from e0 = 1000 on: a record of a 121-base read has 1 + 4 + 1 + 121 + 1 = 128 bytes; 32 of them = 4,096
    s1 = _strings(rng, [121] * 31 + [122])
    a = _ragged(ctx, s1)
    store = kfc.ReadStore(s1)
    routes = _routes(ctx, np.arange(32), (a, None))
    assert routes.fasta(0, 0, DOUBLED, 0) == b"" and routes.fasta(32, 0, DOUBLED, 0) == b""
    assert routes.fasta(4, 1, DOUBLED, 0) == _expect(store, [4], DOUBLED, 0)
    exact = routes.fasta(0, 31, DOUBLED, 0, e0=1000) + routes.fasta(0, 1, DOUBLED, 0, e0=1031)
    assert len(exact) == 4096 and exact == _expect(store, list(range(31)) + [0], DOUBLED, 0, e0=1000)
    # ... and as ONE call of exactly 4,096 bytes (the block edge of 256 threads x 16 bytes), then one byte more
    r2 = _routes(ctx, list(range(31)) + [0], (a, None))
    assert r2.fasta(0, 32, DOUBLED, 0, e0=1000) == exact
    more = routes.fasta(0, 32, DOUBLED, 0, e0=1000)
    assert len(more) == 4097 and more == _expect(store, np.arange(32), DOUBLED, 0, e0=1000)
    # the sizing call sets only the total
    rc, total = _raw_fasta(ctx, routes, a, None, 0, 32, DOUBLED, 0, 1000, None, 0)
    assert (rc, total) == (0, 4097)
    # cap one byte short: SHN_ERR_ARG, the total that is needed, nothing written at or past cap
    buf = np.full(4097 + 64, 0xAB, np.uint8)
    rc, total = _raw_fasta(ctx, routes, a, None, 0, 32, DOUBLED, 0, 1000, buf, 4096)
    assert (rc, total) == (ERR_ARG, 4097)
    assert buf[:4096].tobytes() == more[:4096] and (buf[4096:] == 0xAB).all()


def test_refusals_before_any_launch(ctx, partition_1001):
    from shannon_amd import _lib
    routes, _store, _idx = partition_1001
    a, b = routes.reads
    buf = np.full(256, 0xAB, np.uint8)
    before = ctx.timers().get("reads.fasta", (0, 0))[1]
    for args, word in (((a, b, 1000, 2, DOUBLED, 1), "beyond the routes"), ((a, b, 1002, 0, DOUBLED, 1), "beyond the routes"),
                       ((a, None, 0, 1, DOUBLED, 2), "b is NULL"), ((a, b, 0, 1, 7, 1), "unknown mode"), ((a, b, 0, 1, DOUBLED, 3), "unknown mate")):
        ra, rb, lo, n, mode, mate = args
        rc, _total = _raw_fasta(ctx, routes, ra, rb, lo, n, mode, mate, 0, buf, len(buf))
        assert rc == ERR_ARG and word in _lib.lib().shn_last_error().decode()
    assert (buf == 0xAB).all() and ctx.timers().get("reads.fasta", (0, 0))[1] == before


# ---- shn_k1mers_dict_text

WEIGHTS = [0, 9, 10, 99, 100, 4294967295]


def _dict_case(k1, rng):
    contigs = _strings(rng, [k1 - 1, k1, k1 + 1, 300, k1 - 1, 40])
    text = np.frombuffer("".join(contigs).encode(), np.uint8)
    off = np.zeros(len(contigs) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    n_win = sum(max(len(c) - k1 + 1, 0) for c in contigs)
    w = np.array([WEIGHTS[i % len(WEIGHTS)] for i in range(n_win)], np.uint32)
    rows, p = [], 0
    for c in contigs:
        for i in range(len(c) - k1 + 1):
            rows.append("%s\t%d\n" % (c[i:i + k1], int(w[p])))
            p += 1
    return text, off, w, "".join(rows).encode()


@pytest.mark.parametrize("k1", [21, 26, 32])
def test_k1mers_dict_text(ctx, k1):
    from shannon_amd import kmers_for_component as kfc, _lib
    text, off, w, want = _dict_case(k1, np.random.default_rng(k1))
    assert kfc.k1mers_dict_text(ctx, text, off, k1, w) == want
    # a slice of the contigs whose offsets do not start at 0 (how a partition's contigs lie in the text of all partitions)
    n_first = sum(max(int(off[i + 1] - off[i]) - k1 + 1, 0) for i in range(2))
    sub = kfc.k1mers_dict_text(ctx, text, off[2:], k1, w[n_first:])
    assert want.endswith(sub) and len(sub) == len(want) - sum(k1 + 2 + len(str(int(x))) for x in w[:n_first])
    # no contig, and contigs without a window
    assert kfc.k1mers_dict_text(ctx, np.zeros(1, np.uint8), np.zeros(1, np.uint64), k1, np.zeros(0, np.uint32)) == b""
    assert kfc.k1mers_dict_text(ctx, text, off[:2], k1, np.zeros(0, np.uint32)) == b""
    # sizing call; cap one byte short
    L = _lib.lib()
    total = C.c_uint64(0)
    args = (ctx.h, text.ctypes.data, off.ctypes.data, len(off) - 1, k1, w.ctypes.data)
    assert L.shn_k1mers_dict_text(*args, None, 0, C.byref(total)) == 0 and total.value == len(want)
    buf = np.full(len(want) + 64, 0xAB, np.uint8)
    assert L.shn_k1mers_dict_text(*args, buf.ctypes.data, len(want) - 1, C.byref(total)) == ERR_ARG and total.value == len(want)
    assert buf[:len(want) - 1].tobytes() == want[:-1] and (buf[len(want) - 1:] == 0xAB).all()


# ---- the file drivers

def test_file_drivers_in_many_chunks(ctx, partition_1001, tmp_path, monkeypatch):
    from shannon_amd import kmers_for_component as kfc
    routes, store, idx = partition_1001
    monkeypatch.setenv("SHN_INDISK_STAGE_BYTES", "4096")      # about 40 records a chunk: 27 chunks, each ending on a record boundary
    for mate in (1, 2):
        p = str(tmp_path / ("reads_%d.fasta" % mate))
        one = routes.fasta(0, 1001, DOUBLED, mate, e0=5)
        assert len(one) > 20 * 4096
        assert routes.fasta_file(p, 0, 1001, DOUBLED, mate, e0=5) == len(one)
        assert open(p, "rb").read() == one == _expect(store, idx, DOUBLED, mate, e0=5)
    p = str(tmp_path / "empty.fasta")
    assert routes.fasta_file(p, 3, 0, DOUBLED, 1) == 0 and open(p, "rb").read() == b""
    text, off, w, want = _dict_case(26, np.random.default_rng(26))
    assert len(want) > 2 * 4096
    p = str(tmp_path / "k1mer.dict")
    assert kfc.k1mers_dict_file(ctx, p, text, off, 26, w) == len(want) and open(p, "rb").read() == want


def test_file_driver_reports_the_path_it_could_not_open(ctx, partition_1001, tmp_path):
    from shannon_amd import kmers_for_component as kfc, _lib
    routes, store, idx = partition_1001
    p = str(tmp_path / "no_such_directory" / "reads_1.fasta")
    with pytest.raises(_lib.ShannonError) as ei:
        routes.fasta_file(p, 0, 1001, DOUBLED, 1)
    assert p in str(ei.value) and os.strerror(2) in str(ei.value)
    text, off, w, _want = _dict_case(21, np.random.default_rng(21))
    with pytest.raises(_lib.ShannonError) as ei:
        kfc.k1mers_dict_file(ctx, p, text, off, 21, w)
    assert p in str(ei.value)
    # ... and the device is as it was: the next call gives its text
    assert routes.fasta(0, 3, DOUBLED, 1) == _expect(store, idx[:3], DOUBLED, 1)
