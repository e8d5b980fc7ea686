"""CPU: the pieces of a partition's reads that carry lengths (exchange.RaggedPiece) -- through pack / unpack beside the
fixed-length pieces, whose bytes stay what they were; merged at the owner in the order of the global indices; and the slice of
device.RaggedCodes the N-rank CLI's whole-file fallback takes."""
import numpy as np
import pytest


def _piece(rng, n, paired, lo=0, hi=12):
    from shannon_amd import exchange

    def one():
        lens = rng.integers(lo, hi, n)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        return rng.integers(0, 5, int(off[-1])).astype(np.uint8), off
    c1, o1 = one()
    c2, o2 = one() if paired else (None, None)
    return exchange.RaggedPiece(c1, o1, rng.integers(0, 2, n).astype(np.uint8), c2, o2)


def _same(p, q):
    assert len(p) == len(q) and p.paired == q.paired
    assert np.array_equal(p.codes, q.codes) and np.array_equal(p.off, q.off) and np.array_equal(p.rc, q.rc)
    if p.paired:
        assert np.array_equal(p.codes2, q.codes2) and np.array_equal(p.off2, q.off2)


def _todays_pack(items):
    """exchange.pack_read_pieces as it was before pieces could carry lengths"""
    head = [len(items)]
    body = []
    for p, gidx, (rows, rc1) in items:
        n, L = int(rows.shape[0]), int(rows.shape[1]) if rows.ndim == 2 else 0
        head += [int(p), n, L]
        body += [np.ascontiguousarray(gidx, dtype=np.int64).view(np.uint8).reshape(-1), np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1),
                 np.ascontiguousarray(rc1, dtype=np.uint8).reshape(-1)]
    return np.concatenate([np.asarray(head, dtype=np.int64).view(np.uint8)] + body)


@pytest.mark.parametrize("paired", [False, True])
def test_ragged_pieces_round_trip(paired):
    from shannon_amd import exchange
    rng = np.random.default_rng(3)
    fixed = (rng.integers(0, 4, (6, 9)).astype(np.uint8), rng.integers(0, 2, 6).astype(np.uint8))
    items = [(4, np.arange(7, dtype=np.int64) * 3, _piece(rng, 7, paired)),
             (0, np.zeros(0, np.int64), _piece(rng, 0, paired)),                     # no reads
             (9, np.arange(6, dtype=np.int64) + 100, fixed),                         # a fixed-length piece between them
             (2, np.arange(5, dtype=np.int64), _piece(rng, 5, paired, 0, 1)),        # reads without bases
             (7, np.array([5, 1], np.int64), _piece(rng, 2, paired, 200, 300))]
    buf = exchange.pack_read_pieces(items)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    out = exchange.unpack_read_pieces(buf)
    assert [o[0] for o in out] == [4, 0, 9, 2, 7]
    for (_p, g, d), (_q, g2, d2) in zip(items, out):
        assert np.array_equal(g, g2)
        if isinstance(d, exchange.RaggedPiece):
            assert isinstance(d2, exchange.RaggedPiece)
            _same(d, d2)
        else:
            assert np.array_equal(d[0], d2[0]) and np.array_equal(d[1], d2[1])
    head = buf[8:8 + 24 * 5].view(np.int64).reshape(5, 3)
    assert head[:, 2].tolist() == [-2 if paired else -1] * 2 + [9] + [-2 if paired else -1] * 2


def test_fixed_length_pieces_travel_as_the_bytes_they_always_were():
    from shannon_amd import exchange
    rng = np.random.default_rng(4)
    items = [(i, rng.integers(0, 1 << 40, n).astype(np.int64), (rng.integers(0, 4, (n, L)).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)))
             for i, (n, L) in enumerate(((5, 100), (0, 100), (3, 31), (1, 1)))]
    assert exchange.pack_read_pieces(items).tobytes() == _todays_pack(items).tobytes()
    assert exchange.pack_read_pieces([]).tobytes() == _todays_pack([]).tobytes()


@pytest.mark.parametrize("paired", [False, True])
def test_merge_orders_the_reads_by_their_global_indices(paired):
    from shannon_amd import exchange
    from shannon_amd.distributed import GpuOps
    rng = np.random.default_rng(5)
    gidx = rng.permutation(40).astype(np.int64)
    parts = [np.sort(gidx[:13]), np.sort(gidx[13:14]), np.sort(gidx[14:])]           # interleaved among the three source ranks
    pieces = [(g, _piece(rng, len(g), paired)) for g in parts] + [(np.zeros(0, np.int64), _piece(rng, 0, paired))]
    m = GpuOps._merge_pieces(pieces)
    assert isinstance(m, exchange.RaggedPiece) and m.paired == paired
    rows = sorted(((int(g), r.tolist(), int(c), (r2.tolist() if paired else None)) for gs, p in pieces
                   for g, r, c, r2 in zip(gs, p.reads(), p.rc, p.reads(True) if paired else [None] * len(p))), key=lambda t: t[0])
    assert [r.tolist() for r in m.reads()] == [t[1] for t in rows]
    assert m.rc.tolist() == [t[2] for t in rows]
    if paired:
        assert [r.tolist() for r in m.reads(True)] == [t[3] for t in rows]
    # one source rank, already in order: the piece itself
    alone = GpuOps._merge_pieces(pieces[:1])
    _same(alone, pieces[0][1])


def test_a_fixed_length_piece_merges_with_ragged_ones():
    from shannon_amd.distributed import GpuOps
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 4, (3, 8)).astype(np.uint8)
    rag = _piece(rng, 2, False)
    m = GpuOps._merge_pieces([(np.array([1, 3, 5]), (rows, np.array([0, 1, 0], np.uint8))), (np.array([0, 4]), rag)])
    assert [r.tolist() for r in m.reads()] == [rag.reads()[0].tolist(), rows[0].tolist(), rows[1].tolist(), rag.reads()[1].tolist(), rows[2].tolist()]
    # the two mates of a -s pair side by side in the rows
    both = GpuOps._as_ragged((np.concatenate([rows, rows[::-1]], axis=1), np.zeros(3, np.uint8)), halves=True)
    assert [r.tolist() for r in both.reads()] == rows.tolist() and [r.tolist() for r in both.reads(True)] == rows[::-1].tolist()


def test_ragged_codes_slice():
    from shannon_amd import device
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 20, 50)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    R = device.RaggedCodes(rng.integers(0, 5, int(off[-1])).astype(np.uint8), off)
    for lo, hi in ((0, 50), (7, 31), (49, 50), (12, 12), (50, 50), (0, 0)):
        S = R[lo:hi]
        assert isinstance(S, device.RaggedCodes) and len(S) == hi - lo and int(S.off[0]) == 0 and S.off.dtype == np.uint64
        assert S.total_bases == int(off[hi] - off[lo])
        assert all(np.array_equal(S[i], R[lo + i]) for i in range(hi - lo))
        if hi > lo:
            assert np.shares_memory(S.codes, R.codes) or S.total_bases == 0
            c, o = S.take(np.arange(hi - lo)[::-1])
            assert np.array_equal(c[:int(o[-1])], np.concatenate([R[i] for i in range(hi - 1, lo - 1, -1)]))
    assert np.array_equal(R[3], R.codes[int(off[3]):int(off[4])])                     # (an index is still one read)
    M = device.RaggedCodes.from_matrix(np.arange(12, dtype=np.uint8).reshape(3, 4) % 4)
    assert len(M) == 3 and M.off.tolist() == [0, 4, 8, 12] and M[1].tolist() == [0, 1, 2, 3]
