"""GPU: the two halves of shn_filter_fp_hits -- shn_filter_fp_cover on a share of the routes (filter_fp.coverage_bitmap) and
shn_filter_fp_count over the bitmaps of all shares (filter_fp.hits_from_bitmaps, kernel ffp_merge_count_kernel) -- against the brute
force of tests/filter_fp_cases.py, against the one call, and against the numpy mirror.  Hits are integers: every comparison is
exact.  One process; the shares model the ranks of an N-rank run (routes of a rank = routes of ITS reads, read sets = its slice)."""
import functools
import numpy as np
import pytest
import filter_fp_cases as fc
from test_filter_fp_gpu import upload

pytestmark = pytest.mark.gpu

RAGGED = [14, 15, 29, 30, 59, 60, 64, 100, 150, 250]
CASES = {"synth_ss": lambda: fc.synth_case(True), "synth_ds": lambda: fc.synth_case(False), "partition": fc.partition_case,
         "isoform": fc.isoform_case, "isoform_ds": lambda: fc.isoform_case(ss=False), "edge": fc.edge_case,
         "ragged": lambda: fc.length_case(RAGGED, RAGGED, n_pairs=120, seed=8)}


@functools.lru_cache(maxsize=None)
def case_and_hits(name):
    """(case, brute-force hits): computed once, shared by every test, never changed"""
    case = CASES[name]()
    return case, tuple(fc.brute_hits(case))


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def bitmap(ctx, case, d1, d2, routes, stats=None):
    from shannon_amd import filter_fp
    return filter_fp.coverage_bitmap(ctx, case["transcripts"], case["part_of"], case["n_parts"], d1, d2, routes, case["ss"], stats=stats)


def both_counts(ctx, covers, t_off, word0=0):
    """the kernel's hits, after holding them against the numpy mirror"""
    from shannon_amd import filter_fp
    dev = filter_fp.hits_from_bitmaps(ctx, covers, t_off, word0).tolist()
    assert dev == filter_fp.hits_from_bitmaps(None, covers, t_off, word0).tolist()
    return dev


@pytest.mark.parametrize("name", sorted(CASES))
def test_sharded_routes(ctx, name):
    """route i to shard i % W for W = 1, 2, 3, 5, and for W = 3 once more with a shard that gets no route at all: the count over the
    shards' bitmaps is the brute force's and the one call's"""
    from shannon_amd import filter_fp
    case, want = case_and_hits(name)
    pid, idx = case["routes"]
    n = len(pid)
    t_off = filter_fp.text_offsets(case["transcripts"])
    d1, d2 = upload(ctx, case["r1"]), upload(ctx, case["r2"])
    try:
        whole_stats = {}
        whole = filter_fp.coverage_hits(ctx, case["transcripts"], case["part_of"], case["n_parts"], d1, d2, case["routes"], case["ss"],
                                        stats=whole_stats).tolist()
        assert whole == list(want)
        for W, mod in ((1, 1), (2, 2), (3, 3), (5, 5), (3, 2)):
            shard_of = np.arange(n) % mod
            if name == "partition":                             # the fragment routed twice to partition 0: its two routes in different shards
                twice = [i for i in range(n) if pid[i] == 0 and idx[i] == 12]
                assert len(twice) == 2 and (W == 1 or shard_of[twice[0]] != shard_of[twice[1]])
            covers, stats = [], {}
            for s in range(W):
                sel = shard_of == s
                assert sel.any() or (W, mod, s) == (3, 2, 2)
                covers.append(bitmap(ctx, case, d1, d2, (pid[sel], idx[sel]), stats))
            covers = np.stack(covers)
            assert covers.shape == (W, (int(t_off[-1]) + 63) // 64)
            got = both_counts(ctx, covers, t_off)
            print("W = %d (mod %d): brute force %s\n                 merged      %s" % (W, mod, list(want), got))
            assert got == list(want)
            assert stats["routes"] == n == whole_stats["routes"]
            if name != "partition":                             # (a fragment routed twice is placed once per route)
                assert stats["placed"] == whole_stats["placed"]
            if W > 1 and sum(want):
                assert not all(np.array_equal(c, covers[0]) for c in covers[1:])
    finally:
        d1.close()
        d2.close()


@pytest.mark.parametrize("name", ["synth_ss", "synth_ds", "isoform_ds", "edge", "ragged"])
@pytest.mark.parametrize("W", [2, 3])
def test_sliced_read_sets(ctx, name, W):
    """the read sets cut into W contiguous slices, each uploaded on its own, every route re-based into its slice's numbering and
    mapped with that slice's sets -- what a rank of an N-rank run holds"""
    from shannon_amd import filter_fp
    case, want = case_and_hits(name)
    pid, idx = np.asarray(case["routes"][0]), np.asarray(case["routes"][1]).astype(np.int64)
    N = len(case["r1"])
    frag = idx if case["ss"] else idx % N
    covers, n_routes = [], 0
    for s in range(W):
        lo, hi = s * N // W, (s + 1) * N // W
        n_local = hi - lo
        assert n_local > 0
        sel = (frag >= lo) & (frag < hi)
        local = np.where(idx[sel] < N, idx[sel] - lo, (idx[sel] - N - lo) + n_local) if not case["ss"] else idx[sel] - lo
        assert case["ss"] or ((local >= n_local).any() or not (idx[sel] >= N).any())
        n_routes += int(sel.sum())
        d1, d2 = upload(ctx, case["r1"][lo:hi]), upload(ctx, case["r2"][lo:hi])
        try:
            covers.append(bitmap(ctx, case, d1, d2, (pid[sel], local.astype(np.uint32))))
        finally:
            d1.close()
            d2.close()
    assert n_routes == len(pid)
    assert both_counts(ctx, np.stack(covers), filter_fp.text_offsets(case["transcripts"])) == list(want)


def test_windows_of_the_text(ctx):
    """every contiguous run of transcripts counted from its own word window (word0 > 0, boundary words that carry neighbours' bits):
    the matching slice of the whole text's hits"""
    from shannon_amd import filter_fp
    case, want = case_and_hits("edge")
    assert list(want) == [400, 0, 500, 60, 0, 200]
    t_off = filter_fp.text_offsets(case["transcripts"])
    n = len(want)
    pid, idx = case["routes"]
    d1, d2 = upload(ctx, case["r1"]), upload(ctx, case["r2"])
    try:
        covers = np.stack([bitmap(ctx, case, d1, d2, (pid[s::2], idx[s::2])) for s in range(2)])
    finally:
        d1.close()
        d2.close()
    bits = np.unpackbits(np.bitwise_or.reduce(covers, axis=0).view(np.uint8), bitorder="little")
    inner = [int(b) for b in t_off[1:-1] if int(b) % 64 and bits[int(b) - 1] and bits[int(b)]]
    assert inner, "no transcript boundary inside a word with covered bases on both sides"
    assert both_counts(ctx, covers, t_off) == list(want)
    shifted = 0
    for a in range(n):
        for b in range(a + 1, n + 1):
            w0, w1 = int(t_off[a]) >> 6, (int(t_off[b]) + 63) // 64
            shifted += w0 > 0
            assert both_counts(ctx, covers[:, w0:w1], t_off[a:b + 1], w0) == list(want[a:b]), (a, b)
    assert shifted >= n


def test_refusals_launch_nothing(ctx):
    from shannon_amd import filter_fp, _lib
    t_off = np.array([64, 100, 192], dtype=np.uint64)
    covers = np.full((2, 2), ~np.uint64(0), dtype=np.uint64)
    ctx.sync()
    ctx.timer_reset()
    with pytest.raises(_lib.ShannonError, match="n_covers is 0"):
        filter_fp.hits_from_bitmaps(ctx, covers[:0], t_off, 1)
    with pytest.raises(_lib.ShannonError, match="outside the window"):
        filter_fp.hits_from_bitmaps(ctx, covers, t_off, 2)                     # the window starts behind the first transcript
    with pytest.raises(_lib.ShannonError, match="outside the window"):
        filter_fp.hits_from_bitmaps(ctx, covers[:, :1], t_off, 1)              # ... ends before the last one does
    with pytest.raises(_lib.ShannonError, match="not monotone"):
        filter_fp.hits_from_bitmaps(ctx, covers, t_off[::-1], 1)
    ctx.sync()
    assert "filter_fp.merge" not in ctx.timers()
    assert filter_fp.hits_from_bitmaps(ctx, covers, t_off, 1).tolist() == [36, 92]
    assert filter_fp.hits_from_bitmaps(ctx, covers, t_off[:1], 1).tolist() == []                # (no transcript: nothing to do)
    ctx.sync()
    assert ctx.timers()["filter_fp.merge"][1] == 1
