"""GPU: the walks of the contig extension (csrc/extend.hip) and the readers of a finished extension (csrc/ext_results.hip) on the
planted k1-mer graphs of tests/ext_walk_cases.py, against the sequential reference there -- every rank's n_right, n_left and
tot_weight and every contig, under the default schedule and under every switch that changes how the fixpoint is reached.  The tables
are built with shn_table_create and the reference is computed from the downloaded table, as in tests/test_ext_setup_gpu.py.  Integer
work: every comparison is exact.  Every extension runs with max_iterations = 2000, so a fixpoint that is not reached comes back as
the "did not converge" error."""
import math
import os
import subprocess
import sys
import numpy as np
import pytest
import ext_setup_cases as ec
import ext_walk_cases as wc
from primitives_hooks import table_create

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHN_ERR_ARG = -1
NONE32 = ec.NONE32
MAX_ITERATIONS = 2000

SCHEDULE_CASES = ("chain_canon", "loops_canon", "lengths_26_canon", "dense_6_canon", "dense_7_fwd")
SCHEDULES = ({"LIMIT0": 16, "GROW": 2, "TAIL": 0}, {"LIMIT0": 64, "GROW": 2}, {"BULK": 1}, {"BULK": 1, "DENSE": 1}, {"BULK": 1, "DENSE": 1000000000},
             {"LOGS": 0}, {"BULK": 1, "LOG_CHUNKS": 64}, {"POOL_WORDS": 256}, {"PROMOTE": 4, "LONG_WALK": 2}, {"PROMOTE": 1000000}, {"PRECISE": 0},
             {"MEMO_RELEASE": 0}, {"PREPASS": 0}, {"LIMIT0": 16, "GROW": 2, "PREPASS": 0, "BULK": 1})
READER_CASES = ("lengths_26_canon", "loops_canon", "heavy")
SHARD_CASES = ("chain_canon", "loops_canon", "lengths_26_fwd")


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def make(ctx, name):
    case = wc.table(name)
    t = table_create(ctx, case.keys, case.counts, case.k, case.canonical)
    assert len(t) == len(case.keys)
    return t


_EXPECTED = {}


def expected(t, name, min_weight):
    """(Ref, Walks) of the downloaded table; computed once per case, the download compared with the one it was computed from"""
    keys, counts = t.download()
    if (name, min_weight) not in _EXPECTED:
        ref = ec.reference(keys, counts, t.k, t.canonical, min_weight)
        w = wc.walk_reference(ref, t.k)
        for a in (keys, counts, w.n_right, w.n_left, w.tot_weight):
            a.setflags(write=False)
        _EXPECTED[(name, min_weight)] = (keys, counts, ref, w)
    k0, c0, ref, w = _EXPECTED[(name, min_weight)]
    assert np.array_equal(keys, k0) and np.array_equal(counts, c0), "the table of %s came back in another order" % name
    return ref, w


def set_switches(monkeypatch, switches=None):
    monkeypatch.setenv("SHN_EXT_AUDIT", "2")
    for name, value in (switches or {}).items():
        monkeypatch.setenv("SHN_EXT_" + name, str(value))


def extend(ctx, t, min_weight, **kw):
    from shannon_amd import extension_correction as xc
    return xc.Extension(ctx, t, min_weight, max_iterations=MAX_ITERATIONS, **kw)


def _first_difference(what, got, want, ref, k):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    r = int(bad[0])
    return "%s: %d of %d ranks differ, the first is rank %d (seed %s): %r, expected %r" % (
        what, len(bad), len(want), r, ec.str_of(ref.strings[ref.order[r]], k), got[r], want[r])


def check_stats(stats, ref, w, k, what=""):
    """n_right, n_left and tot_weight of every rank; the message names the first rank that differs and its seed"""
    nr, nl, tw = stats
    assert len(nr) == len(nl) == len(tw) == len(ref.order), "%s%d walks, expected %d" % (what, len(nr), len(ref.order))
    assert nr.dtype == np.uint32 and nl.dtype == np.uint32 and tw.dtype == np.uint64
    for name, got, want in (("n_right", nr, w.n_right), ("n_left", nl, w.n_left), ("tot_weight", tw, w.tot_weight)):
        if not np.array_equal(got, want):
            raise AssertionError(_first_difference(what + name, got, want, ref, k))


def check_contigs(ext, ref, w, k, what=""):
    live = wc.live_of(w)
    if not len(live):
        return
    lengths = w.n_right[live].astype(np.int64) + w.n_left[live] + k
    got = ext.emit(live.astype(np.uint32), lengths)
    want = [w.contigs[r] for r in live.tolist()]
    if got != want:
        full_got, full_want = np.full(len(ref.order), None, object), np.full(len(ref.order), None, object)
        full_got[live], full_want[live] = got, want
        raise AssertionError(_first_difference(what + "contig", full_got, full_want, ref, k))


def check_extension(ext, ref, w, k, what=""):
    assert ext.n_walks == len(ref.order), "%s%d walks, expected %d" % (what, ext.n_walks, len(ref.order))
    stats = ext.stats()
    check_stats(stats, ref, w, k, what)
    check_contigs(ext, ref, w, k, what)
    return stats


# ---------------------------------------------------------------- a. the walks
@pytest.mark.parametrize("name,min_weight", wc.CASES)
def test_walks_equal_the_reference(ctx, name, min_weight, monkeypatch):
    set_switches(monkeypatch)
    t = make(ctx, name)
    try:
        ref, w = expected(t, name, min_weight)
        ext = extend(ctx, t, min_weight)
        try:
            first = check_extension(ext, ref, w, t.k)
            if name in wc.LENGTHS + wc.CHAINS + wc.DENSE:
                assert ext.wave_steps > 0
            if name in wc.CHAINS:
                assert ext.iterations > 1
        finally:
            ext.close()
        ext = extend(ctx, t, min_weight)
        try:
            second = check_extension(ext, ref, w, t.k, "second run: ")
        finally:
            ext.close()
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
    finally:
        t.close()


# ---------------------------------------------------------------- b. the same under every schedule
@pytest.mark.parametrize("switches", SCHEDULES, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
@pytest.mark.parametrize("name", SCHEDULE_CASES)
def test_every_schedule_reaches_the_same_walks(ctx, name, switches, monkeypatch):
    set_switches(monkeypatch, switches)
    t = make(ctx, name)
    try:
        ref, w = expected(t, name, 3)
        ext = extend(ctx, t, 3)
        try:
            check_extension(ext, ref, w, t.k)
        finally:
            ext.close()
    finally:
        t.close()


# ---------------------------------------------------------------- c. the readers
@pytest.fixture(scope="module", params=READER_CASES)
def walked(ctx, request):
    """(table, finished extension, Ref, Walks) of a case under the default switches"""
    name = request.param
    old = os.environ.get("SHN_EXT_AUDIT")
    os.environ["SHN_EXT_AUDIT"] = "2"
    try:
        t = make(ctx, name)
        ref, w = expected(t, name, 3)
        ext = extend(ctx, t, 3)
    finally:
        if old is None:
            del os.environ["SHN_EXT_AUDIT"]
        else:
            os.environ["SHN_EXT_AUDIT"] = old
    check_stats(ext.stats(), ref, w, t.k)
    yield t, ext, ref, w
    ext.close()
    t.close()


def _lengths_of(w, ranks, k):
    return w.n_right[ranks].astype(np.int64) + w.n_left[ranks] + k


def test_live_stats_filter_by_steps(ctx, walked):
    t, ext, ref, w = walked
    live = wc.live_of(w)
    steps = w.n_right[live].astype(np.int64) + w.n_left[live]
    seen = set()
    for m in (0, 1, 16, 17, 1000, 100000):
        want = live[steps >= m]
        rank, nr, nl, tw = ext.live_stats(m)
        assert np.array_equal(rank, want.astype(np.uint32)), "live_stats(%d): ranks" % m
        assert np.array_equal(nr, w.n_right[want]) and np.array_equal(nl, w.n_left[want]) and np.array_equal(tw, w.tot_weight[want]), "live_stats(%d)" % m
        assert tw.dtype == np.uint64
        seen.add(len(want))
    assert 0 in seen and len(live) in seen


def test_stats_range_and_its_refusal(ctx, walked):
    from shannon_amd import _lib
    t, ext, ref, w = walked
    ns = len(ref.order)
    assert ns > 65
    rng = np.random.default_rng(ns)
    lo = int(rng.integers(1, ns - 2))
    inner = (lo, int(rng.integers(1, ns - lo)))
    for lo, n in ((0, 0), (0, 1), (63, 2), (ns - 1, 1), (ns, 0), inner):
        nr, nl, tw = ext.stats_range(lo, n)
        assert len(nr) == n
        assert np.array_equal(nr, w.n_right[lo:lo + n]) and np.array_equal(nl, w.n_left[lo:lo + n]) and np.array_equal(tw, w.tot_weight[lo:lo + n]), (lo, n)
    L = _lib.lib()
    nr, nl, tw = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    for lo, n in ((ns, 1), (ns - 1, 2), (ns + 5, 0)):
        assert L.shn_ext_stats_range(ctx.h, ext.h, lo, n, nr.ctypes.data, nl.ctypes.data, tw.ctypes.data) == SHN_ERR_ARG
        assert b"outside the walks" in L.shn_last_error()
        a, b, c = ext.stats_range(ns - 1, 1)
        assert a[0] == w.n_right[ns - 1] and b[0] == w.n_left[ns - 1] and c[0] == w.tot_weight[ns - 1]


def test_seed_info_of_every_rank(ctx, walked):
    t, ext, ref, w = walked
    skeys, sw = ext.seed_info(np.arange(len(ref.order), dtype=np.uint32))
    assert np.array_equal(skeys, ref.strings[ref.order]) and np.array_equal(sw, ref.weight[ref.order >> 1])
    p = np.random.default_rng(3).permutation(len(ref.order))[:100].astype(np.uint32)
    skeys, sw = ext.seed_info(p)
    assert np.array_equal(skeys, ref.strings[ref.order[p]]) and np.array_equal(sw, ref.weight[ref.order[p] >> 1])


def test_accept_is_the_filter_on_the_reference_numbers(ctx, walked):
    """extension_correction.py:361 -- len >= min_length and len * avg_weight ** 0.25 >= 2 * min_length * min_weight ** 0.25 -- with
    math.pow on the reference's lengths and totals"""
    t, ext, ref, w = walked
    k = t.k
    n_kept = set()
    for min_length, min_weight in ((27, 1), (40, 3), (200, 5)):
        want_r, want_l = [], []
        for r in wc.live_of(w).tolist():
            n_kmers = int(w.n_right[r]) + int(w.n_left[r]) + 1
            length = n_kmers + k - 1
            avg = int(w.tot_weight[r]) / max(1, n_kmers)
            if length >= min_length and length * math.pow(avg, 1 / 4.0) >= 2 * min_length * math.pow(min_weight, 1 / 4.0):
                want_r.append(r), want_l.append(length)
        ranks, lengths = ext.accept(k, min_length, min_weight)
        assert ranks.tolist() == want_r and lengths.tolist() == want_l, (min_length, min_weight)
        n_kept.add(len(want_r))
    assert max(n_kept) > 0


def test_emit_of_subsets_on_the_host_and_on_the_device(ctx, walked):
    from shannon_amd import extension_correction as xc
    t, ext, ref, w = walked
    k = t.k
    live = wc.live_of(w)
    rng = np.random.default_rng(len(live))
    sub = rng.permutation(live)[:max(2, len(live) // 2)].astype(np.uint32)
    if (np.diff(sub.astype(np.int64)) > 0).all():
        sub = sub[::-1].copy()
    assert ext.emit(sub, _lengths_of(w, sub, k)) == [w.contigs[r] for r in sub.tolist()]
    longest = live[np.argmax(_lengths_of(w, live, k))]
    for r in (int(live[0]), int(live[-1]), int(longest)):
        assert ext.emit(np.array([r], np.uint32), _lengths_of(w, np.array([r]), k)) == [w.contigs[r]]
    dev, offs = ext.emit_device(live.astype(np.uint32), _lengths_of(w, live, k))
    try:
        idx = rng.permutation(len(live))
        buf, out_off = dev.segments(offs, idx)
        assert xc.split_strings(buf, out_off) == [w.contigs[live[i]] for i in idx.tolist()]
        buf, out_off = dev.segments(offs, idx[:1])
        assert xc.split_strings(buf, out_off) == [w.contigs[live[idx[0]]]]
    finally:
        dev.close()


def test_emit_and_seed_info_refuse_and_go_on(ctx, walked):
    """a rank selected twice, a room that is not the contig's length (too long, too short -- which must not be overrun --, shorter than
    a k1-mer), a rank beyond the walks: SHN_ERR_ARG each, and the next call on the context is right"""
    from shannon_amd import _lib
    t, ext, ref, w = walked
    L = _lib.lib()
    k = t.k
    ns = len(ref.order)
    live = wc.live_of(w)
    steps = w.n_right[live].astype(np.int64) + w.n_left[live]
    a, b = int(live[np.argmax(steps)]), int(live[0] if live[0] != live[np.argmax(steps)] else live[1])
    assert steps.max() >= 2

    def emit_rc(ranks, lengths):
        ranks = np.array(ranks, dtype=np.uint32)
        offs = np.zeros(len(ranks) + 1, np.uint64)
        offs[1:] = np.cumsum(lengths)
        buf = np.zeros(int(offs[-1]) + 1, np.uint8)
        return L.shn_ext_emit(ctx.h, ext.h, ranks.ctypes.data, len(ranks), offs.ctypes.data, buf.ctypes.data)

    def still_right():
        two = np.array([b, a], np.uint32)
        assert ext.emit(two, _lengths_of(w, two, k)) == [w.contigs[b], w.contigs[a]]

    la, lb = int(_lengths_of(w, np.array([a]), k)[0]), int(_lengths_of(w, np.array([b]), k)[0])
    assert emit_rc([a, b], [la, lb]) == 0
    for what, ranks, lengths, message in (("twice", [a, b, a], [la, lb, la], b"selected twice"), ("too long", [a, b], [la + 1, lb], b"do not fit"),
                                          ("too short", [a, b], [la - 1, lb], b"do not fit"), ("the last too short", [b, a], [lb, la - 1], b"do not fit"),
                                          ("shorter than a k1-mer", [a, b], [la, k - 1], b"do not fit"), ("rank ns", [a, ns], [la, k], b"out of range"),
                                          ("rank 2^32 - 1", [NONE32], [k], b"out of range")):
        assert emit_rc(ranks, lengths) == SHN_ERR_ARG, what
        assert message in L.shn_last_error(), (what, L.shn_last_error())
        still_right()
    ranks = np.array([0, ns], np.uint32)
    keys, sw = np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    assert L.shn_ext_seed_info(ctx.h, ext.h, ranks.ctypes.data, 2, keys.ctypes.data, sw.ctypes.data) == SHN_ERR_ARG
    assert b"out of range" in L.shn_last_error()
    skeys, sw = ext.seed_info(np.array([0, ns - 1], np.uint32))
    assert np.array_equal(skeys, ref.strings[ref.order[[0, ns - 1]]])
    still_right()


# ---------------------------------------------------------------- d. blocks handed over
def test_blocks_are_handed_over_final_and_in_order(ctx, monkeypatch):
    set_switches(monkeypatch, {"LIMIT0": 16, "GROW": 2})
    t = make(ctx, "chain_canon")
    try:
        ref, w = expected(t, "chain_canon", 3)
        calls, wrong = [], []

        def on_block(view, lo, hi, status):
            calls.append((lo, hi, status))
            if status >= 0 and hi > lo:
                nr, nl, tw = view.stats_range(lo, hi - lo)
                if not (np.array_equal(nr, w.n_right[lo:hi]) and np.array_equal(nl, w.n_left[lo:hi]) and np.array_equal(tw, w.tot_weight[lo:hi])):
                    wrong.append((lo, hi))

        ext = extend(ctx, t, 3, on_block=on_block)
        try:
            check_extension(ext, ref, w, t.k)
            ns = ext.n_walks
        finally:
            ext.close()
        assert not wrong, "blocks handed over before they were final: %s" % wrong[:5]
        assert all(status >= 0 for _, _, status in calls), "a healthy run voids nothing"
        assert [status for _, _, status in calls] == [0] * (len(calls) - 1) + [1] and len(calls) >= 4
        edges = [lo for lo, _, _ in calls] + [calls[-1][1]]
        assert edges[0] == 0 and edges[-1] == ns and edges == sorted(edges)
        assert all(calls[i][1] == calls[i + 1][0] for i in range(len(calls) - 1))
        assert calls[0][:2] == (0, 16)
    finally:
        t.close()


# ---------------------------------------------------------------- e. shards
@pytest.mark.parametrize("name", SHARD_CASES)
def test_three_shards_hold_every_live_walk_once(ctx, name, monkeypatch):
    set_switches(monkeypatch)
    t = make(ctx, name)
    try:
        ref, w = expected(t, name, 3)
        k = t.k
        want = {int(ref.strings[ref.order[r]]): (int(w.n_right[r]), int(w.n_left[r]), int(w.tot_weight[r]), w.contigs[r]) for r in wc.live_of(w).tolist()}
        got, n_seeds = {}, 0
        for rank in range(3):
            ext = extend(ctx, t, 3, shard=(3, rank))
            try:
                ns = ext.n_walks
                n_seeds += ns
                if not ns:
                    continue
                nr, nl, tw = ext.stats()
                live = np.flatnonzero(nr != NONE32).astype(np.uint32)
                skeys, sw = ext.seed_info(np.arange(ns, dtype=np.uint32))
                order = np.lexsort((skeys, NONE32 - sw.astype(np.int64)))
                assert np.array_equal(order, np.arange(ns)), "shard %d: its walks are not in (weight descending, string ascending) order" % rank
                contigs = ext.emit(live, nr[live].astype(np.int64) + nl[live] + k) if len(live) else []
                for r, c in zip(live.tolist(), contigs):
                    s = int(skeys[r])
                    assert s not in got, "the walk seeded at %s is in two shards" % ec.str_of(s, k)
                    got[s] = (int(nr[r]), int(nl[r]), int(tw[r]), c)
            finally:
                ext.close()
        assert n_seeds == len(ref.order)
        assert set(got) == set(want), "live walks: %d missing, %d not expected" % (len(set(want) - set(got)), len(set(got) - set(want)))
        for s in sorted(want):
            assert got[s] == want[s], "the walk seeded at %s: %r, expected %r" % (ec.str_of(s, k), got[s][:3], want[s][:3])
    finally:
        t.close()


# ---------------------------------------------------------------- f. poison
def test_the_walks_with_every_workspace_request_poisoned():
    """SHN_DEV_POISON=165 SHN_DEV_POISON_WS=1 (read once per process, hence the child): every allocator block and, on every request,
    every workspace slot is filled with 0xA5 first.  A walker, a mark pass or a reader that relies on what an earlier call left behind
    gives wrong ranks; the child counts them, twice over"""
    p = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "ext_walks_poison_worker.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=dict(os.environ, SHN_DEV_POISON="165", SHN_DEV_POISON_WS="1"), timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    words = p.stdout.split()
    counts = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert counts == {"chain_canon": 0, "dense_6_canon": 0, "lengths_26_canon": 0}, counts
