"""GPU: the set-up of the contig extension against the brute force of tests/ext_setup_cases.py, array by array -- weights and flags
(ext_prepare_kernel), the one-line dictionary (fd_build_kernel, fd_match), the adjacency rows of both orientations
(ext_records_kernel), the seeds and their order (ext_seed_kernel, the two sorts, ext_seed_rank_kernel) -- through the hooks
shn_debug_ext_setup and shn_debug_fine_dict, which call the product functions unchanged and run no walk.  Integer work: every
comparison is exact."""
import ctypes as C
import numpy as np
import pytest
import ext_setup_cases as ec
from primitives_hooks import table_create, table_view

pytestmark = pytest.mark.gpu

SHN_ERR_ARG = -1
POISON32, POISON8 = 0x5A5A5A5A, 0x5A


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data if a.size else None


def ext_setup(ctx, t, min_weight):
    """every output of shn_debug_ext_setup, in arrays that were poisoned before the call"""
    from shannon_amd import _lib
    n = len(t)
    out = {"weight": np.full(n, POISON32, np.uint32), "flags": np.full(n, POISON8, np.uint8), "rows": np.full((2 * n, 8), POISON32, np.int32),
           "rec_weight": np.full(2 * n, POISON32, np.uint32), "seed_rank": np.full(2 * n, POISON32, np.uint32)}
    order = np.full(2 * n + 1, POISON32, np.uint32)
    ns = C.c_uint64(POISON32)
    _lib.check(_lib.lib().shn_debug_ext_setup(ctx.h, t.h, int(min_weight), _ptr(out["weight"]), _ptr(out["flags"]), _ptr(out["rows"]),
                                             _ptr(out["rec_weight"]), _ptr(out["seed_rank"]), C.byref(ns), order.ctypes.data))
    assert ns.value <= 2 * n and (order[ns.value:] == POISON32).all()
    out["order"] = order[:ns.value].copy()
    return out


def fine_dict(ctx, t, queries):
    """(id word, home line) per query and the four statistics of shn_debug_fine_dict"""
    from shannon_amd import _lib
    queries = np.ascontiguousarray(queries, dtype=np.uint64)
    ids, home = np.full(len(queries), POISON32 - 1, np.uint32), np.full(len(queries), POISON32, np.uint64)
    stats = np.full(4, POISON32, np.uint64)
    _lib.check(_lib.lib().shn_debug_fine_dict(ctx.h, t.h, _ptr(queries), len(queries), _ptr(ids), _ptr(home), stats.ctypes.data))
    return ids, home, stats


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, the first at %s (%r, expected %r)" % (what, len(bad), want.size, first, got[first], want[first]))


def check_setup(ctx, t, min_weight, got=None):
    """every output of the set-up hook equals the reference computed from the downloaded table; returns (outputs, reference)"""
    keys, counts = t.download()
    ref = ec.reference(keys, counts, t.k, t.canonical, min_weight)
    got = ext_setup(ctx, t, min_weight) if got is None else got
    _same("flags", got["flags"], ref.flags)
    _same("weight", got["weight"], ref.weight)
    _same("rows", got["rows"], ref.rows)
    _same("record weights of the orientations that exist", got["rec_weight"][ref.exists], np.repeat(ref.weight, 2)[ref.exists])
    _same("number of seeds", np.int64(len(got["order"])), np.int64(len(ref.order)))
    _same("seed order", got["order"], ref.order)
    _same("seed ranks", got["seed_rank"], ref.seed_rank)
    return got, ref


def make(ctx, name):
    case = ec.table(name)
    t = table_create(ctx, case.keys, case.counts, case.k, case.canonical)
    assert len(t) == len(case.keys)
    return t


@pytest.mark.parametrize("name,min_weight", ec.SIZE_RUNS)
def test_sizes_around_a_lane_group_a_wavefront_and_a_seed_block(ctx, name, min_weight):
    t = make(ctx, name)
    try:
        got, ref = check_setup(ctx, t, min_weight)
        if name == "size_5000":
            assert len(got["order"]) == {1: 10000, 7: 0}.get(min_weight, len(ref.order))
    finally:
        t.close()


@pytest.fixture(scope="module")
def tail(ctx):
    """the table of 70,001 k1-mers and what the default grid makes of it"""
    t = make(ctx, "tail")
    got, ref = check_setup(ctx, t, 3)
    yield t, got
    t.close()


@pytest.mark.parametrize("blocks", ec.TAIL_BLOCKS)
def test_a_records_grid_that_strides(ctx, tail, blocks, monkeypatch):
    """SHN_EXT_ADJ_BLOCKS caps the grid of ext_records_kernel: its loop runs again (as it does above 134 M k1-mers), the last trip with
    a partial wavefront -- the same arrays as from the default grid, and as from the reference"""
    t, whole = tail
    assert 8 * len(t) > 256 * blocks and (8 * len(t)) % 64
    monkeypatch.setenv("SHN_EXT_ADJ_BLOCKS", str(blocks))
    got, _ = check_setup(ctx, t, 3)
    for name in whole:
        _same(name + " against the default grid", got[name], whole[name])


@pytest.mark.parametrize("min_weight", [1, 4])
@pytest.mark.parametrize("name", ec.SMALL_K)
def test_every_k1mer_at_small_k(ctx, name, min_weight):
    """all 4^k strings (forward tables) or their canonical halves: every neighbour exists, most k1-mers are low-complexity, at even k
    every palindrome is there; six counts, so the seed order is mostly ties"""
    t = make(ctx, name)
    try:
        check_setup(ctx, t, min_weight)
    finally:
        t.close()


@pytest.mark.parametrize("name", ec.EDGE_K)
def test_k1_32_31_20_with_planted_edges(ctx, name):
    t = make(ctx, name)
    try:
        check_setup(ctx, t, 3)
    finally:
        t.close()


@pytest.mark.parametrize("name", ec.WEIGHTS)
def test_weights_at_the_clamp_and_around_bit_31(ctx, name):
    t = make(ctx, name)
    try:
        got, ref = check_setup(ctx, t, 3)
        if name == "weights_extreme":
            assert {0xFFFFFFFE, 0xFFFFFFFF, 0x80000000} <= set(got["weight"].tolist())
    finally:
        t.close()


def check_dictionary(ctx, t, absent):
    """every stored key is found with its index and palindrome bit, low-complexity keys, absent keys and key 0 are not; returns
    (home lines of the table's keys, statistics)"""
    keys, counts = t.download()
    ref = ec.reference(keys, counts, t.k, t.canonical, 3)
    queries = np.concatenate([keys, np.asarray(absent, dtype=np.uint64), np.zeros(1, np.uint64)])
    want = ec.expected_ids(keys, ref.flags, queries)
    n = len(keys)
    assert (want[:n][(ref.flags & 2) == 0] != ec.NONE32).all() and (want[n:] == ec.NONE32).all()
    ids, home, stats = fine_dict(ctx, t, queries)
    _same("id words", ids, want)
    return keys, home, stats


def test_dictionary_lines_that_overflow_four_times(ctx):
    """45 keys homed at one line and 8 at the next and the one after the next but one, 15 at another, 12 at the last hashed line, 20
    each at two more (ext_setup_cases.collision_case says why): the hop loop of fd_match, the tally in the count word, the keys stored
    in the spare lines, the key stored nowhere and found through the table; and the records made through that dictionary"""
    c = ec.collision_case()
    t = make(ctx, ec.COLLIDE)
    try:
        bits, layout, _ = table_view(ctx, t)
        assert layout == 0
        absent = np.concatenate([c.absent, c.low_complexity])
        keys, home, stats = check_dictionary(ctx, t, absent)
        n = len(keys)
        _same("home lines", home, ec.home_lines(np.concatenate([keys, absent, np.zeros(1, np.uint64)]), c.lines).astype(np.uint64))
        assert int(stats[0]) == c.lines == 1025
        assert int(stats[1]) >= 5, "lines over FD_SLOTS: %d" % int(stats[1])
        assert int(stats[2]) >= 30, "keys stored away from home: %d" % int(stats[2])
        assert int(stats[3]) >= 1, "keys stored in no line: %d" % int(stats[3])
        assert set(home[n:n + 200].tolist()) == {c.L, c.L + 1, c.L + 2, c.L + 3, c.M, c.last}
        check_setup(ctx, t, 3)
    finally:
        t.close()


def layout1_table(ctx, k1, both, monkeypatch):
    from shannon_amd import device
    monkeypatch.setenv("SHN_COUNT_DIRECT", "0")
    monkeypatch.setenv("SHN_COUNT_SK", "2")
    d = device.Reads.from_codes(ctx, ec.layout1_reads(k1))
    try:
        t = device.count_k1mers(ctx, [d], k1, both)
    finally:
        d.close()
    bits, layout, _ = table_view(ctx, t)
    assert layout == 1 and t.canonical == both and t.k == k1
    return t


@pytest.mark.parametrize("k1,both", ec.LAYOUT1)
def test_tables_of_the_minimizer_layout(ctx, k1, both, monkeypatch):
    """tables whose buckets are minimizers: the records kernel derives the eight neighbours' buckets from the k1-mer's own m-mers (8 to
    18 windows over the eight lanes); records, seeds and dictionary against the reference of the downloaded table"""
    t = layout1_table(ctx, k1, both, monkeypatch)
    try:
        keys, counts = t.download()
        assert 3000 < len(keys) < 70001
        got, ref = check_setup(ctx, t, 3)
        assert (ref.flags & 2).any() and (k1 % 2 or not both or (ref.flags & 1).any())
        assert ((ref.rows[:, :4] >= 0).sum(axis=1) > 1).any() and len(ref.order) > 1000
        absent = ec._random_keys(np.random.default_rng(k1), 1000, k1, both, avoid=keys)
        check_dictionary(ctx, t, absent)
    finally:
        t.close()


def _walks(ctx, t):
    from shannon_amd import extension_correction as xc
    ext = xc.Extension(ctx, t, 3)
    try:
        stats = [a.copy() for a in ext.stats()]
    finally:
        ext.close()
    res = xc.run_correction(ctx, t, 3, 30, 500, want_allowed=False)
    return stats, res.contigs


@pytest.mark.parametrize("which", ["collide", "layout1"])
def test_the_product_path_on_the_same_tables(ctx, which, monkeypatch):
    """shn_extend itself on the collision table and on a table of the minimizer layout: seed_info of every rank is (string, weight) of
    the reference's order, weights() of present, absent and low-complexity strings is the reference's; and the walks do not depend on
    the records kernel's grid"""
    from shannon_amd import extension_correction as xc
    t = make(ctx, ec.COLLIDE) if which == "collide" else layout1_table(ctx, 26, True, monkeypatch)
    try:
        keys, counts = t.download()
        ref = ec.reference(keys, counts, t.k, t.canonical, 3)
        ext = xc.Extension(ctx, t, 3)
        try:
            assert ext.n_walks == len(ref.order)
            skeys, sw = ext.seed_info(np.arange(len(ref.order), dtype=np.uint32))
            _same("seed strings", skeys, ref.strings[ref.order])
            _same("seed weights", sw, ref.weight[ref.order >> 1])
            rng = np.random.default_rng(7)
            alive = np.flatnonzero(ref.alive)
            lc = np.flatnonzero((ref.flags & 2) != 0)
            assert len(lc)
            absent = ec._random_keys(rng, 150, t.k, False, avoid=ref.strings)
            lowc = np.concatenate([keys[lc], ec.revcomp(keys[lc], t.k)])[:50]
            n_present = 500 - len(absent) - len(lowc)
            present = ref.strings[rng.choice(alive, n_present, replace=False)]
            q = np.concatenate([present, absent, lowc])
            want = np.zeros(len(q), np.uint32)
            where = {s: o for o, s in enumerate(ref.strings.tolist()) if ref.alive[o]}
            for i, s in enumerate(q.tolist()):
                if s in where:
                    want[i] = ref.weight[where[s] >> 1]
            assert len(q) == 500 and (want[:n_present] > 0).all() and (want[n_present:] == 0).all()
            _same("weights", ext.weights(q), want)
        finally:
            ext.close()
        stats, contigs = _walks(ctx, t)
        monkeypatch.setenv("SHN_EXT_ADJ_BLOCKS", "1")
        stats1, contigs1 = _walks(ctx, t)
        assert contigs1 == contigs and (which == "collide" or len(contigs) >= 2)      # (the 4,000 bases the reads come from, on both strands)
        for a, b in zip(stats, stats1):
            assert np.array_equal(a, b)
    finally:
        t.close()


def test_refusals_leave_the_context_usable(ctx):
    from shannon_amd import _lib
    L = _lib.lib()
    t = make(ctx, "size_9")
    try:
        ids = np.zeros(4, np.uint32)
        assert L.shn_debug_fine_dict(ctx.h, None, None, 0, None, None, None) == SHN_ERR_ARG
        assert L.shn_debug_fine_dict(ctx.h, t.h, None, 4, ids.ctypes.data, None, None) == SHN_ERR_ARG
        assert b"shn_debug_fine_dict" in L.shn_last_error()
        assert L.shn_debug_ext_setup(ctx.h, None, 3, None, None, None, None, None, None, None) == SHN_ERR_ARG
        assert b"shn_debug_ext_setup" in L.shn_last_error()
        _lib.check(L.shn_debug_ext_setup(ctx.h, t.h, 3, None, None, None, None, None, None, None))      # every output is optional
        _lib.check(L.shn_debug_fine_dict(ctx.h, t.h, None, 0, None, None, None))
        check_setup(ctx, t, 3)
        check_dictionary(ctx, t, np.zeros(0, np.uint64))
    finally:
        t.close()
