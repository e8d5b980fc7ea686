"""shn_probe_build (csrc/probe_gpu.hip: the k1mers2component table read routing looks up) against the brute force of
tests/probe_cases.py, path by path: k1-mers of one partition, of exactly two (pg_pair_kernel, the pair sort over
32 + shn_bits_for(n_parts) bits, pg_pair_patch_kernel), of three or more (pg_multi_kernel, the host's interning map,
pg_patch_kernel) and that path's relaunch above 65,536 windows; key widths 2 .. 32; degenerate shapes; refusals; and the table
handed to the routing kernel.  Every comparison is exact.  Every case first asserts, from the brute force alone, that its input
reaches the path it is named for (probe_cases.require)."""
import ctypes as C
import numpy as np
import pytest
import probe_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def _build(ctx, text, off, n_contigs, part_of, n_parts, k1):
    """(return code, probe handle) of one shn_probe_build"""
    from shannon_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().shn_probe_build(ctx.h, text.ctypes.data if text is not None else None, off.ctypes.data if off is not None else None, n_contigs,
                                    part_of.ctypes.data if part_of is not None else None, n_parts, k1, C.byref(h))
    return rc, h


def _sets_of(h):
    from shannon_amd import _lib
    L = _lib.lib()
    n_sets, n_mem = int(L.shn_probe_n_sets(h)), int(L.shn_probe_n_members(h))
    set_off = np.full(n_sets + 1, 0xFFFFFFFF, dtype=np.uint32)
    set_mem = np.full(max(n_mem, 1), 0xFFFFFFFF, dtype=np.uint32)
    _lib.check(L.shn_probe_sets(h, set_off.ctypes.data, set_mem.ctypes.data))
    return set_off, set_mem[:n_mem]


def probe_of(ctx, parts, k1):
    """shn_probe_build on the contigs of `parts`: ({key: member tuple of its set}, set_off, set_mem).  The table of the probe
    object is borrowed (shn_probe_destroy frees it): it is downloaded through the library, never wrapped in a device.Table."""
    from shannon_amd import _lib
    L = _lib.lib()
    text, off, part_of, n = pc.flatten(parts)
    rc, h = _build(ctx, text, off, n, part_of, len(parts), k1)
    _lib.check(rc)
    try:
        set_off, set_mem = _sets_of(h)
        th = L.shn_probe_table(h)
        assert th
        nk = int(L.shn_table_size(th))
        keys, vals = np.empty(nk, dtype=np.uint64), np.empty(nk, dtype=np.uint32)
        _lib.check(L.shn_table_download(ctx.h, th, keys.ctypes.data, vals.ctypes.data))
    finally:
        L.shn_probe_destroy(h)
    assert len(set_off) >= 1 and set_off[0] == 0 and int(set_off[-1]) == len(set_mem) and (np.diff(set_off.astype(np.int64)) >= 1).all()
    assert len(np.unique(keys)) == nk, "a key twice in the table"
    assert nk == 0 or (1 <= int(vals.min()) and int(vals.max()) <= len(set_off) - 1), "a value that names no set"
    so, sm = set_off.tolist(), set_mem.tolist()
    table = {k: tuple(sm[so[v - 1]:so[v]]) for k, v in zip(keys.tolist(), vals.tolist())}
    return table, set_off, set_mem, dict(zip(keys.tolist(), vals.tolist()))


def check_case(ctx, parts, k1, need):
    """everything the issue asks of a case; returns the brute-force sets"""
    sets, _runs = pc.require(parts, k1, need)
    n_parts = len(parts)
    table, set_off, set_mem, value_of = probe_of(ctx, parts, k1)
    want = {pc.key_of(km): s for km, s in sets.items()}
    assert len(want) == len(sets)
    # the keys are exactly the distinct k1-windows
    assert sorted(table) == sorted(want)
    # every member list strictly ascending and, as a set, the brute force's
    wrong = [(k, table[k], sorted(want[k])) for k in want if list(table[k]) != sorted(want[k])]
    assert not wrong, "%d of %d k1-mers with a wrong set, the first: key %#x got %r want %r" % ((len(wrong), len(want)) + wrong[0])
    # sets 0 .. n_parts - 1 are the singletons {p}
    assert len(set_off) - 1 >= n_parts
    assert np.array_equal(set_off[:n_parts + 1], np.arange(n_parts + 1)) and np.array_equal(set_mem[:n_parts], np.arange(n_parts))
    # no member list under two set ids, and no set that no k1-mer names: the sets beyond the singletons are the distinct sets of
    # several partitions, once each
    so, sm = set_off.tolist(), set_mem.tolist()
    lists = [tuple(sm[so[i]:so[i + 1]]) for i in range(len(so) - 1)]
    assert len(set(lists)) == len(lists), "a member list under two set ids"
    assert all(list(m) == sorted(set(m)) for m in lists[n_parts:])
    assert set(lists[n_parts:]) == set(tuple(sorted(s)) for s in sets.values() if len(s) > 1)
    # a k1-mer of one partition names the singleton itself
    assert all(value_of[k] == next(iter(want[k])) + 1 for k in want if len(want[k]) == 1)
    return sets


# ---- one partition per k1-mer

def test_single_a_k1mer_repeated_inside_one_contig(ctx):
    check_case(ctx, *pc.single_repeat_in_contig())


def test_single_a_k1mer_on_two_contigs_of_one_partition(ctx):
    """runs longer than one window whose partitions are all the same: multi stays 0, the value is the singleton"""
    check_case(ctx, *pc.single_shared_in_partition())


# ---- exactly two partitions

@pytest.mark.parametrize("n_parts", pc.PAIR_N_PARTS)
def test_pair_path_at_the_digit_edges_of_the_pair_sort(ctx, n_parts):
    """pairs (0, 1), (0, n_parts - 1), (n_parts - 2, n_parts - 1) and more, many k1-mers on a pair and a pair of one k1-mer, runs
    (p, p, q) and (p, q, q); n_parts at the edges of the sort's 32 + shn_bits_for(n_parts) bits (most partitions empty)"""
    parts, k1, need = pc.pairs(n_parts)
    assert need["n3"] == 0 and need["n2"] > 0                        # the pair path alone
    check_case(ctx, parts, k1, need)


def test_pair_path_at_k1_32(ctx):
    check_case(ctx, *pc.pairs(257, 32))


# ---- three or more partitions

@pytest.mark.parametrize("k1", [21, 32])
def test_host_path_sets_of_3_4_and_40_partitions(ctx, k1):
    """k1-mers of 3, 4 and 40 partitions, one set reached from different contigs (one id), a run (p, q, q, r) -- and no k1-mer of
    exactly two partitions: the pair path has nothing to do"""
    parts, k1, need = pc.multi(k1)
    assert need["n2"] == 0 and need["n3"] > 0
    check_case(ctx, parts, k1, need)


@pytest.mark.parametrize("k1", [21, 26, 32])
def test_mixed_single_pair_and_host_path_in_one_call(ctx, k1):
    parts, k1, need = pc.mixed(k1)
    assert need["n1"] > 0 and need["n2"] > 0 and need["n3"] > 0
    check_case(ctx, parts, k1, need)


def test_relaunch_of_the_host_path_above_65536_windows(ctx):
    """66,000 windows on k1-mers of three partitions: pg_multi_kernel runs again with the room its first run counted; no window
    may be lost or doubled (the brute force counts them before the device is asked)"""
    parts, k1, need = pc.relaunch()
    assert need["windows3"] == 1 << 16
    check_case(ctx, parts, k1, need)


# ---- key width

def test_k1_2_sixteen_keys_in_long_runs(ctx):
    check_case(ctx, *pc.width_2())


def test_k1_32_poly_a_and_poly_t(ctx):
    """the all-zero and the all-ones key, each a k1-mer of its own (the table is not canonical), alone and shared"""
    parts, k1, need = pc.width_32_poly()
    sets = check_case(ctx, parts, k1, need)
    assert sets["A" * 32] == frozenset([0]) and sets["T" * 32] == frozenset([1, 4]) and sets["G" * 32] == frozenset([2, 3, 5])


# ---- degenerate shapes

@pytest.mark.parametrize("case", ["degenerate_lengths", "no_window", "all_empty", "no_contig", "empty_ends"])
def test_degenerate_shapes(ctx, case):
    """contigs shorter than k1, of exactly k1 bases, empty; no window at all; no contig; first and last partitions empty"""
    check_case(ctx, *getattr(pc, case)())


def test_no_contig_with_null_pointers(ctx):
    from shannon_amd import _lib
    rc, h = _build(ctx, None, None, 0, None, 4, 21)
    _lib.check(rc)
    try:
        set_off, set_mem = _sets_of(h)
        assert set_off.tolist() == [0, 1, 2, 3, 4] and set_mem.tolist() == [0, 1, 2, 3]
        assert int(_lib.lib().shn_table_size(_lib.lib().shn_probe_table(h))) == 0
    finally:
        _lib.lib().shn_probe_destroy(h)


# ---- refusals

def _refusals():
    parts, k1, _need = pc.mixed(21)
    text, off, part_of, n = pc.flatten(parts)
    desc = part_of.copy()
    desc[3], desc[4] = 5, 2
    assert desc[4] < desc[3] < len(parts)
    high = part_of.copy()
    high[n - 1] = len(parts)
    with_n = text.copy()
    with_n[int(off[2]) + 30] = ord("N")
    assert int(off[3]) - int(off[2]) > 30 + k1
    return {"part_of descending": ((text, off, n, desc, len(parts), k1), "ascending"),
            "part_of[c] >= n_parts": ((text, off, n, high, len(parts), k1), "< n_parts"),
            "k1 = 1": ((text, off, n, part_of, len(parts), 1), "bad argument"),
            "k1 = 33": ((text, off, n, part_of, len(parts), 33), "bad argument"),
            "a contig with N": ((with_n, off, n, part_of, len(parts), k1), "outside ACGT")}


@pytest.mark.parametrize("what", ["part_of descending", "part_of[c] >= n_parts", "k1 = 1", "k1 = 33", "a contig with N"])
def test_refusals_leave_the_context_usable(ctx, what):
    from shannon_amd import _lib
    (text, off, n, part_of, n_parts, k1), word = _refusals()[what]
    rc, h = _build(ctx, text, off, n, part_of, n_parts, k1)
    msg = _lib.lib().shn_last_error().decode()
    assert rc != 0 and not h.value, "%s was accepted" % what
    assert word in msg, msg
    if what == "a contig with N":
        assert "shn_contig_stage" not in msg, msg                    # (the check is shared with the contig stage: no caller's name)
    check_case(ctx, *pc.mixed(21))                                   # the next call answers, and correctly


# ---- end to end: the probe object's own table and sets under the routing kernel

@pytest.mark.parametrize("k1,mode", [(21, "se"), (32, "pe"), (21, "pe_ss")])
def test_routes_through_the_built_table_equal_get_comps(ctx, k1, mode):
    """reads drawn from the contigs of a mixed case (both strands), routed by shn_route_reads_mode over the table and the sets
    shn_probe_build made, against get_rmers / get_comps over the brute-force sets"""
    from oracle import seqs
    from shannon_amd import device, _lib, kmers_for_component as kfc
    from test_routing_gpu import _python_routes
    parts, k1, need = pc.mixed(k1)
    sets = pc.require(parts, k1, need)[0]
    paired, ss = mode != "se", mode == "pe_ss"
    L = 100
    r1 = pc.reads_from(parts, 240, L, 11)
    r2 = pc.reads_from(parts, 240, L, 12)
    if ss:
        files = seqs.strand_specific(r1, r2)
    else:
        files = list(seqs.double_strand_paired(r1, r2)) if paired else [seqs.double_strand_single(r1)]
    want = _python_routes(files, paired, ss, sets, k1)
    by_read = {}
    for p, d in want:
        by_read.setdefault(d, set()).add(p)
    assert any(len(s) == 1 for s in by_read.values()) and any(len(s) == 2 for s in by_read.values()) and any(len(s) >= 3 for s in by_read.values())
    assert len(by_read) < len(files[0])                              # some reads hit nothing
    lib = _lib.lib()
    text, off, part_of, n = pc.flatten(parts)
    rc, h = _build(ctx, text, off, n, part_of, len(parts), k1)
    _lib.check(rc)
    d1 = d2 = None
    try:
        set_off, set_mem = _sets_of(h)
        d1 = device.Reads.from_strings(ctx, r1)
        d2 = device.Reads.from_strings(ctx, r2) if paired else None
        rh = C.c_void_p()
        _lib.check(lib.shn_route_reads_mode(ctx.h, d1.h, d2.h if paired else None, k1, C.c_void_p(lib.shn_probe_table(h)), set_off.ctypes.data,
                                            set_mem.ctypes.data, len(set_off) - 1, 1 if ss else 0, C.byref(rh)))
        routes = kfc.Routes(ctx, rh)
        pid, ridx = routes.download()
        routes.close()
    finally:
        lib.shn_probe_destroy(h)
        for d in (d1, d2):
            if d is not None:
                d.close()
    assert list(zip(pid.tolist(), ridx.tolist())) == want
