"""CPU: the checkers of tests/primitives_cases.py reject wrong answers, and its inputs can tell a right primitive from a wrong one
(numpy alone; the GPU side is tests/test_primitives_gpu.py)."""
import numpy as np
import pytest
import primitives_cases as pc

U64 = np.uint64


# ---------------------------------------------------------------- the checkers reject wrong answers
def _sorted_case(name):
    c = pc.sort_case(name)
    order = pc.stable_order(c.keys, c.lo, c.hi)
    return c, c.keys[order].copy(), c.vals[order].copy()


def _first_tie(c, ks):
    m = pc.masked(ks, c.lo, c.hi)
    return int(np.flatnonzero(m[1:] == m[:-1])[0])


def test_sort_checkers_accept_the_stable_sort():
    for name in ("range_0_26_random_outside", "distinct17_4097", "range_5_5_random_outside", "range_8_0_random_outside", "range_0_64_zero_outside",
                 "size_0_b0_64", "size_1_b0_24"):
        c, ks, vs = _sorted_case(name)
        pc.check_sorted_pairs(c.keys, c.vals, ks, vs, c.lo, c.hi)
        pc.check_sorted_keys(c.keys, ks, c.lo, c.hi)
    c = pc.sort_case("range_8_0_random_outside")                       # an empty range: the output is the input
    pc.check_sorted_pairs(c.keys, c.vals, c.keys, c.vals, c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, np.sort(c.keys), c.lo, c.hi)


def test_sort_checkers_reject_two_tied_elements_swapped():
    c, ks, vs = _sorted_case("range_0_26_random_outside")
    i = _first_tie(c, ks)
    assert ks[i] != ks[i + 1]                                           # (tied inside the range, different outside: the words tell)
    ks[[i, i + 1]] = ks[[i + 1, i]]
    vs[[i, i + 1]] = vs[[i + 1, i]]
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, ks, vs, c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, ks, c.lo, c.hi)
    c, ks, vs = _sorted_case("distinct17_4097")                        # equal words: only the values tell
    i = _first_tie(c, ks)
    vs[[i, i + 1]] = vs[[i + 1, i]]
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, ks, vs, c.lo, c.hi)


@pytest.mark.parametrize("name", ["range_0_26_random_outside", "range_0_33_random_outside", "range_32_62_random_outside"])
def test_sort_checkers_reject_the_range_rounded_up_to_whole_digits(name):
    c = pc.sort_case(name)
    order = pc.stable_order(c.keys, c.lo, pc.rounded_hi(c.lo, c.hi))
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, c.keys[order], c.vals[order], c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, c.keys[order], c.lo, c.hi)


def test_sort_checkers_reject_a_changed_or_duplicated_element():
    c, ks, vs = _sorted_case("range_0_26_random_outside")
    bad = vs.copy()
    bad[len(bad) // 2] ^= 1                                             # one value changed
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, ks, bad, c.lo, c.hi)
    bad = ks.copy()
    bad[7] ^= U64(1 << 63)                                              # one bit outside the range changed
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, bad, vs, c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, bad, c.lo, c.hi)
    bk, bv = ks.copy(), vs.copy()
    bk[100], bv[100] = bk[99], bv[99]                                   # one element duplicated over its neighbour
    with pytest.raises(AssertionError):
        pc.check_sorted_pairs(c.keys, c.vals, bk, bv, c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, bk, c.lo, c.hi)
    with pytest.raises(AssertionError):
        pc.check_sorted_keys(c.keys, ks[:-1], c.lo, c.hi)


def test_scan_checker():
    v = pc.scan_case("ones32_1025")
    want = np.concatenate([[0], np.cumsum(v.astype(np.uint64))]).astype(np.uint64)
    pc.check_scan(v, want, want[-1])
    pc.check_scan(pc.scan_case("zeros_0"), np.zeros(1, np.uint64), 0)
    with pytest.raises(AssertionError):                                 # off by one element: the inclusive scan
        pc.check_scan(v, np.concatenate([want[1:], want[-1:]]), want[-1])
    wrapped = np.concatenate([[0], np.cumsum(v, dtype=np.uint32)]).astype(np.uint64)
    assert wrapped[-1] != want[-1]
    with pytest.raises(AssertionError):                                 # summed in 32 bits: wraps
        pc.check_scan(v, wrapped, wrapped[-1])
    with pytest.raises(AssertionError):
        pc.check_scan(v, want, int(want[-1]) + 1)                        # a total that is not out[n]
    with pytest.raises(AssertionError):
        pc.check_scan(v, want.astype(np.int64), want[-1])
    r = pc.scan_case("random_1025")
    good = np.concatenate([[0], np.cumsum(r.astype(np.uint64))]).astype(np.uint64)
    bad = good.copy()
    bad[700] += U64(1)
    with pytest.raises(AssertionError):
        pc.check_scan(r, bad, good[-1])


def _good_runs(name):
    c = pc.run_case(name)
    st = pc.run_starts(c.keys, c.shift)
    n = len(c.keys)
    head = np.zeros(n, dtype=np.uint64)
    head[st] = 1
    return c, [len(st), c.keys[st].copy(), np.r_[st, n].astype(np.uint32), np.diff(np.r_[st, n]).astype(np.uint32),
               np.r_[0, np.cumsum(head)].astype(np.uint64)]


def test_runs_checker_accepts_the_reference_and_rejects_four_wrong_answers():
    for name in pc.RUN_CASES:
        c, good = _good_runs(name)
        pc.check_runs(c.keys, c.shift, *good)
    c, good = _good_runs("random_runs_1025")
    n_runs, rk, start, length, pos = good
    with pytest.raises(AssertionError):                                 # the last run missing
        pc.check_runs(c.keys, c.shift, n_runs - 1, rk[:-1], np.r_[start[:-2], start[-1:]], length[:-1], pos)
    bad = start.copy()
    bad[-1] -= 1                                                        # start[n_runs] is not n
    with pytest.raises(AssertionError):
        pc.check_runs(c.keys, c.shift, n_runs, rk, bad, length, pos)
    bad = length.copy()
    bad[len(bad) // 2] += 1                                             # a length off by one
    with pytest.raises(AssertionError):
        pc.check_runs(c.keys, c.shift, n_runs, rk, start, bad, pos)
    with pytest.raises(AssertionError):
        pc.check_runs(c.keys, c.shift, n_runs, rk, start, length - np.uint32(1), pos)
    c, good = _good_runs("shift20_1025")                                # the runs of the whole keys: split where the bits below the shift change
    st0 = pc.run_starts(c.keys, 0)
    assert len(st0) > good[0]
    n = len(c.keys)
    head = np.zeros(n, dtype=np.uint64)
    head[st0] = 1
    with pytest.raises(AssertionError):
        pc.check_runs(c.keys, c.shift, len(st0), c.keys[st0], np.r_[st0, n].astype(np.uint32), np.diff(np.r_[st0, n]).astype(np.uint32),
                      np.r_[0, np.cumsum(head)].astype(np.uint64))
    with pytest.raises(AssertionError):                                 # the first key of a run, not its shifted form
        pc.check_runs(c.keys, c.shift, good[0], good[1] >> U64(c.shift), *good[2:])


def test_run_cases_are_what_they_claim():
    assert len(set(pc.RUN_CASES)) == len(pc.RUN_CASES) == len(pc.RUN_SIZES) * len(pc.RUN_PATTERNS)
    for name in pc.RUN_CASES:
        c = pc.run_case(name)
        n = int(name.rsplit("_", 1)[1])
        k = c.keys >> U64(c.shift)
        assert c.keys.dtype == np.uint64 and len(c.keys) == n and (k[1:] >= k[:-1]).all()
    for n in pc.RUN_SIZES:
        runs = {p: pc.run_starts(*pc.run_case("%s_%d" % (p, n))) for p in pc.RUN_PATTERNS}
        assert len(runs["all_equal"]) == min(n, 1) and len(runs["all_distinct"]) == n
        if n >= 2:
            b = pc.run_case("bit63_%d" % n).keys
            assert len(runs["bit63"]) == 2 and int(b[0]) ^ int(b[-1]) == 1 << 63
        if n >= 3:
            e = runs["edge_runs"]
            assert e[1] == 1 and e[-1] == n - 1                         # a first and a last run of one element
        if n:
            assert int(pc.run_case("all_ones_%d" % n).keys[-1]) == pc.ALL64
        if n >= 255:
            s = pc.run_case("shift20_%d" % n)
            assert s.shift == 20 and 2 * len(runs["shift20"]) < len(pc.run_starts(s.keys, 0))     # ignoring the shift splits most runs
            assert 1 < len(runs["random_runs"]) < n


def test_find_checker():
    tk = np.array([40, 10, 30, 20], dtype=np.uint64)                    # (download order: by bucket, not by key)
    q = np.array([10, 11, 20, 40, 0], dtype=np.uint64)
    good = np.array([1, -1, 3, 0, -1], dtype=np.int64)
    pc.check_find(tk, q, good)
    pc.check_find(tk, q, good, want=pc.expected_find(tk, q))
    for at, wrong in ((0, 2), (2, -1), (1, 0), (4, 3)):                 # the wrong position, -1 for a hit, a hit for a miss
        bad = good.copy()
        bad[at] = wrong
        with pytest.raises(AssertionError):
            pc.check_find(tk, q, bad)
    with pytest.raises(AssertionError):                                 # a key stored twice has no "one index"
        pc.check_find(np.array([10, 20, 10], dtype=np.uint64), q, good)
    with pytest.raises(AssertionError):
        pc.check_find(tk, q, good.astype(np.int32))


def test_reduce_by_key_and_the_content_checker():
    keys = np.array([5, 3, 5, 9, 3, 5], dtype=np.uint64)
    cnts = np.array([1, 2, 0xFFFFFFFF, 4, 5, 6], dtype=np.uint32)
    uk, sums = pc.reduce_by_key(keys, cnts)
    assert uk.tolist() == [3, 5, 9] and sums.tolist() == [7, 0xFFFFFFFF + 7, 4] and sums.dtype == np.uint64
    small = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint32)
    pc.check_table_content(keys, small, np.array([9, 3, 5], dtype=np.uint64), np.array([4, 7, 10], dtype=np.uint32))
    for tk, tc in (([9, 3, 5], [4, 7, 11]), ([9, 3], [4, 7]), ([9, 3, 5, 5], [4, 7, 4, 6]), ([9, 3, 6], [4, 7, 10])):
        with pytest.raises(AssertionError):
            pc.check_table_content(keys, small, np.array(tk, dtype=np.uint64), np.array(tc, dtype=np.uint32))


def test_fmix64_is_the_one_of_the_exchange():
    from shannon_amd import exchange
    x = np.concatenate([pc.table_case("uniform_k32").keys, np.array([0, 1, pc.ALL64], dtype=np.uint64)])
    assert np.array_equal(pc.fmix64(x), exchange.fmix64_np(x))


# ---------------------------------------------------------------- the inputs can tell right from wrong
def test_sort_case_list_is_the_stated_one():
    assert len(set(pc.SORT_CASES)) == len(pc.SORT_CASES) == 2 * len(pc.SORT_SIZES) + 2 * len(pc.SHAPES) + 2 * len(pc.RANGES)
    for n in pc.SORT_SIZES:
        assert len(pc.sort_case("size_%d_b0_64" % n).keys) == n
    for name in pc.SORT_CASES:
        c = pc.sort_case(name)
        assert c.keys.dtype == np.uint64 and c.vals.dtype == np.uint32 and np.array_equal(c.vals, np.arange(len(c.keys)))
    # an odd and an even number of passes: both return buffers of shn_sort_keys, the copy-back branch of shn_sort_pairs and its absence
    passes = {(pc.rounded_hi(lo, hi) - lo) // 8 if hi > lo else 0 for lo, hi in pc.RANGES}
    assert {p & 1 for p in passes} == {0, 1} and 0 in passes
    z = pc.sort_case("zeros_4097")
    assert not z.keys.any() and len(z.keys) % pc.TILE == 1               # a last tile of one real zero key beside 4,095 padding lanes
    d = pc.sort_case("digits256_70001")
    cnt = np.bincount(d.keys.astype(np.int64), minlength=256)
    assert len(cnt) == 256 and cnt.max() - cnt.min() <= 1
    lane = pc.sort_case("lane_digit_4097").keys
    assert all(len(set(lane[r:r + 64].tolist())) == 64 for r in range(0, 4096, 64))


@pytest.mark.parametrize("name", pc.TIE_CASES)
def test_tie_cases_hold_ties(name):
    c = pc.sort_case(name)
    _u, inv, cnt = np.unique(pc.masked(c.keys, c.lo, c.hi), return_inverse=True, return_counts=True)
    assert 2 * int((cnt[inv] > 1).sum()) >= len(c.keys)


@pytest.mark.parametrize("name", pc.ZERO_OUTSIDE_CASES + pc.RANDOM_OUTSIDE_CASES)
def test_range_cases(name):
    c = pc.sort_case(name)
    assert len(c.keys) == pc.RANGE_N
    keep = (pc.range_mask(c.lo, c.hi) << c.lo) & pc.ALL64 if c.hi > c.lo else 0
    outside = c.keys & U64(pc.ALL64 ^ keep)
    if name.endswith("_zero_outside"):
        assert not outside.any()                                        # today's callers' case
    elif keep != pc.ALL64:
        assert len(np.unique(outside)) >= 4                             # live bits on both sides of the range where it has two sides
    if c.hi > c.lo:                                                     # ties inside the range, so that stability is on trial too
        _u, inv, cnt = np.unique(pc.masked(c.keys, c.lo, c.hi), return_inverse=True, return_counts=True)
        assert 4 * int((cnt[inv] > 1).sum()) >= len(c.keys)
    if name.endswith("_random_outside") and c.hi > c.lo and (c.hi - c.lo) % 8:
        exact = pc.stable_order(c.keys, c.lo, c.hi)
        rounded = pc.stable_order(c.keys, c.lo, pc.rounded_hi(c.lo, c.hi))
        assert pc.rounded_hi(c.lo, c.hi) <= 64
        assert int((exact != rounded).sum()) * 100 >= len(c.keys)      # a sort by whole digits is wrong in at least 1 % of the positions


def test_the_widths_that_need_a_masked_last_digit_are_among_the_cases():
    odd = sorted((hi - lo) for lo, hi in pc.RANGES if hi > lo and (hi - lo) % 8)
    assert odd == [26, 30, 33, 50, 62]
    assert (3, 19) in pc.RANGES                                         # 16 wide from bit 3: two whole digits, neither byte-aligned


def test_scan_cases():
    assert len(pc.SCAN_CASES) == len(pc.SCAN_SIZES) * len(pc.SCAN_VALUES)
    for n in pc.SCAN_SIZES:
        v = pc.scan_case("ones32_%d" % n)
        assert len(v) == n and v.dtype == np.uint32
        if n >= 2:
            assert int(v.astype(np.uint64).sum()) > 1 << 32
            assert int(v[:4].astype(np.uint64).sum()) > 1 << 32 or n < 4   # ... inside the first thread's four elements already
    assert [(n + 1023) // 1024 for n in pc.SCAN_SIZES if n > 1 << 20][0] == 1025      # per = 2: the upper half of the threads get nothing
    f = pc.scan_case("flags97_%d" % ((1 << 21) + 5))
    assert set(np.unique(f).tolist()) == {0, 1} and abs(int(f.sum()) * 97 - len(f)) < len(f) // 10
    one = pc.scan_case("final_one_1025")
    assert int(one.sum()) == 1 and one[-1] == 1


@pytest.mark.parametrize("name", pc.TABLE_CASES)
def test_table_cases(name):
    c = pc.table_case(name)
    top = pc._key_mask(c.k)
    assert c.keys.dtype == np.uint64 and c.counts.dtype == np.uint32 and len(c.keys) == len(c.counts)
    assert not len(c.keys) or int(c.keys.max()) <= top
    uk, sums = pc.table_reference(name)
    assert not len(sums) or int(sums.max()) < 1 << 32                   # (sums past 2^32 are not part of this)
    q = pc.table_queries(name)
    assert int(q.max()) <= top and q[-2] == 0 and q[-1] == top
    hit = np.isin(q, uk)
    if len(c.keys) >= 5000 and name != "uniform_k2":                   # (k = 2: all 16 keys there are are stored -- nothing can miss)
        assert int(hit.sum()) >= 1000 and int((~hit).sum()) >= 1000
    assert np.array_equal(pc.reference_counts(name, q)[hit] > 0, np.ones(int(hit.sum()), bool))
    assert not pc.reference_counts(name, q)[~hit].any()


def test_table_cases_are_what_they_claim():
    assert [len(pc.table_case("n%d" % n).keys) for n in (0, 1, 2, 3, 96, 97)] == [0, 1, 2, 3, 96, 97]
    assert pc.start_bits(96) == 0 and pc.start_bits(97) == 1           # 97: the first n with more than one bucket
    assert len(pc.table_reference("uniform_k2")[0]) <= 256
    k32 = pc.table_case("uniform_k32").keys
    assert int((k32 == U64(pc.ALL64)).sum()) >= 2
    for name, top16 in (("top16_ones", 0xFFFF), ("top16_zeros", 0)):
        c = pc.table_case(name)
        assert len(c.keys) == 20000 and set((c.keys >> U64(2 * c.k - 16)).tolist()) == {top16}
    c = pc.table_case("clustered")
    s = np.sort(c.keys)
    assert len(s) == 50000 and c.k == 31 and np.array_equal(s - s[0], np.arange(50000, dtype=np.uint64))
    assert len(set((c.keys >> U64(62 - 16)).tolist())) == 1             # one interpolated first guess for every query of a bucket
    c = pc.table_case("one_key")
    assert len(c.keys) == 100000 and len(np.unique(c.keys)) == 1 and set(c.counts.tolist()) == {3}
    c = pc.table_case("dups")
    assert len(c.keys) == 60000 and len(np.unique(c.keys)) == 20000


def test_retry_case_overflows_one_first_bucket_and_no_second():
    c = pc.table_case("retry")
    assert len(c.keys) == len(np.unique(c.keys)) == 100000 and c.k == 25 and int(c.keys.max()) < 1 << 50
    bits = pc.start_bits(len(c.keys))
    assert bits == 11
    first = np.bincount(pc.bucket_of(c.keys, bits), minlength=1 << bits)
    assert int((first > pc.CAP_LIMIT).sum()) == 1
    second = np.bincount(pc.bucket_of(c.keys, bits + 2), minlength=1 << (bits + 2))
    assert int(second.max()) <= pc.CAP_LIMIT
    heavy = int(np.argmax(first))
    assert all(second[4 * heavy + s] >= 300 for s in range(4))          # the heavy bucket's keys fall on all four sub-buckets
