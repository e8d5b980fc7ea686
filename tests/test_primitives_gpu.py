"""GPU: the shared device primitives, each against a plain numpy reference through its test hook (csrc/debug_hooks.hip) -- the radix
sort (shn_sort_pairs, shn_sort_keys), the scan (shn_device_scan_u32), the runs of a sorted array (shn_sorted_runs), the three bucket searches of csrc/common.h (shn_table_find,
shn_table_find_k, shn_tab_find) and the two table builds (shn_table_create on the host, shn_table_from_pairs on the device).  The
inputs and checkers are tests/primitives_cases.py; tests/test_primitives_cases.py shows on the CPU that they tell right from wrong."""
import os, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT
import primitives_cases as pc
import primitives_hooks as ph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(ctx):
    """(table, downloaded keys, downloaded counts) of a table case by one of the two builds, made once"""
    cache = {}

    def get(name, how):
        if (name, how) not in cache:
            c = pc.table_case(name)
            t = ph.BUILDS[how](ctx, c.keys, c.counts, c.k, c.canonical)
            tk, tc = t.download()
            cache[(name, how)] = (t, tk, tc)
        return cache[(name, how)]
    yield get
    for t, _tk, _tc in cache.values():
        t.close()


# ---------------------------------------------------------------- sort
@pytest.mark.parametrize("name", pc.SORT_CASES)
def test_sort_pairs_is_the_stable_sort_by_the_exact_bit_range(ctx, name):
    c = pc.sort_case(name)
    ko, vo = ph.sort_pairs(ctx, c.keys, c.vals, c.lo, c.hi)
    pc.check_sorted_pairs(c.keys, c.vals, ko, vo, c.lo, c.hi)


@pytest.mark.parametrize("name", pc.SORT_CASES)
def test_sort_keys_is_the_stable_sort_by_the_exact_bit_range(ctx, name):
    c = pc.sort_case(name)
    pc.check_sorted_keys(c.keys, ph.sort_keys(ctx, c.keys, c.lo, c.hi), c.lo, c.hi)


def test_sort_hooks_refuse_a_range_outside_the_word(ctx):
    from shannon_amd import _lib
    k = np.arange(4, dtype=np.uint64)
    for lo, hi in ((-1, 8), (0, 65), (65, 70)):
        with pytest.raises(_lib.ShannonError):
            ph.sort_keys(ctx, k, lo, hi)
        with pytest.raises(_lib.ShannonError):
            ph.sort_pairs(ctx, k, k.astype(np.uint32), lo, hi)


# ---------------------------------------------------------------- scan
@pytest.mark.parametrize("name", pc.SCAN_CASES)
def test_scan_with_and_without_the_host_total(ctx, name):
    v = pc.scan_case(name)
    for with_total in (True, False):
        out, total = ph.scan(ctx, v, with_total)
        pc.check_scan(v, out, total)


# ---------------------------------------------------------------- runs
@pytest.mark.parametrize("name", pc.RUN_CASES)
def test_sorted_runs_heads_keys_starts_lengths_and_positions(ctx, name):
    """shn_sorted_runs with everything wanted (its scan and scatter are shn_runs_from_heads').  The refusal of 2^32 keys or more is not
    tested: it would take 32 GB of keys."""
    c = pc.run_case(name)
    pc.check_runs(c.keys, c.shift, *ph.sorted_runs(ctx, c.keys, c.shift))


# ---------------------------------------------------------------- tables: content
@pytest.mark.parametrize("how", sorted(ph.BUILDS))
@pytest.mark.parametrize("name", pc.TABLE_CASES)
def test_table_content(ctx, built, name, how):
    c = pc.table_case(name)
    t, tk, tc = built(name, how)
    uk, sums = pc.table_reference(name)
    assert len(t) == len(uk) and t.k == c.k and t.canonical == bool(c.canonical)
    pc.check_table_content(c.keys, c.counts, tk, tc)
    assert t.total == int(c.counts.astype(np.uint64).sum())
    bits, layout, off = ph.table_view(ctx, t, offsets=True)
    assert layout == 0
    # grouped by bucket (the top bits of the key's hash), ascending inside a bucket, the offsets those of the groups
    b = pc.bucket_of(tk, bits)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(b, minlength=1 << bits))]).astype(np.uint64))
    assert (np.diff(b) >= 0).all() and (tk[1:] > tk[:-1])[np.diff(b) == 0].all()
    q = pc.table_queries(name)
    got = t.lookup(q)
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), pc.reference_counts(name, q))


# ---------------------------------------------------------------- tables: the three searches
@pytest.mark.parametrize("how", sorted(ph.BUILDS))
@pytest.mark.parametrize("name", pc.TABLE_CASES)
def test_table_searches(ctx, built, name, how):
    t, tk, _tc = built(name, how)
    q = pc.table_queries(name)
    want = pc.expected_find(tk, q)
    uk, _sums = pc.table_reference(name)
    assert np.array_equal(want >= 0, np.isin(q, uk))                    # (the download holds the reference's keys: test_table_content)
    for variant in (0, 1, 2):
        pc.check_find(tk, q, ph.find(ctx, t, q, variant), want=want)


def test_the_gallop_of_the_clustered_case_runs_past_its_first_steps(ctx, built):
    """all keys of `clustered` share their top 16 bits, so the interpolated first guess of shn_table_find_k is the same end of the
    bucket for every query: in a bucket of 64 keys the gallop doubles its step six times before the bisection takes over"""
    for how in sorted(ph.BUILDS):
        t, _tk, _tc = built("clustered", how)
        _bits, _layout, off = ph.table_view(ctx, t, offsets=True)
        assert int(np.diff(off.astype(np.int64)).max()) >= 64


def test_find_hook_arguments(ctx, built):
    from shannon_amd import _lib
    t, tk, _tc = built("n97", "create")
    rc, _idx = ph.find_rc(ctx, t, tk, 3)
    assert rc == -1
    assert len(ph.find(ctx, t, np.zeros(0, np.uint64), 1)) == 0
    with pytest.raises(_lib.ShannonError, match="variant"):
        ph.find(ctx, t, tk, -1)


# ---------------------------------------------------------------- the super-k-mer layout
def test_the_searches_on_a_table_of_the_minimizer_layout(ctx, monkeypatch):
    """SHN_COUNT_SK is read at every call (csrc/count_sk.hip): 2 sends 3,000 reads through the super-k-mer path, whose tables are
    bucketed by minimizer (layout 1).  shn_tab_find finds every stored key where the download has it; the two searches that know the
    hashed buckets only are refused."""
    from shannon_amd import device
    monkeypatch.setenv("SHN_COUNT_SK", "2")
    rng = np.random.default_rng(20)
    reads = device.Reads.from_codes(ctx, rng.integers(0, 4, size=(3000, 100), dtype=np.uint8))
    t = device.count_k1mers(ctx, [reads], 26)
    try:
        _bits, layout, _off = ph.table_view(ctx, t)
        assert layout == 1
        tk, tc = t.download()
        assert len(tk) > 100000
        top = (1 << 52) - 1
        q = np.concatenate([tk, np.minimum(tk + np.uint64(1), np.uint64(top)), rng.integers(0, 1 << 52, size=2000, dtype=np.uint64),
                            np.array([0, top], dtype=np.uint64)])
        want = pc.expected_find(tk, q)
        assert int((want >= 0).sum()) >= len(tk) and int((want < 0).sum()) >= 1000
        pc.check_find(tk, q, ph.find(ctx, t, q, 2), want=want)
        assert np.array_equal(t.lookup(q), np.where(want >= 0, tc[np.maximum(want, 0)], 0))
        for variant in (0, 1):
            rc, idx = ph.find_rc(ctx, t, q, variant)
            assert rc == -1 and (idx == -7).all()                       # SHN_ERR_ARG, nothing written
    finally:
        t.close()
        reads.close()


# ---------------------------------------------------------------- the retry of shn_table_from_pairs
def test_from_pairs_tries_again_with_more_buckets_after_a_bucket_overflows(ctx, built):
    """`retry`: 1,200 of 100,000 distinct keys lie in ONE of the 2^11 buckets the build starts with -- more distinct keys than a
    bucket's LDS table takes (950) -- and spread over its four sub-buckets at 13 bits: the first attempt overflows, the second
    (bits += 2) does not.  Content and searches of the result are held by test_table_content / test_table_searches[retry-from_pairs];
    here: the table that came out is the second attempt's."""
    c = pc.table_case("retry")
    assert pc.start_bits(len(c.keys)) == 11
    t, tk, tc = built("retry", "from_pairs")
    bits, _layout, off = ph.table_view(ctx, t, offsets=True)
    assert bits >= 13 and len(off) - 1 >= 1 << 13
    assert int(np.diff(off.astype(np.int64)).max()) <= pc.CAP_LIMIT
    pc.check_table_content(c.keys, c.counts, tk, tc)
    # the host build of the same pairs keeps the 11 bits (no LDS table there): one bucket of more than 950 keys, searched all the same
    th, _tkh, _tch = built("retry", "create")
    bits_h, _l, off_h = ph.table_view(ctx, th, offsets=True)
    assert bits_h == 11 and int(np.diff(off_h.astype(np.int64)).max()) > pc.CAP_LIMIT


# ---------------------------------------------------------------- poisoned workspaces
def test_the_primitives_with_every_workspace_request_poisoned():
    """SHN_DEV_POISON=165 SHN_DEV_POISON_WS=1 (read once per process, hence the child): every allocator block and, on every request,
    every workspace slot is filled with 0xA5 first.  A primitive that reads a slot it did not write -- the sort's histogram, the scan's
    block sums, the runs' positions, the build's cursors -- gives wrong elements; the child counts them."""
    p = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "tests", "primitives_poison_worker.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=dict(os.environ, SHN_DEV_POISON="165", SHN_DEV_POISON_WS="1"), timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    words = p.stdout.split()
    counts = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert counts == {"FIND": 0, "RUNS": 0, "SCAN": 0, "SORT_KEYS": 0, "SORT_PAIRS": 0, "TABLE": 0}, counts
