"""GPU: shn_reads_collect (device.Reads.collect) -- the reads of resident sets as base codes one after the other -- against
device.RaggedCodes.take over the same reads on the host.  Fixed-length and ragged sets, two sets of different geometry in one
call, bases outside ACGT at the edges of the 32-base words and of the 64-base mask words, selections with repeats, empty, of one
read, and one that takes more than one pass of the grid; reads without a base; an output that ends exactly on a block."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 250)
EMPTY_LENS = [0, 5, 0, 0, 0, 33, 64, 0, 1, 0] * 30               # 300 reads: empty ones first, last and three in a row


def _with_n(codes, off, every=5):
    """a base outside ACGT at the first base, the last base and at bases 31 and 32 of every `every`-th read (where it has them)"""
    codes = codes.copy()
    for r in range(0, len(off) - 1, every):
        a, b = int(off[r]), int(off[r + 1])
        for p in (0, b - a - 1, 31, 32):
            if 0 <= p < b - a:
                codes[a + p] = 4
    return codes


def _ragged(rng, lens, with_n, every=5):
    from shannon_amd import device
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    codes = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    if with_n:
        codes = _with_n(codes, off, every)
    return device.RaggedCodes(codes, off)


def _fixed(rng, n, L, with_n):
    from shannon_amd import device
    return _ragged(rng, [L] * n, with_n), L


class _Sets(object):
    def __init__(self):
        from shannon_amd import device
        self.ctx = device.Context(0)
        self.host, self.dev = {}, {}
        rng = np.random.default_rng(11)
        for with_n in (False, True):
            tag = "N" if with_n else "acgt"
            self.add("ragged_" + tag, _ragged(rng, [LENS[i % len(LENS)] for i in range(312)], with_n), None)
            for L in (31, 32, 33, 64, 80, 100):
                self.add("L%d_%s" % (L, tag), *_fixed(rng, 300, L, with_n))
        self.add("short", _ragged(rng, [30 + (7 * i) % 67 for i in range(500)], True), None)
        for with_n in (False, True):
            self.add("empties_" + ("N" if with_n else "acgt"), _ragged(rng, EMPTY_LENS, with_n, every=3), None)

    def add(self, name, host, L):
        from shannon_amd import device
        self.host[name] = host
        self.dev[name] = (device.Reads.from_ragged(self.ctx, host.codes, host.off) if L is None
                          else device.Reads.from_codes(self.ctx, host.codes.reshape(len(host), L)))

    def close(self):
        for d in self.dev.values():
            d.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def sets():
    s = _Sets()
    yield s
    s.close()


def _expected(sets, a, b, sel, flags):
    """RaggedCodes.take over the reads of a followed by those of b"""
    from shannon_amd import device
    ha, hb = sets.host[a], (sets.host[b] if b else None)
    both = ha if hb is None else device.RaggedCodes(np.concatenate([ha.codes, hb.codes]), np.concatenate([ha.off, hb.off[1:] + ha.off[-1]]))
    codes, off = both.take(np.asarray(sel, dtype=np.int64) + np.asarray(flags, dtype=np.int64) * len(ha))
    return codes[:int(off[-1])], off


def _sizing(sets, a, b, sel, flags):
    from shannon_amd import _lib
    sel, flags = np.ascontiguousarray(sel, dtype=np.uint32), np.ascontiguousarray(flags, dtype=np.uint8)
    lens = np.zeros(max(len(sel), 1), np.uint32)
    total = C.c_uint64(12345)
    _lib.check(_lib.lib().shn_reads_collect(sets.ctx.h, sets.dev[a].h, sets.dev[b].h if b else None, sel.ctypes.data, flags.ctypes.data, len(sel),
                                            lens.ctypes.data, None, 0, C.byref(total)))
    return int(total.value), lens[:len(sel)]


def _check(sets, a, b, sel, flags):
    from shannon_amd import device
    codes, off = device.Reads.collect(sets.dev[a], sets.dev[b] if b else None, sel, flags)
    want, woff = _expected(sets, a, b, sel, flags)
    assert off.dtype == np.uint64 and np.array_equal(off, woff)
    assert codes.dtype == np.uint8 and np.array_equal(codes, want)
    total, lens = _sizing(sets, a, b, sel, flags)
    assert total == int(woff[-1]) and np.array_equal(lens, (woff[1:] - woff[:-1]).astype(np.uint32))


PAIRS = ([("ragged_%s" % t, None) for t in ("acgt", "N")] + [("L%d_%s" % (L, t), None) for L in (31, 32, 33, 64, 100) for t in ("acgt", "N")]
         + [("ragged_N", "ragged_acgt"), ("ragged_N", "L64_acgt"), ("ragged_acgt", "L33_N"), ("L100_N", "L80_N"), ("L100_acgt", "L80_acgt"),
            ("L100_acgt", "L80_N")])


@pytest.mark.parametrize("a,b", PAIRS, ids=["%s+%s" % (a, b) if b else a for a, b in PAIRS])
def test_collect_equals_the_host_take(sets, a, b):
    rng = np.random.default_rng(5)
    na, nb = len(sets.host[a]), (len(sets.host[b]) if b else 0)
    flags = rng.integers(0, 2, 1000).astype(np.uint8) if b else np.zeros(1000, np.uint8)
    sel = np.where(flags == 1, rng.integers(0, max(nb, 1), 1000), rng.integers(0, na, 1000)).astype(np.uint32)      # unsorted, with repeats
    _check(sets, a, b, sel, flags)
    _check(sets, a, b, np.arange(na, dtype=np.uint32), np.zeros(na, np.uint8))                                         # every read once, in order
    _check(sets, a, b, np.zeros(0, np.uint32), np.zeros(0, np.uint8))                                                  # nothing
    for one in (0, na - 1):
        _check(sets, a, b, np.array([one], np.uint32), np.zeros(1, np.uint8))
    if b:
        _check(sets, a, b, np.array([nb - 1], np.uint32), np.ones(1, np.uint8))


def test_a_selection_of_more_than_one_pass(sets):
    """70,000 short reads: more threads than the length pass launches, more bytes than one pass of the expansion writes"""
    rng = np.random.default_rng(6)
    sel = rng.integers(0, len(sets.host["short"]), 70000).astype(np.uint32)
    _check(sets, "short", None, sel, np.zeros(len(sel), np.uint8))
    flags = rng.integers(0, 2, len(sel)).astype(np.uint8)
    _check(sets, "short", "L31_acgt", np.where(flags == 1, sel % 300, sel).astype(np.uint32), flags)


@pytest.mark.parametrize("tag", ["acgt", "N"])
def test_a_ragged_set_with_empty_reads(sets, tag):
    """reads without a base are stepped over wherever they lie; a selection of nothing but such reads launches no expansion"""
    from shannon_amd import device
    name = "empties_" + tag
    n = len(sets.host[name])
    empty = np.nonzero(np.asarray(EMPTY_LENS) == 0)[0]
    assert n == 300 and len(empty) == 180 and empty[0] == 0 and empty[-1] == n - 1
    rng = np.random.default_rng(8)
    for sel in (np.arange(n), rng.integers(0, n, 1000), empty, empty[:1], np.array([n - 1])):
        _check(sets, name, None, sel.astype(np.uint32), np.zeros(len(sel), np.uint8))
    sets.ctx.timer_reset()
    codes, off = device.Reads.collect(sets.dev[name], None, empty.astype(np.uint32), np.zeros(len(empty), np.uint8))
    assert len(codes) == 0 and len(off) == len(empty) + 1 and not off.any()
    assert "reads.collect" not in sets.ctx.timers()


def _block_edge(sets):
    """128 reads of 32 bases = 4,096 codes: exactly one block of the expansion (256 threads x 16 bytes)"""
    sel = np.random.default_rng(9).integers(0, len(sets.host["L32_acgt"]), 128).astype(np.uint32)
    return sel, np.zeros(128, np.uint8)


def test_an_output_that_ends_on_a_block_and_one_code_behind_it(sets):
    sel, flags = _block_edge(sets)
    want, _off = _expected(sets, "L32_acgt", None, sel, flags)
    assert len(want) == 4096
    _check(sets, "L32_acgt", None, sel, flags)
    assert sets.host["ragged_acgt"].off[1] == 1                    # read 0 of the ragged set: one base
    sel, flags = np.append(sel, np.uint32(0)), np.append(flags, np.uint8(1))
    want, _off = _expected(sets, "L32_acgt", "ragged_acgt", sel, flags)
    assert len(want) == 4097
    _check(sets, "L32_acgt", "ragged_acgt", sel, flags)


def test_a_capacity_one_short_leaves_the_rest_of_the_buffer_alone(sets):
    """4,097 codes into codes_cap = 4,096: refused, and nothing is written at or behind the capacity"""
    from shannon_amd import _lib
    sel, flags = _block_edge(sets)
    sel, flags = np.append(sel, np.uint32(0)), np.append(flags, np.uint8(1))
    want, _off = _expected(sets, "L32_acgt", "ragged_acgt", sel, flags)
    assert len(want) == 4097
    buf = np.full(4097 + 64, 0xAB, np.uint8)
    total = C.c_uint64(0)
    rc = _lib.lib().shn_reads_collect(sets.ctx.h, sets.dev["L32_acgt"].h, sets.dev["ragged_acgt"].h, sel.ctypes.data, flags.ctypes.data, len(sel), None,
                                      buf.ctypes.data, 4096, C.byref(total))
    assert rc != 0 and "codes_cap" in _lib.lib().shn_last_error().decode()
    assert total.value == 4097                                     # (a ragged set: the device's total, known after the call)
    assert np.all(buf[4096:] == 0xAB)
    assert np.array_equal(buf[:4096], want[:4096])
    _check(sets, "L32_acgt", "ragged_acgt", sel, flags)            # the context stays usable


def test_bad_arguments_are_refused_and_the_context_stays_usable(sets):
    from shannon_amd import device, _lib
    a, b = sets.dev["ragged_N"], sets.dev["L80_N"]
    good = (np.array([3, 1, 2], np.uint32), np.array([0, 1, 0], np.uint8))

    def still_fine():
        _check(sets, "ragged_N", "L80_N", *good)
    still_fine()
    for sel, flags, second, what in (([len(a)], [0], b, "out of range"), ([len(b)], [1], b, "out of range"), ([0], [1], None, "b is NULL"),
                                     ([0], [2], b, "flags"), ([0], [3], b, "flags")):
        with pytest.raises(_lib.ShannonError, match=what):
            device.Reads.collect(a, second, np.array(sel, np.uint32), np.array(flags, np.uint8))
        still_fine()
    # a buffer one code too small: fixed-length sets (the host knows the total) and a ragged one (the device does)
    for first, name in ((sets.dev["L100_N"], "L100_N"), (a, "ragged_N")):
        sel, flags = np.array([5, 6, 7], np.uint32), np.zeros(3, np.uint8)
        want, _off = _expected(sets, name, None, sel, flags)
        buf = np.zeros(len(want), np.uint8)
        total = C.c_uint64(0)
        rc = _lib.lib().shn_reads_collect(sets.ctx.h, first.h, None, sel.ctypes.data, flags.ctypes.data, 3, None, buf.ctypes.data, len(want) - 1, C.byref(total))
        assert rc != 0 and "codes_cap" in _lib.lib().shn_last_error().decode()
        still_fine()
        rc = _lib.lib().shn_reads_collect(sets.ctx.h, first.h, None, sel.ctypes.data, flags.ctypes.data, 3, None, buf.ctypes.data, len(want), C.byref(total))
        assert rc == 0 and total.value == len(want) and np.array_equal(buf, want)
