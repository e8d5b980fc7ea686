"""Thin numpy wrappers of the primitives' test hooks (include/shannon_hip.h: shn_debug_sort_pairs ... shn_debug_table_view, shn_debug_sorted_runs) and the two
table builds, for tests/test_primitives_gpu.py and its child process tests/primitives_poison_worker.py."""
import ctypes as C
import numpy as np


def _L():
    from shannon_amd import _lib
    return _lib, _lib.lib()


def _ptr(a):
    return a.ctypes.data if a.size else None


def sort_pairs(ctx, keys, vals, lo, hi):
    _lib, L = _L()
    keys, vals = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(vals, dtype=np.uint32)
    ko, vo = np.full(len(keys), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), np.full(len(keys), 0x5A5A5A5A, dtype=np.uint32)
    _lib.check(L.shn_debug_sort_pairs(ctx.h, _ptr(keys), _ptr(vals), len(keys), lo, hi, _ptr(ko), _ptr(vo)))
    return ko, vo


def sort_keys(ctx, keys, lo, hi):
    _lib, L = _L()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    ko = np.full(len(keys), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    _lib.check(L.shn_debug_sort_keys(ctx.h, _ptr(keys), len(keys), lo, hi, _ptr(ko)))
    return ko


def scan(ctx, values, with_total):
    """(out uint64[n + 1], total): total from the host form of the scan, or out[n] of the device-only form"""
    _lib, L = _L()
    values = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.full(len(values) + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    total = C.c_uint64(0x5A5A5A5A)
    _lib.check(L.shn_debug_scan_u32(ctx.h, _ptr(values), len(values), out.ctypes.data, C.byref(total) if with_total else None))
    return out, (int(total.value) if with_total else int(out[-1]))


def sorted_runs(ctx, keys, shift):
    """(n_runs, run keys[n_runs], start[n_runs + 1], len[n_runs], pos[n + 1]) of keys sorted by (key >> shift)"""
    _lib, L = _L()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n = len(keys)
    rk, ln = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), np.full(n, 0x5A5A5A5A, dtype=np.uint32)
    st, pos = np.full(n + 1, 0x5A5A5A5A, dtype=np.uint32), np.full(n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    n_runs = C.c_uint64(0x5A5A5A5A)
    _lib.check(L.shn_debug_sorted_runs(ctx.h, _ptr(keys), n, int(shift), _ptr(rk), st.ctypes.data, _ptr(ln), pos.ctypes.data, C.byref(n_runs)))
    r = int(n_runs.value)
    assert r <= n
    return r, rk[:r], st[:r + 1], ln[:r], pos


def table_create(ctx, keys, counts, k, canonical):
    """the host build (shn_table_create lays tables of up to 2^22 pairs out on the host)"""
    from shannon_amd import device
    _lib, L = _L()
    keys, counts = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
    h = C.c_void_p()
    _lib.check(L.shn_table_create(ctx.h, _ptr(keys), _ptr(counts), len(keys), int(k), int(canonical), C.byref(h)))
    return device.Table(ctx, h)


def table_from_pairs(ctx, keys, counts, k, canonical):
    """the device pipeline (shn_table_from_pairs) on device tensors"""
    import torch
    from shannon_amd import device
    dk = torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).to("cuda:%d" % ctx.device)
    dc = torch.from_numpy(np.array(counts, dtype=np.uint32).view(np.int32)).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    t = device.Table.from_pairs(ctx, dk.data_ptr() if len(keys) else 0, dc.data_ptr() if len(keys) else 0, len(keys), int(k), bool(canonical))
    ctx.sync()
    return t


BUILDS = {"create": table_create, "from_pairs": table_from_pairs}


def find_rc(ctx, table, queries, variant):
    """(return code, idx int64[n])"""
    _lib, L = _L()
    queries = np.ascontiguousarray(queries, dtype=np.uint64)
    idx = np.full(len(queries), -7, dtype=np.int64)
    rc = L.shn_debug_table_find(ctx.h, table.h, _ptr(queries), len(queries), int(variant), _ptr(idx))
    return rc, idx


def find(ctx, table, queries, variant):
    _lib, _l = _L()
    rc, idx = find_rc(ctx, table, queries, variant)
    _lib.check(rc)
    return idx


def table_view(ctx, table, offsets=False):
    """(hash bits, layout, bucket offsets uint64[2^bits + 1] or None)"""
    _lib, L = _L()
    bits, layout = C.c_int(-1), C.c_int(-1)
    _lib.check(L.shn_debug_table_view(ctx.h, table.h, C.byref(bits), C.byref(layout), None))
    off = None
    if offsets:
        off = np.zeros((1 << bits.value) + 1, dtype=np.uint64)
        _lib.check(L.shn_debug_table_view(ctx.h, table.h, None, None, off.ctypes.data))
    return bits.value, layout.value, off
