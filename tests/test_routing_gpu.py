"""GPU parity: partitions, k1-mer emit and read routing (rows a8-a11) vs the reference goldens."""
import collections
import numpy as np
import pytest
from golden_util import *

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(MANIFEST))
@pytest.mark.parametrize("probe_gpu", ["0", "1"])
def test_routing_matches_golden(ctx, name, probe_gpu, monkeypatch):
    """probe_gpu: k1mers2component by numpy on the host / by the device sort of csrc/probe_gpu.hip"""
    from shannon_amd import device, extension_correction as ec, kmers_for_component as kfc
    monkeypatch.setenv("SHN_PROBE_GPU", probe_gpu)
    g = load_case(name)
    K, paired = g["K"], g["paired"]
    psize = MANIFEST[name].get("partition_size", 500)
    inp = load_inputs(name)
    sets = [device.Reads.from_strings(ctx, r) for r in inp]
    ss = strand_specific(name)
    t = count_case(ctx, name, sets)
    res = ec.run_correction(ctx, t, 3, 75, psize)
    pv = [part_vectors(len(cl), psize) for cl, _ in res.big_components] or None
    for (cl, metis), gb, (p1, p2) in zip(res.big_components, g["big_components"], pv or []):
        assert kfc.weight_updated_graph(metis, p1, 5) == gb["metis_r2"]
    out = kfc.kmers_for_component(ctx, res, sets[0], sets[1] if paired else None, K, psize, part_vectors=pv, strand_specific=ss)
    assert list(out["new_components"]) == list(g["partitions"])
    store = kfc.ReadStore(inp[0], inp[1] if paired else None)
    files = read_files(name, inp)                          # strand-specific: routes are plain read indices into these
    for comp, gp in g["partitions"].items():
        idx = out["routes"][comp]
        assert len(idx) == gp["n_reads"]
        reads = [[files[0][int(d)] for d in idx]] if ss else [[store.mate1(int(d)) for d in idx]]
        if paired:
            reads.append([files[1][int(d)] for d in idx] if ss else [store.mate2(int(d)) for d in idx])
        assert digest(reads) == gp["reads_digest"]
        assert digest([[a, str(b)] for a, b in out["k1mers"][comp]]) == gp["k1mers_digest"]




def test_lazy_routes_equal_downloaded_routes(ctx):
    """kmers_for_component(lazy_routes=True) leaves the routes on the device (RouteView: length, forward-half count and
    slices on demand) -- the same routes as the full download."""
    from shannon_amd import device, synth, extension_correction as ec, kmers_for_component as kfc
    (r1, r2), _ = synth.make_dataset(12000, 12, seed=4)
    d1, d2 = device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2)
    t = device.count_k1mers(ctx, [d1, d2], 26, True)
    try:
        res = ec.run_correction(ctx, t, 3, 75, 500, want_allowed=False)
        full = kfc.kmers_for_component(ctx, res, d1, d2, 25, 500, want_rows=False)
        lazy = kfc.kmers_for_component(ctx, res, d1, d2, 25, 500, want_rows=False, lazy_routes=True)
        assert list(full["routes"]) == list(lazy["routes"]) and len(full["routes"]) > 0
        for name, r in full["routes"].items():
            v = lazy["routes"][name]
            assert len(v) == len(r) and v.count_below_split() == int(np.searchsorted(r, len(d1)))
            assert np.array_equal(np.asarray(v), r)
            a, b = len(r) // 3, 2 * len(r) // 3
            assert np.array_equal(v[a:b], r[a:b]) and np.array_equal(v[:5], r[:5]) and len(v[len(r):]) == 0
    finally:
        t.close(); d1.close(); d2.close()


def _python_routes(files, paired, ss, sets_of, k1):
    """(partition, doubled read index) pairs of get_rmers / get_comps (kmers_for_component.py:186-205) over the read files of
    shannon.py:396-424, sorted as shn_route_reads leaves them"""
    from oracle.partition import get_rmers
    comps = lambda read: set().union(*[sets_of[km] for km in get_rmers(read, k1) if km in sets_of])
    out = []
    for d in range(len(files[0])):
        parts = comps(files[0][d]) | (comps(files[1][d]) if paired else set())
        out.extend((p, d) for p in parts)
    return sorted(out)


@pytest.mark.parametrize("mode", ["se", "pe", "pe_ss"])
@pytest.mark.parametrize("L", ["K+1", "K+2", "2(K+1)", "2(K+1)+1", 64, 128, 150, 250])
def test_routing_kernel_equals_get_comps_at_read_lengths(ctx, L, mode):
    """shn_route_reads_mode against get_rmers / get_comps in Python at read lengths around the probe spacing (K+1) and the 32-base
    words, on a probe table of random sets (1-3 of 48 partitions) planted at probe windows of both strands -- and one pair (read 0,
    both mates on both strands) whose probes name 40 partitions between them: get_comps has no cap on the union."""
    from oracle.seqs import double_strand_paired, double_strand_single, strand_specific
    from oracle.partition import get_rmers
    from shannon_amd import device, _lib, kmers_for_component as kfc
    import ctypes as C
    K = 20
    k1 = K + 1
    L = {"K+1": k1, "K+2": k1 + 1, "2(K+1)": 2 * k1, "2(K+1)+1": 2 * k1 + 1}.get(L, L)
    paired, ss = mode != "se", mode == "pe_ss"
    rng = np.random.RandomState(L * 7 + len(mode))
    N, n_parts = 300, 48
    A = np.frombuffer(b"ACGT", np.uint8)
    m1 = rng.randint(0, 4, size=(N, L)).astype(np.uint8)
    m2 = rng.randint(0, 4, size=(N, L)).astype(np.uint8)
    r1 = [A[r].tobytes().decode() for r in m1]
    r2 = [A[r].tobytes().decode() for r in m2]
    if ss:
        files = strand_specific(r1, r2)
    else:
        files = list(double_strand_paired(r1, r2)) if paired else [double_strand_single(r1)]
    sets_of = {}
    for f in files:
        for read in f:
            if rng.rand() < 0.4:
                probes = get_rmers(read, k1)
                km = probes[rng.randint(len(probes))]
                sets_of.setdefault(km, set(rng.choice(n_parts, size=rng.randint(1, 4), replace=False).tolist()))
    # read 0: every probe of its first mate names a run of the 40 partitions 0..39 (runs overlap: duplicates between probes)
    wide = get_rmers(files[0][0], k1)
    step = -(-40 // len(wide))
    for i, km in enumerate(wide):
        lo = max(0, min(i * step, 40 - step - 1))
        sets_of[km] = set(range(lo, lo + step + 1)) | sets_of.get(km, set())
    keys = sorted(sets_of)
    sid = {}
    for km in keys:
        sid.setdefault(tuple(sorted(sets_of[km])), len(sid))
    sets = sorted(sid, key=sid.get)
    code = {c: i for i, c in enumerate("ACGT")}
    kv = np.array([int("".join("%d" % code[c] for c in km), 4) for km in keys], dtype=np.uint64)
    vals = np.array([sid[tuple(sorted(sets_of[km]))] + 1 for km in keys], dtype=np.uint32)
    set_off = np.zeros(len(sets) + 1, np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    set_mem = np.array([p for s in sets for p in s], dtype=np.uint32)
    want = _python_routes(files, paired, ss, sets_of, k1)
    assert max(collections.Counter(d for _p, d in want).values()) >= 40
    d1 = device.Reads.from_codes(ctx, m1)
    d2 = device.Reads.from_codes(ctx, m2) if paired else None
    probe = kfc.make_table(ctx, kv, vals, k1)
    h = C.c_void_p()
    try:
        _lib.check(_lib.lib().shn_route_reads_mode(ctx.h, d1.h, d2.h if paired else None, k1, probe.h, set_off.ctypes.data,
                                                   set_mem.ctypes.data, len(sets), 1 if ss else 0, C.byref(h)))
        routes = kfc.Routes(ctx, h)
        pid, ridx = routes.download()
        routes.close()
    finally:
        probe.close(); d1.close()
        if d2 is not None:
            d2.close()
    assert list(zip(pid.tolist(), ridx.tolist())) == want
