"""The ways the native graph stage takes in the reads of ONE partition (csrc/mbgraph_reads.h: choose_intake and the intake forms
of PartitionReads), called directly: every entry point and every form must leave the graph that shn_mbgraph_run makes without a
GPU, array for array of shn_graph_export.  The partitions are built by hand so that the intake, not the graph surgery, is what
can differ: a read that occurs many times, a read and its reverse complement both routed, a read whose last occurrence has
another role (and, where the pairs are free text, another mate) than its first -- in a partition where that role and that mate
decide whether find_mate_pairs finds a path, so the export shows them --, and a small partition whose routed reads exceed the
read cap of ten times its K-mers plus one."""
import numpy as np
import pytest

K, L, N_SAMPLED, N_BEHIND_CAP = 24, 64, 1400, 200
SWITCHES = ("SHN_GRAPH_RESIDENT_READS", "SHN_GRAPH_DEVICE_DEDUP", "SHN_GRAPH_LAZY_TEXT", "SHN_GRAPH_DEV_ATTRS", "SHN_GRAPH_BULK_MIN")
_CASE = {}


def _text(codes):
    return np.frombuffer(b"ACGT", np.uint8)[codes].tobytes().decode()


def _n_kmers(contigs):
    return len({c[i:i + K] for c in contigs for i in range(len(c) - K + 1)})


def _cut_at_shared_k1mers(texts):
    """contigs the way the extension leaves them: every (K+1)-mer of the transcripts once (isoforms share exons; a k1-mer listed
    twice would be an edge made twice)"""
    seen, out = set(), []
    for t in texts:
        start = None
        for i in range(len(t) - K):
            fresh = t[i:i + K + 1] not in seen
            seen.add(t[i:i + K + 1])
            if fresh and start is None:
                start = i
            if not fresh and start is not None:
                out.append(t[start:i + K])
                start = None
        if start is not None:
            out.append(t[start:])
    return out


def _hairpin():
    """contigs of partition 2 and 64-base reads inside its nodes: RA in A, MC = RC(RA) in rc(A), MB in B, MX in the branch off A"""
    rng = np.random.RandomState(23)
    A, B, X, Y = (rng.randint(0, 4, 80).astype(np.uint8) for _ in range(4))
    rcA = 3 - A[::-1]
    X[0] = (B[0] + 1) & 3                            # (the branches share a K-mer with the chain, no k1-mer)
    Y[-1] = (B[-1] + 1) & 3
    contigs = [_text(np.concatenate([A, B, rcA])), _text(np.concatenate([A[-K:], X])), _text(np.concatenate([Y, rcA[:K]]))]
    return dict(contigs=contigs, RA=A[8:72].copy(), MC=rcA[8:72].copy(), MB=B[8:72].copy(), MX=X[8:72].copy())


def _free_pairs(order):
    """text pairs on partition 2, the last three in the given order: q = (MX, RA): RA a second mate; x = (RA, MX): RA's mate in the
    branch next to A (adjacent: no path asked for); c = (RA, MC): the mate in rc(A), the pair that finds the path"""
    from shannon_amd import mbgraph_native as mn
    hp = _hairpin()
    pairs = [(hp["MB"], hp["MX"])] * 40 + [{"q": (hp["MX"], hp["RA"]), "x": (hp["RA"], hp["MX"]), "c": (hp["RA"], hp["MC"])}[o] for o in order]
    return mn._pack_reads([_text(a) for a, _b in pairs]) + mn._pack_reads([_text(b) for _a, b in pairs])


def _run_free(c, order, **kw):
    from shannon_amd import mbgraph_native as mn
    rb = c["rows"][2]
    h = mn.run_partition_handle(rb, len(rb) // (K + 1), K, *_free_pairs(order), **kw)
    try:
        return mn.export_arrays(h.h)
    finally:
        h.close()


def _case():
    """contigs, read matrices and routed lists of the two partitions (made once, never changed)"""
    if _CASE:
        return _CASE
    from shannon_amd import synth, kmers_for_component as kfc
    iso, _ = synth.make_transcriptome(4, seed=7)
    r1, r2 = synth.sample_pairs(iso, N_SAMPLED, 7, read_len=L, frag_len=200, err=0.002)
    X = r1[5].copy()
    r1[10:50] = X                                   # a read that occurs many times,
    r2[7] = X                                       # ... and (paired) comes last as a SECOND mate: slot N + 7 is (RC(X), X)
    rng = np.random.RandomState(11)
    P, Q1, Q2 = (rng.randint(0, 4, 70).astype(np.uint8) for _ in range(3))
    Q2[0] = (Q1[0] + 1) & 3
    small = [_text(np.concatenate([P, Q1])), _text(np.concatenate([P[-K:], Q2]))]       # a fork: one shared K-mer, no shared k1-mer
    cap = 10 * _n_kmers(small) + 1
    JA, JB = np.concatenate([P[-32:], Q1[:32]]), np.concatenate([P[-32:], Q2[:32]])       # reads across the fork, one per branch
    # partition 2, the mates: A -> B -> rc(A) with a branch off A and a branch into rc(A), so that the three stay three nodes.  A
    # first mate inside A whose mate lies inside rc(A) gives find_mate_pairs its one path (A, B, rc(A)); the same read as a second
    # mate, or with a mate inside the branch, gives none.
    hp = _hairpin()
    RA, MC = hp["RA"], hp["MC"]                     # MC = RC(RA)
    mates = np.stack([MC, RA] + [hp["MB"]] * 40)    # rows: (RC(RA), RA) first -- RA a second mate --, then (RA, RC(RA)): the last one wins
    m1 = np.ascontiguousarray(np.concatenate([r1, np.tile(JA, (cap, 1)), np.tile(JB, (N_BEHIND_CAP, 1)), mates]))
    m2 = np.ascontiguousarray(np.concatenate([r2, rng.randint(0, 4, (cap + N_BEHIND_CAP + len(mates), L)).astype(np.uint8)]))
    n = len(m1)
    # partition 0: every sampled read on both strands (single-end: R[d] and RC(R[d]); paired: (R1[d], RC(R1[d])) and (RC(R2[d]), R2[d]))
    # partition 1: `cap` reads across one branch of its fork, then reads across the other, which the cap must leave out
    didx = [np.concatenate([np.arange(N_SAMPLED), n + np.arange(N_SAMPLED)]).astype(np.uint32), (N_SAMPLED + np.arange(cap + N_BEHIND_CAP)).astype(np.uint32),
            (N_SAMPLED + cap + N_BEHIND_CAP + np.arange(len(mates))).astype(np.uint32)]
    contigs = [_cut_at_shared_k1mers([_text(t) for t in iso]), small, hp["contigs"]]
    rows = [kfc._rows_bytes(cl, K + 1) for cl in contigs]
    _CASE.update(m1=m1, m2=m2, didx=didx, contigs=contigs, rows=rows, cap=cap)
    return _CASE


def _gathered(c, paired, didx):
    """the routed reads as gathered code rows + strand flags, the way the pipeline hands them to shn_mbgraph_run{,_unitigs,_resident}"""
    from shannon_amd import kmers_for_component as kfc
    store = kfc.ReadStore(c["m1"], c["m2"] if paired else None)
    b1, o1, rc1, enc = store.gather_codes(didx, 1)
    b1, o1 = b1[:len(didx) * L].copy(), o1.copy()
    return dict(r1_buf=b1, r1_off=o1, r2_buf=b1 if paired else None, r2_off=o1 if paired else None, enc=enc, rc1=rc1,
                rc2=(1 - rc1).astype(np.uint8) if paired else None)


def _run_cpu(c, paired, part, didx=None):
    from shannon_amd import mbgraph_native as mn
    g = _gathered(c, paired, c["didx"][part] if didx is None else didx)
    rb = c["rows"][part]
    h = mn.run_partition_handle(rb, len(rb) // (K + 1), K, g.pop("r1_buf"), g.pop("r1_off"), **g)
    try:
        return mn.export_arrays(h.h)
    finally:
        h.close()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("paired", [False, True])
def test_the_read_cap_trims_and_the_host_forms_agree(paired, monkeypatch):
    """without a GPU: the small partition's graph is the graph of its first 10 * K-mers + 1 routed reads (the reads behind the cap
    cross the other branch of the fork: routed first they do change it), and the parallel duplicate search numbers the reads of
    both partitions as the interner does"""
    c = _case()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    d1 = c["didx"][1]
    assert len(d1) > c["cap"]
    capped = _run_cpu(c, paired, 1)
    assert _same(capped, _run_cpu(c, paired, 1, d1[:c["cap"]]))
    assert not _same(capped, _run_cpu(c, paired, 1, d1[::-1].copy()))
    assert len(capped["e_cc"]) > 0
    big = _run_cpu(c, paired, 0)
    assert len(big["n_cc"]) > 10 and big["info"][5] > 0                  # components with known paths: the reads were used
    monkeypatch.setenv("SHN_GRAPH_BULK_MIN", "64")
    assert _same(big, _run_cpu(c, paired, 0)) and _same(capped, _run_cpu(c, paired, 1))


@pytest.mark.parametrize("bulk_min", [None, "64"])
def test_the_mate_and_role_of_the_last_occurrence_decide_the_mate_path(bulk_min, monkeypatch):
    """without a GPU, interner (None) and parallel search ("64"): in partition 2 the one mate path exists only while RA's LAST
    occurrence is as a first mate whose mate lies in rc(A).  Resident rows (the mate of a read is its reverse complement: only the
    role can change) and free text pairs (mate and role): the routed order as given finds the path, the same occurrences in another
    order do not."""
    c = _case()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if bulk_min:
        monkeypatch.setenv("SHN_GRAPH_BULK_MIN", bulk_min)
    d2 = c["didx"][2]
    rows = _run_cpu(c, True, 2)
    assert rows["info"][6] == 1 and len(rows["p_ids"]) >= 3
    flipped = _run_cpu(c, True, 2, d2[::-1].copy())                    # RA's last occurrence is now the second mate of (RC(RA), RA)
    assert flipped["info"][6] == 0 and not _same(rows, flipped)
    assert _run_cpu(c, False, 2)["info"][6] == 0                       # (single-end: no mates at all)
    free = _run_free(c, "qxc")
    assert free["info"][6] == 1 and len(free["p_ids"]) >= 3
    for order in ("qcx", "xcq"):                                       # the last mate is the one in the branch / the last role is second mate
        other = _run_free(c, order)
        assert other["info"][6] == 0 and not _same(free, other), order


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_every_entry_point_and_intake_form_makes_the_graph_of_the_host_run(ctx, paired, monkeypatch):
    from shannon_amd import device, mbgraph_native as mn, kmers_for_component as kfc
    c = _case()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    want = [_run_cpu(c, paired, part) for part in (0, 1, 2)]
    assert want[2]["info"][6] == (1 if paired else 0)                   # the mate path of partition 2: the last occurrence's role
    d1 = device.Reads.from_codes(ctx, c["m1"])
    d2 = device.Reads.from_codes(ctx, c["m2"]) if paired else None
    h1, h2 = c["m1"], (c["m2"] if paired else None)
    ug = mn.Unitigs(ctx, c["contigs"], K)
    routes = kfc.Routes.from_arrays(ctx, np.repeat(np.arange(3, dtype=np.uint32), [len(x) for x in c["didx"]]), np.concatenate(c["didx"]))
    lo = np.concatenate([[0], np.cumsum([len(x) for x in c["didx"]])]).tolist()
    assert [ug.n_kmers(p) for p in (0, 1, 2)] == [_n_kmers(cl) for cl in c["contigs"]]

    def by_routes(part):                    # shn_mbgraph_run_routes: the list known by its place on the device only
        return mn.run_partition_rows(ctx, ug, part, d1, d2, h1, h2, len(c["didx"][part]), c["rows"][part], len(c["rows"][part]) // (K + 1), routes=(routes, lo[part]))

    def by_rows(part):                      # shn_mbgraph_run_rows
        return mn.run_partition_rows(ctx, ug, part, d1, d2, h1, h2, c["didx"][part], c["rows"][part], len(c["rows"][part]) // (K + 1))

    def gathered(part, resident, unitigs=True, on_gpu=True):
        g = _gathered(c, paired, c["didx"][part])
        rb = c["rows"][part]
        return mn.run_partition_handle(rb, len(rb) // (K + 1), K, g.pop("r1_buf"), g.pop("r1_off"), ctx=ctx if on_gpu else None, unitigs=ug if unitigs else None,
                                       part=part, resident=(d1, d2, c["didx"][part]) if resident else None, **g)

    forms = [
        ("routes", {}, by_routes),                                                                  # device attributes, lazy text
        ("routes, attributes in host arrays", {"SHN_GRAPH_DEV_ATTRS": "0"}, by_routes),             # device dedup, lazy text
        ("rows", {}, by_rows),
        ("rows, text up front", {"SHN_GRAPH_LAZY_TEXT": "0"}, by_rows),                             # device dedup, text from the matrices
        ("resident", {}, lambda p: gathered(p, True)),                                              # interner, rows noted for the gather
        ("resident, device dedup", {"SHN_GRAPH_BULK_MIN": "64"}, lambda p: gathered(p, True)),      # device dedup, text from the gathered rows
        ("resident, parallel search", {"SHN_GRAPH_BULK_MIN": "64", "SHN_GRAPH_DEVICE_DEDUP": "0"}, lambda p: gathered(p, True)),
        ("resident, text uploaded", {"SHN_GRAPH_RESIDENT_READS": "0"}, lambda p: gathered(p, True)),
        ("unitigs", {}, lambda p: gathered(p, False)),
        ("unitigs, parallel search", {"SHN_GRAPH_BULK_MIN": "64"}, lambda p: gathered(p, False)),
        ("unitigs, parallel search, no device dedup", {"SHN_GRAPH_BULK_MIN": "64", "SHN_GRAPH_DEVICE_DEDUP": "0"}, lambda p: gathered(p, False)),
        ("k1-mer rows on the GPU context", {}, lambda p: gathered(p, False, unitigs=False)),
    ]

    def export(run, part):
        h = run(part)
        try:
            return mn.export_arrays(h.h)
        finally:
            h.close()

    try:
        for name, env, run in forms:
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            for part in (0, 1, 2):
                got = export(run, part)
                for k in want[part]:
                    assert np.array_equal(got[k], want[part][k]), (name, "paired" if paired else "single-end", part, k)
        # a lease that served a larger call before a smaller one, and a smaller one before a larger: large, small, large on this
        # one thread, for a form of each kind of buffer (lazy text; arena; decode text + arena)
        for name, env, run in (forms[0], forms[5], forms[6], ("no GPU", {}, lambda p: gathered(p, False, unitigs=False, on_gpu=False))):
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            for part in (0, 1, 0):
                got = export(run, part)
                assert all(np.array_equal(got[k], want[part][k]) for k in got), (name, part)
    finally:
        routes.close(); ug.close(); d1.close()
        if d2 is not None:
            d2.close()


@pytest.mark.gpu
def test_free_pairs_keep_the_mate_and_role_of_the_last_occurrence(ctx, monkeypatch):
    """pairs given as text (no resident rows: the mates are not each other's reverse complement) on partition 2, where the mate
    and the role of RA's last occurrence make the mate path: interner and parallel search on a GPU context, with k1-mer rows and
    with GPU unitigs, against the run without a GPU"""
    from shannon_amd import mbgraph_native as mn
    c = _case()
    monkeypatch.delenv("SHN_GRAPH_BULK_MIN", raising=False)
    want = _run_free(c, "qxc")
    assert want["info"][6] == 1
    ug = mn.Unitigs(ctx, c["contigs"], K)
    try:
        for bulk in (None, "64"):
            monkeypatch.delenv("SHN_GRAPH_BULK_MIN", raising=False)
            if bulk:
                monkeypatch.setenv("SHN_GRAPH_BULK_MIN", bulk)
            for kw in ({"ctx": ctx}, {"ctx": ctx, "unitigs": ug, "part": 2}):
                assert _same(want, _run_free(c, "qxc", **kw)), (bulk, sorted(kw))
    finally:
        ug.close()
