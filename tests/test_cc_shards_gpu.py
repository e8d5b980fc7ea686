"""Component labelling on owner shards (include/shannon_hip.h: shn_cc_*, the N-rank path without a replicated table).
The W ranks are played one after the other in ONE process (the exchange between them is done by hand on the tensors): the labels
must partition the k1-mers exactly as the connected components of the k1-mer graph do -- restated here in numpy + scipy from the
rule of the labelling kernel (extension_correction.py:202-245, 372-390: adjacent k1-mers, and k1-mers that share a K-mer at the
same end, both not low-complexity) -- and the component exchange must give every rank whole components."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


from cc_reference import reference_labels, same_partition


def play_ranks(ctx, table, W, K1, canonical, base0=0):
    """the whole exchange with W ranks in one process.  Returns per rank (keys of the shard in table order, their global labels,
    (keys, counts) received after the component exchange).  base0: added to every rank's base and to id_limit -- the global ids
    of a job whose earlier shards hold that many k1-mers (64-bit ids through shn_cc_answer, shn_cc_solve and shn_cc_labels)."""
    import torch
    from shannon_amd import device
    dev = torch.device("cuda", 0)
    n = len(table)
    dk = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    dc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    per = table.shard_by_minimizer(W, dk.data_ptr(), dc.data_ptr()).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(per)])
    shards, ccs = [], []
    for r in range(W):
        torch.cuda.synchronize()
        t = device.Table.from_pairs(ctx, dk[off[r]:].data_ptr(), dc[off[r]:].data_ptr(), int(per[r]), K1, canonical)
        assert len(t) == per[r]
        shards.append(t)
        ccs.append(device.ComponentShards(ctx, t, W, r))
    sizes = [len(t) for t in shards]
    base = [base0 + sum(sizes[:r]) for r in range(W)]
    # queries of every rank, grouped by destination
    sent = []
    for r in range(W):
        pq = ccs[r].query_counts().astype(np.int64)
        assert pq[:r + 1].sum() == 0                                 # only higher ranks are asked
        qk = torch.empty(max(int(pq.sum()), 1), dtype=torch.int64, device=dev)
        ql = torch.empty(max(int(pq.sum()), 1), dtype=torch.int32, device=dev)
        ccs[r].queries(qk.data_ptr(), ql.data_ptr())
        sent.append((pq, np.concatenate([[0], np.cumsum(pq)]), qk, ql))
    all_edges = []
    for d in range(W):
        rcl = [int(sent[s][0][d]) for s in range(W)]
        rk = torch.cat([sent[s][2][sent[s][1][d]:sent[s][1][d + 1]] for s in range(W)] + [torch.empty(0, dtype=torch.int64, device=dev)])
        rl = torch.cat([sent[s][3][sent[s][1][d]:sent[s][1][d + 1]] for s in range(W)] + [torch.empty(0, dtype=torch.int32, device=dev)])
        edges = torch.empty(2 * max(sum(rcl), 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ne = ccs[d].answer(rk.data_ptr(), rl.data_ptr(), rcl, base, edges.data_ptr())
        all_edges.append(edges[:2 * ne].clone())
    ge = torch.cat(all_edges)
    E = ge.numel() // 2
    nodes = torch.empty(2 * max(E, 1), dtype=torch.int64, device=dev)
    labels = torch.empty(2 * max(E, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    nn = device.ComponentShards.solve(ctx, ge.data_ptr(), E, base0 + sum(sizes) + 1, nodes.data_ptr(), labels.data_ptr())
    # the same from the edges in another order: the answer must not depend on it
    if E > 1:
        perm = torch.randperm(E, device=dev)
        ge2 = ge.view(E, 2)[perm].flip(1).contiguous().view(-1)
        nodes2, labels2 = torch.empty_like(nodes), torch.empty_like(labels)
        torch.cuda.synchronize()
        nn2 = device.ComponentShards.solve(ctx, ge2.data_ptr(), E, 0, nodes2.data_ptr(), labels2.data_ptr())
        assert nn2 == nn and torch.equal(nodes[:nn], nodes2[:nn]) and torch.equal(labels[:nn], labels2[:nn])
    out = []
    glabels = []
    for r in range(W):
        gl = torch.empty(max(sizes[r], 1), dtype=torch.int64, device=dev)
        ccs[r].labels(base[r], nodes.data_ptr(), labels.data_ptr(), nn, gl.data_ptr())
        glabels.append(gl)
    # owners: two of the components pinned to ranks by the caller, the rest by hash
    torch.cuda.synchronize()
    allg = torch.cat([glabels[r][:sizes[r]] for r in range(W)])
    u, c = torch.unique(allg, return_counts=True)
    top = u[torch.argsort(c, descending=True)[:2]].cpu().numpy()
    big = np.sort(top).astype(np.int64)
    big_owner = np.array([(W - 1 - i) % W for i in range(len(big))], dtype=np.uint8)
    dbig = torch.as_tensor(big if len(big) else np.zeros(1, np.int64), device=dev)
    dbo = torch.as_tensor(big_owner if len(big) else np.zeros(1, np.uint8), device=dev)
    recv = [[] for _ in range(W)]
    for r in range(W):
        owner = torch.empty(max(sizes[r], 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ccs[r].owners(glabels[r].data_ptr(), dbig.data_ptr(), dbo.data_ptr(), len(big), owner.data_ptr())
        sk = torch.empty(max(sizes[r], 1), dtype=torch.int64, device=dev)
        sc = torch.empty(max(sizes[r], 1), dtype=torch.int32, device=dev)
        send = ccs[r].shard(owner.data_ptr(), sk.data_ptr(), sc.data_ptr()).astype(np.int64)
        assert send.sum() == sizes[r]
        so = np.concatenate([[0], np.cumsum(send)])
        torch.cuda.synchronize()
        for d in range(W):
            recv[d].append((sk[so[d]:so[d + 1]].cpu().numpy().view(np.uint64), sc[so[d]:so[d + 1]].cpu().numpy().view(np.uint32)))
        ow = owner[:sizes[r]].cpu().numpy()
        gl = glabels[r][:sizes[r]].cpu().numpy()
        for i, b in enumerate(big):
            assert (ow[gl == b] == big_owner[i]).all()
        keys, _ = shards[r].download()
        out.append((keys, gl, ow))
    for r in range(W):
        ccs[r].close()
        shards[r].close()
    got = [(np.concatenate([k for k, _ in recv[d]]), np.concatenate([c for _, c in recv[d]])) for d in range(W)]
    return out, got


def _case(W, n_genes, seed, K, ss, base0=0):
    """(the cases without base0 keep the ids they had before base0 existed)"""
    name = "%d-%d-%d-%d-%s" % (W, n_genes, seed, K, ss)
    return pytest.param(W, n_genes, seed, K, ss, base0, id=name if not base0 else "%s-base0=%d" % (name, base0))


@pytest.mark.parametrize("W,n_genes,seed,K,ss,base0", [_case(2, 3, 11, 25, False), _case(3, 12, 4, 25, False), _case(4, 40, 8, 24, False),
                                                       _case(8, 12, 5, 31, False), _case(3, 12, 4, 25, True), _case(5, 1, 3, 20, False),
                                                       _case(2, 3, 11, 25, False, 2 ** 32 - 5), _case(2, 3, 11, 25, False, 2 ** 40)])
def test_labels_of_the_shards_are_the_components(W, n_genes, seed, K, ss, base0):
    from shannon_amd import device, synth
    (q1, q2), _ = synth.make_dataset(12000, n_genes, seed=seed)
    ctx = device.Context(0)
    d1, d2 = device.Reads.from_codes(ctx, q1), device.Reads.from_codes(ctx, q2)
    try:
        if ss:
            table = device.count_k1mers_strand_specific(ctx, d1, d2, K + 1)
        else:
            table = device.count_k1mers(ctx, [d1, d2], K + 1, True)
        canonical = table.canonical
        assert canonical == (not ss)
        tk, tc = table.download()
        out, got = play_ranks(ctx, table, W, K + 1, canonical, base0)
        keys = np.concatenate([o[0] for o in out])
        gl = np.concatenate([o[1] for o in out])
        ow = np.concatenate([o[2] for o in out])
        if base0:                                                    # every label is a global id of this job: ids at and above 2^32
            assert int(gl.min()) >= base0 and int(gl.max()) < base0 + len(tk) and base0 + len(tk) > 2 ** 32
        assert len(keys) == len(tk) and np.array_equal(np.sort(keys), np.sort(tk))            # the shards partition the table
        ref = reference_labels(keys, K + 1, canonical)
        assert len(np.unique(ref)) > 1 or n_genes == 1               # (one gene at K = 20: its errors hang on it as siblings -- one component)
        assert same_partition(gl, ref)
        # a component lives on one rank after the exchange, with every k1-mer and count of it
        pairs = np.unique(np.stack([gl, ow.astype(np.int64)], axis=1), axis=0)
        assert len(pairs) == len(np.unique(gl))
        want = dict(zip(tk.tolist(), tc.tolist()))
        seen = 0
        for d, (k, c) in enumerate(got):
            assert np.array_equal(np.sort(k), np.sort(keys[ow == d]))
            assert all(want[a] == b for a, b in zip(k.tolist(), c.tolist()))
            seen += len(k)
        assert seen == len(tk)
        table.close()
    finally:
        d1.close()
        d2.close()
        ctx.close()


@pytest.mark.parametrize("ss", [False, True])
def test_labels_are_the_same_on_every_repeat(ss):
    """40 repeats of the labelling of one table: the same label for every k1-mer every time, and the reference's partition.  (Round 5:
    the kernel that gives every k1-mer its root compressed paths while others stored their roots -- a k1-mer could keep an ancestor
    for a label; with every edge asked from one end the trees were deep enough for 70 % of the runs to show it.)"""
    from shannon_amd import device, synth
    (q1, q2), _ = synth.make_dataset(12000, 12, seed=4)
    ctx = device.Context(0)
    d1, d2 = device.Reads.from_codes(ctx, q1), device.Reads.from_codes(ctx, q2)
    try:
        table = device.count_k1mers_strand_specific(ctx, d1, d2, 26) if ss else device.count_k1mers(ctx, [d1, d2], 26, True)
        first = None
        for rep in range(40):
            out, _got = play_ranks(ctx, table, 2, 26, table.canonical)
            keys = np.concatenate([o[0] for o in out])
            gl = np.concatenate([o[1] for o in out])
            if first is None:
                first = (keys, gl)
                assert same_partition(gl, reference_labels(keys, 26, table.canonical))
            else:
                assert np.array_equal(keys, first[0]) and np.array_equal(gl, first[1]), "repeat %d: %d labels differ" % (rep, int((gl != first[1]).sum()))
        table.close()
    finally:
        d1.close()
        d2.close()
        ctx.close()


def test_tiny_inputs_and_empty_shards():
    """a handful of k1-mers over 16 ranks: shards without a k1-mer, ranks that receive no component, no edge between shards at all"""
    import torch
    from shannon_amd import device, synth
    (q1, q2), _ = synth.make_dataset(40, 1, seed=9)
    ctx = device.Context(0)
    d1 = device.Reads.from_codes(ctx, q1[:3])
    try:
        table = device.count_k1mers(ctx, [d1], 26, True)
        tk, tc = table.download()
        assert 0 < len(tk) < 400
        out, got = play_ranks(ctx, table, 16, 26, True)
        assert any(len(o[0]) == 0 for o in out)
        keys = np.concatenate([o[0] for o in out])
        gl = np.concatenate([o[1] for o in out])
        assert np.array_equal(np.sort(keys), np.sort(tk)) and same_partition(gl, reference_labels(keys, 26, True))
        assert sum(len(k) for k, _ in got) == len(tk)
        table.close()
        # one k1-mer, two ranks: nothing to ask, nothing to solve
        one = torch.as_tensor(np.array([0x1B2C3D4E5F60 & ((1 << 52) - 1)], dtype=np.int64), device="cuda")
        cnt = torch.ones(1, dtype=torch.int32, device="cuda")
        t1 = device.Table.from_pairs(ctx, one.data_ptr(), cnt.data_ptr(), 1, 26, True)
        out, got = play_ranks(ctx, t1, 2, 26, True)
        assert sum(len(o[0]) for o in out) == 1 and sum(len(k) for k, _ in got) == 1
        t1.close()
    finally:
        d1.close()
        ctx.close()


def test_shard_rule_mirror():
    """the host mirror of the owner rule (exchange.owner_of_minimizer) against the device's shards"""
    import torch
    from shannon_amd import device, synth, exchange
    (q1, q2), _ = synth.make_dataset(6000, 4, seed=2)
    ctx = device.Context(0)
    d1 = device.Reads.from_codes(ctx, q1)
    try:
        for K1, both in ((26, True), (21, True), (32, True), (26, False)):
            table = device.count_k1mers(ctx, [d1], K1, both)
            n = len(table)
            for W in (2, 5, 8):
                dk = torch.empty(n, dtype=torch.int64, device="cuda")
                dc = torch.empty(n, dtype=torch.int32, device="cuda")
                per = table.shard_by_minimizer(W, dk.data_ptr(), dc.data_ptr()).astype(np.int64)
                keys = dk.cpu().numpy().view(np.uint64)
                own = exchange.owner_of_minimizer(keys, K1, table.canonical, W)
                assert np.array_equal(own, np.repeat(np.arange(W), per))
            table.close()
    finally:
        d1.close()
        ctx.close()
