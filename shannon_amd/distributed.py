"""Multi-GPU hot path on one node: one process per GPU, torch.distributed ("nccl" = RCCL over xGMI).  DESIGN.md section 6.

No rank holds the job: not its reads (every rank ingests its share of the files' BYTES: ingest_rank_slice), not its k1-mer table.
  1. every rank counts its slice of the reads; the (key, count) pairs go to the rank that owns the k1-mer's MINIMIZER in ONE
     all-to-all(v) -- the k-mer bucket exchange -- and the owner reduces by key (a k1-mer and its neighbours share their
     minimizer 7 times out of 8: most edges of the k1-mer graph stay inside a shard);
  2. the connected components of the k1-mer graph are labelled ON the owner shards (local union-find; the keys a higher rank owns
     are asked there in one all-to-all; the edges between local components are all-gathered and solved on every rank alike), and
     whole components travel to the rank that walks them (one all-to-all): a table of its own per rank, the unsharded greedy
     extension on it (SHN_OWNER_LABELS=0: the replicated table of rounds 2-4, kept for comparison);
  3. the candidates of all ranks meet in the walk order of the reference (one all-gather of arrays: seed weights and keys, offsets,
     text), the contig stage runs on them, every rank routes ITS reads against the accepted contigs' probe table; partitions are
     dealt to ranks by the reads their graphs consume (deal_partitions) and those reads -- the first 10 * nodes + 1 of the global
     strand-doubled order (multibridging.py:26-30) -- travel to the owner in one all-to-all of bytes;
  4. owners build the multibridged graphs and run the sparse flow of their partitions; rank 0 gathers the FASTA and merges.
The result equals the single-GPU pipeline on the concatenated reads (tests/test_distributed_*.py, test_nrank_midsize_gpu.py).

`ops` abstracts the per-rank compute (GpuOps: HIP kernels through the C ABI; the CPU tests plug an oracle-backed implementation
to exercise the collective choreography with gloo).
"""
from collections.abc import Mapping
from contextlib import contextmanager
from types import SimpleNamespace
import os
import numpy as np
import torch
import torch.distributed as dist
from . import exchange, graph_intake, sparse_flow, post, _lib


def _all_gather_var(t, group=None, name="table all-gather (owned k1-mer shards)"):
    """all-gather of 1-D tensors of different lengths (padded to the max)."""
    import time
    t_begin = time.time()
    out, ns = _all_gather_var_(t, group)
    if dist.get_world_size(group) > 1:
        if out.device.type == "cuda":
            torch.cuda.synchronize()
        me = dist.get_rank(group)
        es = t.element_size()
        exchange.note(name, es * ns[me] * (len(ns) - 1), es * (sum(ns) - ns[me]), time.time() - t_begin)
    return out, ns


def _all_gather_var_(t, group=None):
    W = dist.get_world_size(group)
    cdev = exchange.coll_device(t.device, group)
    n = torch.tensor([t.numel()], dtype=torch.int64, device=cdev)
    ns = [torch.zeros_like(n) for _ in range(W)]
    dist.all_gather(ns, n, group=group)
    ns = [int(x.item()) for x in ns]
    if W == 1:
        return t, ns
    # in rounds of at most exchange.chunk_elems() elements per rank (see there), each round padded to its longest piece
    C = exchange.chunk_elems()
    out = torch.empty(sum(ns), dtype=t.dtype, device=cdev)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    src = t.to(cdev)
    for j in range((max(ns + [1]) + C - 1) // C):
        lens = [int(min(max(k - j * C, 0), C)) for k in ns]
        mx = max(lens + [1])
        pad = torch.zeros(mx, dtype=t.dtype, device=cdev)
        mine = lens[dist.get_rank(group)]
        pad[:mine] = src[j * C: j * C + mine]
        outs = [torch.empty_like(pad) for _ in range(W)]
        dist.all_gather(outs, pad, group=group)
        for r in range(W):
            if lens[r]:
                out[int(off[r]) + j * C: int(off[r]) + j * C + lens[r]] = outs[r][:lens[r]]
    return out.to(t.device), ns


def ingest_rank_slice(paths, rank, world, group, device, ctx=None, stats=None, ragged=False, text_spans=None):
    """The N-rank CLI's reads by BYTES of the files (round 6; the reference streams its read files once, 10 M reads at a time:
    kmers_for_component.py:322-403).  Every rank counts the records that start in its share of each file's bytes
    (shn_text_records_in_range), the counts of all ranks say which record every share starts with, and the records
    [n r / W, n (r + 1) / W) of this rank -- a few records into some share -- go through shn_reads_ingest as one stretch of text.
    Host memory and parsing per rank: its share of the text (memory-mapped) + its slice's code matrix, not the whole job's.
    Returns (code matrices of this rank's slice, one per file; n records of the job) or None when a file cannot be shared out this
    way (.gz: no random access; reads of different lengths; multi-line FASTA) and the caller reads whole files as before.
    ragged=True: reads of different lengths are shared out too.  A rank whose stretch of text holds them keeps the
    device.RaggedCodes it ingests as; the ranks tell each other (the flags all-gather), and where some rank's slice of a file is
    ragged -- or two ranks hold matrices of two lengths -- every rank's slice of that file becomes RaggedCodes (a matrix is codes
    + arange * L already): one kind of store per file on all ranks.
    stats (dict): bytes this rank looked at / holds.
    text_spans (list): gets one (a, b) per file appended -- the bytes [a, b) of the file that hold this rank's records (a == b: it
    holds none); a caller that needs more of the records than their bases (the quality lines: shannon_amd.correct) reads them there."""
    import ctypes as C
    from . import _lib, device as dev_mod
    if any(p.endswith(".gz") for p in paths):
        return None
    L_ = _lib.lib()
    mats, n_job = [], None
    scanned = held = 0
    for path in paths:
        size = os.path.getsize(path)
        text = np.memmap(path, dtype=np.uint8, mode="r") if size else np.zeros(0, np.uint8)
        B = int(len(text))
        lo_b, hi_b = rank * B // world, (rank + 1) * B // world
        first, cnt, n_idx = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ptr = text.ctypes.data if B else None
        ok = 1
        # (with the count: the offset of every 1,024th record of the share -- from the shares' sparse indices any record of the file is
        # at most 1,023 records away, whoever's share it starts in; shares below 4 MB index more densely, one record per 4 KB of the
        # share, so that the walk to a slice's first record stays a few per cent of the share: the same on every rank)
        STRIDE = int(max(16, min(1024, (B // max(world, 1)) >> 12)))
        idx_buf = np.zeros(max(1, (hi_b - lo_b) // (2 * STRIDE) + 2), dtype=np.uint64)         # (a record is at least 2 bytes)
        try:
            _lib.check(L_.shn_text_records_in_range(ptr, B, lo_b, hi_b, 0, C.byref(first), C.byref(cnt), STRIDE, idx_buf.ctypes.data, len(idx_buf),
                                                    C.byref(n_idx)))
        except _lib.ShannonError:
            ok = 0
        scanned += hi_b - lo_b
        sparse = [p_[0] for p_ in exchange.all_gather_arrays((idx_buf[:n_idx.value],), device, group, "ingest: sparse record index of the shares")]
        mine = torch.tensor([first.value, cnt.value, ok], dtype=torch.int64, device=device)
        parts = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        tab = np.stack([x.cpu().numpy() for x in parts])                      # [W, 3]: first record start, records, ok
        if not tab[:, 2].all():
            return None
        firsts, cnts = tab[:, 0], tab[:, 1]
        prefix = np.concatenate([[0], np.cumsum(cnts)])
        n = int(prefix[-1])
        if n_job is None:
            n_job = n
        elif n != n_job:
            raise _lib.ShannonError("--left and --right hold different numbers of reads (%d, %d)" % (n_job, n))

        def locate(idx):
            # byte offset at which record `idx` of the file starts
            nonlocal scanned
            if idx >= n:
                return B
            k = int(np.searchsorted(prefix, idx, side="right")) - 1
            j, rest = divmod(int(idx - prefix[k]), STRIDE)
            start = int(sparse[k][j])
            off = C.c_uint64()
            _lib.check(L_.shn_text_skip_records(ptr, B, start, rest, 0, C.byref(off)))
            scanned += int(off.value) - start
            return int(off.value)
        rlo, rhi = rank * n // world, (rank + 1) * n // world
        a, b = locate(rlo), locate(rhi)
        if text_spans is not None:
            text_spans.append((a, b) if rhi > rlo else (a, a))
        if rhi == rlo:                                        # (more ranks than records: this rank holds none)
            codes = np.zeros((0, 0), np.uint8)
        else:
            try:
                _d, codes = dev_mod.Reads.ingest(None, text[a:b])
            except _lib.ShannonError as ex:
                if "unsupported" not in str(ex):
                    raise
                codes = None
        is_ragged = isinstance(codes, dev_mod.RaggedCodes)
        fine = codes is not None and (ragged or not is_ragged) and len(codes) == rhi - rlo
        flag = torch.tensor([1 if fine else 0, codes.shape[1] if fine and not is_ragged and len(codes) else 0, 1 if fine and is_ragged else 0],
                            dtype=torch.int64, device=device)
        flags = [torch.zeros_like(flag) for _ in range(world)]
        dist.all_gather(flags, flag, group=group)
        ft = np.stack([x.cpu().numpy() for x in flags])
        lens = set(int(v) for v in ft[:, 1] if v)
        some_ragged = bool(ft[:, 2].any()) or len(lens) > 1
        if not ft[:, 0].all() or (some_ragged and not ragged):
            return None
        if some_ragged:
            if not is_ragged:
                codes = dev_mod.RaggedCodes.from_matrix(codes) if len(codes) else dev_mod.RaggedCodes(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        elif len(codes) == 0 and lens:                                        # (a rank without records still holds a matrix of the job's read length)
            codes = np.zeros((0, lens.pop()), np.uint8)
        scanned += b - a
        held += (b - a) + (codes.total_bases if some_ragged else codes.size)
        mats.append(codes if some_ragged else np.ascontiguousarray(codes))
        del text
    if stats is not None:
        stats.update({"bytes_scanned": int(scanned), "bytes_held": int(held), "file_bytes": int(sum(os.path.getsize(p) for p in paths)), "records": int(n_job or 0)})
    return mats, int(n_job or 0)


def deal_partitions(load, W):
    """owner[i] of partition i: partitions in order of decreasing load, each to the rank with the least load so far (ties: the
    lowest rank, the lowest partition index first) -- identical on every rank."""
    load = np.asarray(load, dtype=np.int64)
    owner = np.zeros(len(load), dtype=np.int64)
    acc = np.zeros(W, dtype=np.int64)
    for i in np.argsort(-load, kind="stable").tolist():
        r = int(np.argmin(acc))
        owner[i] = r
        acc[r] += load[i]
    return owner


class Clock(object):
    """One rank's stage times and its compute lock.  `with clock.stage(name)`: a stretch of this rank's own compute -- the lock is
    held, the seconds go to timings[name].  `with clock.collective(name)`, inside a stage or between two: time spent with the other
    ranks -- the enclosing stage's stopwatch stops and the lock is free until the block is left, by an exception too; the seconds
    go to timings[name] ("x:...").  So the lock is held exactly while a stage is open and no collective is.
    lock (development aid; acquire() / release()): with several ranks on ONE GPU it serialises their compute, so the per-stage
    times are those of a rank that has a GPU to itself.  timings: the dict itself, for callees that keep sub-stage keys in it
    (run_correction, kmers_for_component).  Clock() alone holds no lock and measures into a dict nobody reads."""

    def __init__(self, timings=None, lock=None, now=None):
        import time
        self.timings = timings if timings is not None else {}
        self._lock, self._now, self._open = lock, now or time.time, None      # _open: [name, start] of the open stage

    def _add(self, name, since):
        self.timings[name] = self.timings.get(name, 0.0) + self._now() - since

    def _switch(self, name):
        """closes the open stage, if there is one (its seconds booked, the lock given back), and opens stage `name`, unless None"""
        if self._open is not None:
            self._add(*self._open)
            self._open = None
            if self._lock is not None:
                self._lock.release()
        if name is not None:
            if self._lock is not None:
                self._lock.acquire()
            self._open = [name, self._now()]

    @contextmanager
    def stage(self, name):
        if self._open is not None:
            raise RuntimeError("Clock: stage %r opened inside stage %r" % (name, self._open[0]))
        self._switch(name)
        try:
            yield
        finally:
            self._switch(None)

    @contextmanager
    def collective(self, name):
        around = self._open[0] if self._open is not None else None
        self._switch(None)
        since = self._now()
        try:
            yield
        finally:
            self._add(name, since)
            self._switch(around)


class RankOps(object):
    """What assemble_distributed asks of a rank's compute (GpuOps below: HIP kernels through the C ABI; the CPU tests: the oracle).
    Required: paired; n_reads(); local_pairs(W, by_minimizer=False) -> (keys, counts, per rank); reduce_pairs(keys, counts);
    table_from_pairs(keys, counts); extension(table, partition_size, group, presharded=None: or the job's k1-mers, `table` holding
    this rank's whole components); route(res, K, partition_size, part_vectors) -> {"new_components", "routes", ...};
    n_nodes(part, name, K); collect(doubled indices) -> a piece of reads; graph(part, name, pieces, K, paired) -> (singles,
    components); sparse_flow(components, ids, seed).  Set by assemble_distributed: clock, strand_specific, min_weight, min_length,
    kmer_hard_cutoff.  Two things are looked for, not declared: their absence refuses foreign ops before any collective --
    supports_strand_specific (true: -s is implemented) and filter_cover / filter_count (--filter_FP: see filter_owned_texts)."""
    owner_labelling = False       # capability: owned_table(keys, counts), component_table(owned, group) -> (table, k1-mers of the job)
    resident_rows = False         # capability: an owner's partition routed by its own reads alone is handed over as LocalRows, not collected
    array_payload = False         # capability: collect() gives arrays (rows + flags, or exchange.RaggedPiece) that travel as bytes, not pickles
    local_table = None            # capability, () -> table: a one-rank job's counted table as it is.  None: not offered
    graph_batch = None            # capability, (part, names, owned, mine, K, paired, sample, seed) -> {partition: FASTA} in stages of its
    #                               own, or None: "one partition at a time through graph(), please".  None: not offered
    graph_threads = 1             # tuning: threads over the owned partitions on the way through graph()
    device = None                 # where the rank's tensors live (None: the host); collectives are staged by exchange.coll_device
    ctx = None                    # device.Context for rank 0's merge (None: the host form)
    clock = Clock()               # side channel: the driver's Clock, for the ops' own stages and collectives
    strand_specific = False
    min_weight, min_length, kmer_hard_cutoff = 3, 75, 1       # (shannon.py:55-57, 237-247)



def assemble_distributed(ops, K=25, partition_size=500, sample="shannon", seed=0, part_vectors=None, group=None,
                         timings=None, lock=None, double_stranded=True, min_weight=3, min_length=75, kmer_hard_cutoff=1, filter_fp=False):
    """Returns on rank 0 a dict {partitions: {name: fasta}, final, contigs, ...}; None elsewhere.
    filter_fp: --filter_FP (shannon.py:170-195, run_MB_SF_fn.py:110, 272-277) -- between the owners' sparse flow and the gather every
    partition's transcripts are held against the read pairs ALL ranks routed to it (filter_owned_texts); "partitions" and "final" are
    the filtered ones, rank 0's dict gains "partitions_org", "filter_logs" and "filter_fp_stats".  Paired input only, as in the
    reference (single-end: "filter_fp_note" says so, nothing is filtered); ops without filter_cover / filter_count are refused.
    min_weight / min_length: hyp_min_weight (--kmer_soft_cutoff) / hyp_min_length as run_correction gets them (shannon.py:243-247,
    457); kmer_hard_cutoff: `jellyfish dump -L` (shannon.py:237-241, 441), applied by the ops to the REDUCED counts -- on the owner
    of a k1-mer after the bucket exchange, never to a rank's local counts.  The ops read them as attributes of the same names.
    double_stranded=False (-s / --ss / --strand_specific, shannon.py:407-411): the reads are not strand-doubled -- forward counting
    of reads_1 and RC(reads_2), routes of plain read indices (the global order is the global read index, there is no
    reverse-complement half), pairs (reads_1[i], RC(reads_2[i])) at the owners, process_concatenated_fasta with the user's flag
    (:596).  The ops say whether they can (`ops.strand_specific`, set here); ops without the attribute `supports_strand_specific`
    are refused rather than run double-stranded.
    timings: seconds per stage, compute ("count", "extension", ...) and collectives ("x:...") apart.
    lock (development aid): held while this rank computes, free around every collective and on entry, return and raise (Clock)."""
    ss = not double_stranded
    if filter_fp and not (hasattr(ops, "filter_cover") and hasattr(ops, "filter_count")):
        raise ValueError("assemble_distributed: filter_fp=True needs ops that map read pairs onto transcripts (filter_cover / filter_count: "
                         "GpuOps has them); these ops do not, and nothing would be filtered")
    if ss and not getattr(ops, "supports_strand_specific", False):
        raise NotImplementedError("assemble_distributed: these ops do not implement -s / --strand_specific (forward counting, plain read "
                                  "indices, pairs of reads_1 and RC(reads_2)); a strand_specific run needs ops that do (GpuOps does)")
    ops.strand_specific = ss
    ops.min_weight, ops.min_length, ops.kmer_hard_cutoff = int(min_weight), int(min_length), int(kmer_hard_cutoff)
    ops.clock = clock = Clock(timings, lock)
    # What the stages share.  Left behind by _table: table, n_k1mers, presharded; _extension: res; _route: part, names, n_local, base,
    # n_glob, allc; _deal_and_collect: cutoffs, owner, payload; _exchange_reads: recv; _graphs: texts, err; the filter: extra.
    S = SimpleNamespace(ops=ops, clock=clock, group=group, W=dist.get_world_size(group), rank=dist.get_rank(group), K=K, partition_size=partition_size,
                        sample=sample, seed=seed, part_vectors=part_vectors, ss=ss, presharded=None, err=None, extra=None)
    _table(S)
    _extension(S)
    _route(S)
    _deal_and_collect(S)
    _exchange_reads(S)
    _graphs(S)
    if filter_fp:
        S.texts, S.extra, S.err = _filter_step(ops, S.part, S.texts, S.names, S.owner, group, clock, S.err)
    return _gather_and_merge(S.texts, S.names, S.res, S.n_k1mers, group, clock, error=S.err, device=ops.device, ctx=ops.ctx,
                             double_stranded=double_stranded, extra=S.extra)


def _table(S):
    """1. The k1-mer table this rank extends.  Which of the three ways is decided here and nowhere else; SHN_OWNER_LABELS=2 (tests)
    takes a one-rank job through the owner shards."""
    forced = os.environ.get("SHN_OWNER_LABELS") == "2" and S.ops.owner_labelling
    if S.W == 1 and S.ops.local_table is not None and not forced:
        _table_one_rank(S)
    elif S.ops.owner_labelling:
        _table_owner_shards(S)
    else:
        _table_replicated(S)


def _table_one_rank(S):
    """One rank: nothing to exchange, reduce or gather -- the counted table IS the table (it used to be exported to pairs, reduced
    into a table, exported again and rebuilt: two passes through the pairs path, 0.2 s at configs[2]).  No collective."""
    with S.clock.stage("count"):
        S.table = S.ops.local_table()
        S.n_k1mers = len(S.table)


def _exchanged_pairs(S, by_minimizer):
    """local count, then the (key, count) pairs to the ranks that own them.  Collective: the bucket exchange (one all-to-all)."""
    with S.clock.stage("count"):
        keys, counts, send = S.ops.local_pairs(S.W, by_minimizer=by_minimizer)
    with S.clock.collective("x:bucket exchange"):
        rk, rc, _ = exchange.all_to_all_pairs(keys, counts, send, S.group)
    return rk, rc


def _table_owner_shards(S):
    """No rank ever holds the whole table (BASELINE configs[4]): the k1-mers go to the rank that owns their minimizer, the components
    of the k1-mer graph are labelled on those shards (local union-find + one exchange of the edges that cross shards), and whole
    components travel to the rank that walks them -- a table of its own per rank, the unsharded extension on it.
    Collectives: the bucket exchange, then those of component_table."""
    rk, rc = _exchanged_pairs(S, True)
    with S.clock.stage("reduce"):
        owned = S.ops.owned_table(rk, rc)
        del rk, rc
    S.table, S.n_k1mers = S.ops.component_table(owned, S.group)
    S.presharded = S.n_k1mers


def _table_replicated(S):
    """The path of rounds 2-4, kept for comparison: every rank reduces the pairs it owns, the (small) distinct-k1-mer table is
    replicated, extension + partitioning on every rank.  Collectives: the bucket exchange, two all-gathers (keys, counts)."""
    rk, rc = _exchanged_pairs(S, False)
    with S.clock.stage("reduce"):
        ok, oc = S.ops.reduce_pairs(rk, rc)
    with S.clock.collective("x:allgather table"):
        gk, _ = _all_gather_var(ok, S.group)
        gc, _ = _all_gather_var(oc, S.group)
    with S.clock.stage("table"):
        S.table = S.ops.table_from_pairs(gk, gc)
    S.n_k1mers = int(gk.numel())


def _extension(S):
    """2. Greedy extension + contig stage on the rank's table -> S.res.  Collectives: the ops' own, if they shard the work over the
    group ("x:contig gathers": GpuOps gathers what the shards' contig stages accept)."""
    with S.clock.stage("extension"):
        S.res = S.ops.extension(S.table, S.partition_size, S.group, presharded=S.presharded)
    del S.table


def _forward_routes(r, n_local):
    """how many of a partition's routes (ascending doubled indices) lie in the forward half.  A route is an array or a
    kmers_for_component.RouteView, which knows: that depends on how the partition was routed, not on the ops."""
    return r.count_below_split() if hasattr(r, "count_below_split") else int(np.searchsorted(r, n_local))


def _route(S):
    """3a. Partitions, this rank's routes into them, and every rank's routed reads per partition and strand half (S.allc [W, P, 2]):
    the global strand-doubled order is all ranks' forward reads in rank order, then all ranks' reverse halves.
    Collectives: two all-gathers of int64 (reads per rank; the counts), "x:route counts"."""
    ops, group, W = S.ops, S.group, S.W
    with S.clock.stage("partition+route"):
        S.part = ops.route(S.res, S.K, S.partition_size, S.part_vectors)
        S.names = list(S.part["new_components"])
        P = len(S.names)
        S.n_local = ops.n_reads()
        cnt = np.zeros((P, 2), dtype=np.int64)          # routed reads of this rank: forward half / RC half
        for i, nm in enumerate(S.names):
            r = S.part["routes"][nm]
            f = _forward_routes(r, S.n_local)
            cnt[i] = (f, len(r) - f)
        with S.clock.collective("x:route counts"):
            cdev = exchange.coll_device(ops.device, group)
            nl = torch.tensor([S.n_local], dtype=torch.int64, device=cdev)
            nls = [torch.zeros_like(nl) for _ in range(W)]
            dist.all_gather(nls, nl, group=group)
            nls = [int(x.item()) for x in nls]
            ct = torch.as_tensor(cnt.reshape(-1), device=cdev)
            cts = [torch.zeros_like(ct) for _ in range(W)]
            dist.all_gather(cts, ct, group=group)
            S.allc = np.stack([c.cpu().numpy().reshape(P, 2) for c in cts])
    S.base, S.n_glob = sum(nls[:S.rank]), sum(nls)


def read_caps(allc, cutoffs, rank):
    """How many of its forward and of its reverse-half routed reads rank `rank` sends for every partition, when a partition's graph
    consumes the first cutoffs[p] reads of the global strand-doubled order (multibridging.py:26-30).  allc [W, P, 2]: every rank's
    routed reads per partition, forward / reverse half.  The kept reads are prefixes of the rank's two halves.  -> (keep_f, keep_r) [P]"""
    allc, cutoffs = np.asarray(allc, dtype=np.int64), np.asarray(cutoffs, dtype=np.int64)
    # position of this rank's first forward / first RC routed read of partition p in the global order
    fwd_before = allc[:rank, :, 0].sum(axis=0)
    rc_before = allc[:, :, 0].sum(axis=0) + allc[:rank, :, 1].sum(axis=0)
    keep_f = np.maximum(0, np.minimum(allc[rank, :, 0], cutoffs - fwd_before))
    keep_r = np.maximum(0, np.minimum(allc[rank, :, 1], cutoffs - rc_before))
    return keep_f, keep_r


def _deal_and_collect(S):
    """3b. The owner of every partition, the reads under its cap, and this rank's share of them per destination (S.payload: per rank
    [(partition, global doubled indices, reads)]).  No collective: every rank deals alike from the gathered counts."""
    ops, part, names, allc, rank = S.ops, S.part, S.names, S.allc, S.rank
    with S.clock.stage("collect reads"):
        # owner of every partition: largest first onto the least loaded rank (load = the reads its graph will consume, known to
        # every rank from the gathered counts) -- the reference's size-sorted job list (shannon.py:546-551) dealt over the ranks
        S.cutoffs = np.array([10 * ops.n_nodes(part, nm, S.K) + 1 for nm in names], dtype=np.int64)
        S.owner = deal_partitions(np.minimum(allc.sum(axis=(0, 2)), S.cutoffs) + 1, S.W)
        keep_f, keep_r = read_caps(allc, S.cutoffs, rank)
        S.payload = [[] for _ in range(S.W)]
        for i, nm in enumerate(names):
            kf, kr = int(keep_f[i]), int(keep_r[i])
            if kf + kr == 0:
                continue
            r = part["routes"][nm]                      # array, or a RouteView: only the kept prefixes are fetched
            f = int(allc[rank, i, 0])
            rf, rr = np.asarray(r[:kf], dtype=np.int64), np.asarray(r[f:f + kr], dtype=np.int64)
            sel = np.concatenate([rf, rr])
            gidx = np.concatenate([S.base + rf, S.n_glob + S.base + (rr - S.n_local)])
            if not S.ss and int(S.owner[i]) == rank and ops.resident_rows and int(allc[:, i, :].sum()) == int(allc[rank, i].sum()):
                # every routed read of this partition is a row of this rank's own resident input, and this rank owns the partition:
                # nothing is collected -- the graph stage names the reads by their rows, as the single-GPU pipeline does
                S.payload[rank].append((i, gidx, LocalRows(sel)))
            else:
                S.payload[int(S.owner[i])].append((i, gidx, ops.collect(sel)))


def _exchange_reads(S):
    """3c. The capped reads to the partitions' owners -> S.recv, per source rank.  Collective: one all-to-all(v) of bytes
    (array_payload), or of python objects through one all-gather (the oracle-backed test ops: small inputs only)."""
    ops, rank = S.ops, S.rank
    with S.clock.collective("x:read exchange"):
        if ops.array_payload:                       # code rows + flags; what a rank owns itself stays put
            got = exchange.all_to_all_bytes([exchange.pack_read_pieces(items if d != rank else []) for d, items in enumerate(S.payload)], ops.device, S.group)
            S.recv = [exchange.unpack_read_pieces(b) if src != rank else S.payload[rank] for src, b in enumerate(got)]
        else:
            S.recv = [None] * S.W
            _a2a_objects(S.recv, S.payload, S.group)
    del S.payload


def _graphs(S):
    """4. Graph + sparse flow of the partitions this rank owns -> S.texts {partition: FASTA}.  No collective.  Either all of them
    through the single-GPU graph stage (ops.graph_batch), whose failure is kept in S.err and told to every rank in the gather --
    nobody waits there for a rank that has left; or, where the ops have no batch or it declines, one partition at a time."""
    ops = S.ops
    with S.clock.stage("graph"):
        mine = {}
        for lst in S.recv:
            for p, gidx, data in lst:
                mine.setdefault(p, []).append((gidx, data))
        del S.recv
        owned = sorted((i for i in range(len(S.names)) if int(S.owner[i]) == S.rank), key=lambda i: -int(min(S.allc[:, i, :].sum(), S.cutoffs[i])))
    S.texts = None
    if ops.graph_batch is not None:
        try:
            S.texts = ops.graph_batch(S.part, S.names, owned, mine, S.K, ops.paired, S.sample, S.seed)
        except Exception as ex:
            S.texts, S.err = {}, "%s: %s" % (type(ex).__name__, ex)
    if S.texts is None:
        S.texts = _graphs_one_by_one(S, owned, mine)


def _graphs_one_by_one(S, owned, mine):
    """ops.graph per owned partition (independent: threads, the native stage releases the GIL), one ops.sparse_flow over all"""
    ops, names = S.ops, S.names

    def one(i):
        singles, comps = ops.graph(S.part, names[i], mine.get(i, []), S.K, ops.paired)      # pieces: [(global indices, reads)] per source rank
        return (i, singles, comps)

    with S.clock.stage("graph"):
        nthreads = min(len(owned), ops.graph_threads)
        if nthreads > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=nthreads) as pool:
                jobs = list(pool.map(one, owned))
        else:
            jobs = [one(i) for i in owned]
    with S.clock.stage("sparse flow"):
        flat = [(c["nodes"], c["edges"], c["paths"]) for _, _, comps in jobs for c in comps]
        ids = [c for _, _, comps in jobs for c in range(len(comps))]
        trs = ops.sparse_flow(flat, ids, S.seed) if flat else []
        k, texts = 0, {}
        for i, singles, comps in jobs:
            sname = "%s_%s" % (S.sample, names[i])
            texts[i] = "".join(sparse_flow.fasta_records(sname, str(c), trs[k + c]) for c in range(len(comps))) + sparse_flow.single_nodes_fasta(sname, singles)
            k += len(comps)
    return texts


def _filter_step(ops, part, texts, names, owner, group, clock, err):
    """5. --filter_FP between the owners' sparse flow and the gather: (texts for the merge, what travels beside them, error).  Whether
    it runs is decided from what every rank holds (the flag, ops.paired): all ranks reach filter_owned_texts' collectives or none."""
    if not ops.paired:
        return texts, {"note": "--filter_FP: single-end input -- the reference sets the flag only for paired-end runs "
                               "(run_MB_SF_fn.py:110); nothing filtered"}, err
    kept, org, logs, stats, ferr = filter_owned_texts(texts, names, owner, lambda seqs, part_of, n_parts: ops.filter_cover(part, seqs, part_of, n_parts),
                                                      ops.filter_count, ops.device, group, clock)
    return kept, {"org": org, "logs": logs, "stats": stats}, err or ferr


def _runs_of(owner, d):
    """[(first, last + 1)] of the maximal runs of consecutive partitions that rank d owns"""
    runs = []
    for i in np.nonzero(np.asarray(owner) == d)[0].tolist():
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [tuple(r) for r in runs]


def filter_owned_texts(texts, names, owner, cover, count, device=None, group=None, clock=None):
    """--filter_FP on N ranks (filter_FP.py:29-55 as run_MB_SF_fn.py:272-277 runs it per partition).  A fragment lives on one rank; its
    minimum cost and the placements that attain it depend on the fragment and on its partition's transcripts alone, and coverage is a
    set union over fragments: the OR over the ranks of what each rank's pairs cover IS the one-process bitmap, provided every rank
    marks the same layout of the same transcripts.
      texts   {partition index: unfiltered FASTA text} of the partitions this rank owns (owner[i] == rank)
      cover   (seqs, part_of, n_parts) -> (uint64 bitmap of the layout filter_fp.text_offsets(seqs), {"routes", "placed"}): what this
              rank's routes cover (GpuOps.filter_cover: shn_filter_fp_cover; the CPU tests: numpy)
      count   (covers [W, n_words], t_off, word0) -> hits (GpuOps.filter_count: shn_filter_fp_count; filter_fp.hits_from_bitmaps(None, ...))
    1. the owners' texts to every rank (all-gather of bytes), parsed and laid out in partition order: one layout on all ranks;
    2. cover; 3. for every owner the words under each run of its partitions (one all-to-all of bytes; a boundary word may carry a
    neighbour's bits, count ignores them), the owner counts over the W pieces; 4. the owner decides (filter_fp._filter_records).
    Every rank reaches every collective: a rank whose cover or count raises goes on with zeros and returns the message.
    clock: one stage "filter_FP" with the three collectives inside it (Clock); called between two stages.
    Returns (kept {i: text}, org {i: text as given}, logs {i: rec.log text}, stats summed over the ranks, error or None)."""
    from . import filter_fp as ffp
    W, rank = dist.get_world_size(group), dist.get_rank(group)
    clock = clock or Clock()
    cdev = exchange.coll_device(device, group)
    P = len(names)
    err = None
    with clock.stage("filter_FP"):
        # ---- 1. texts to every rank
        mine = {int(i): _as_bytes(t) for i, t in texts.items()}
        buf = _pack_columns({i: [a] for i, a in mine.items()}, 1)
        with clock.collective("x:filter_FP texts"):
            got = exchange.all_gather_arrays((buf,), cdev, group, "filter_FP texts (the owners' unfiltered transcripts to every rank, all-gather)")
        n_words = 0
        seqs, part_of, first = [], [], np.zeros(P + 1, dtype=np.int64)
        parsed = [([], [])] * P
        try:
            every = {}
            for (b,) in got:
                every.update({i: cols[0] for i, cols in _unpack_columns(b, 1).items()})
            parsed = [ffp.records(every[i]) if i in every else ([], []) for i in range(P)]
            for i, (_nm, sq) in enumerate(parsed):
                seqs += sq
                part_of += [i] * len(sq)
                first[i + 1] = len(seqs)
            t_off = ffp.text_offsets(seqs)
            n_words = (int(t_off[-1]) + 63) // 64
        except Exception as ex:
            err = "%s: %s" % (type(ex).__name__, ex)
            seqs, part_of, first, t_off = [], [], np.zeros(P + 1, dtype=np.int64), np.zeros(1, np.uint64)
        # ---- 2. what this rank's routes cover
        st = {}
        bitmap = None
        if err is None:
            try:
                bitmap, st = cover(seqs, part_of, P)
                bitmap = np.ascontiguousarray(bitmap, dtype=np.uint64)
                if bitmap.shape != (n_words,):
                    raise ValueError("filter_owned_texts: a bitmap of %s words for a text of %d" % (bitmap.shape, n_words))
            except Exception as ex:
                err, bitmap = "%s: %s" % (type(ex).__name__, ex), None
        if bitmap is None:
            bitmap = np.zeros(n_words, dtype=np.uint64)
        # ---- 3. the words under every owner's partitions to that owner
        def windows(d):           # [(first transcript, behind the last, first word, behind the last word)] per run of d's partitions
            out = []
            for a, b in _runs_of(owner, d):
                ta, tb = int(first[a]), int(first[b])
                if tb > ta:
                    out.append((ta, tb, int(t_off[ta]) >> 6, (int(t_off[tb]) + 63) // 64))
            return out
        send = [np.concatenate([bitmap[w0:w1] for _a, _b, w0, w1 in windows(d)] + [np.zeros(0, np.uint64)]).view(np.uint8) for d in range(W)]
        with clock.collective("x:filter_FP coverage"):
            got = exchange.all_to_all_bytes(send, device, group, "filter_FP coverage (every rank's bitmap words under an owner's partitions, all-to-all)")
        hits = np.zeros(len(seqs), dtype=np.uint32)
        if err is None:
            try:
                pieces = [np.ascontiguousarray(b).view(np.uint64) for b in got]
                at = 0
                for ta, tb, w0, w1 in windows(rank):
                    covers = np.stack([p_[at:at + (w1 - w0)] for p_ in pieces])
                    hits[ta:tb] = count(covers, t_off[ta:tb + 1], w0)
                    at += w1 - w0
            except Exception as ex:
                err = "%s: %s" % (type(ex).__name__, ex)
        # ---- 4. the owner decides
        kept, org, logs = {}, {}, {}
        n_tr = n_kept = 0
        for i in sorted(mine):
            nm, sq = parsed[i]
            k, lg = "", ""
            if err is None:
                try:
                    k, lg = ffp._filter_records(nm, sq, hits[int(first[i]):int(first[i + 1])].tolist())
                except Exception as ex:
                    err = "%s: %s" % (type(ex).__name__, ex)
            kept[i], org[i], logs[i] = k, mine[i], lg
            n_tr += len(sq)
            n_kept += k.count(">")
        with clock.collective("x:filter_FP coverage"):
            parts = exchange.all_gather_object((int(st.get("routes", 0)), int(st.get("placed", 0)), n_tr, n_kept), group, "filter_FP counters")
        tot = np.asarray(parts, dtype=np.int64).sum(axis=0).tolist()
    return kept, org, logs, dict(zip(("routes", "placed", "transcripts", "kept"), tot)), err


class LocalRows(object):
    """the reads of a partition as doubled read indices into the owner's own resident input (no rows collected)"""
    def __init__(self, sel):
        self.sel = np.ascontiguousarray(sel, dtype=np.uint32)

    def __len__(self):
        return len(self.sel)


class _Texts(Mapping):
    """{partition name: reconstructed FASTA}; the texts stay the byte arrays they arrived as until somebody reads one"""
    def __init__(self, names, arrays):
        self._names, self._a = list(names), dict(zip(names, arrays))

    def __getitem__(self, k):
        return bytes(memoryview(self._a[k])).decode()

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


def _as_bytes(t):
    return np.frombuffer(t.encode(), dtype=np.uint8) if isinstance(t, str) else np.ascontiguousarray(t, dtype=np.uint8)


def _pack_columns(cols, ncol):
    """{partition index: [ncol uint8 arrays]} -> one uint8 array: the count, (index, sizes) per partition, then the bytes"""
    idx = sorted(cols)
    head = np.asarray([len(idx)] + [v for i in idx for v in [i] + [cols[i][c].size for c in range(ncol)]], dtype=np.int64).view(np.uint8)
    return np.concatenate([head] + [cols[i][c] for i in idx for c in range(ncol)])


def _unpack_columns(b, ncol):
    """inverse of _pack_columns (views into b)"""
    out = {}
    if b.size == 0:
        return out
    n = int(b[:8].view(np.int64)[0])
    wd = 8 * (1 + ncol)
    head = b[8:8 + wd * n].view(np.int64).reshape(n, 1 + ncol)
    pos = 8 + wd * n
    for row in head.tolist():
        out[int(row[0])] = []
        for sz in row[1:]:
            out[int(row[0])].append(b[pos:pos + sz])
            pos += sz
    return out


def _gather_and_merge(texts, names, res, n_k1mers, group, clock=None, error=None, device=None, ctx=None, double_stranded=True, extra=None):
    """6. The per-partition FASTA of every owner to rank 0, which merges (shannon.py:584-604).  error: what went wrong in this rank's
    graph stage, if anything -- it travels with the gather, so every rank raises together and none is left waiting.
    extra (--filter_FP): {"org", "logs": {i: text}, "stats"} -- the unfiltered texts and the rec.log texts travel beside the kept
    ones (three columns per partition instead of one), rank 0's dict gains partitions_org / filter_logs / filter_fp_stats; or
    {"note": ...} for a run that was not filtered.  device, ctx: the ops' (where the bytes are staged; the merge on the device).
    Collectives ("x:gather fasta"): the status of the ranks (one all-gather of objects), the texts (one all-to-all of bytes)."""
    W, rank = dist.get_world_size(group), dist.get_rank(group)
    clock = clock or Clock()
    filtered = extra is not None and "org" in extra
    ncol = 3 if filtered else 1
    cols = {}
    with clock.collective("x:gather fasta"):
        # what went wrong, if anything (a few bytes per rank); then the texts as bytes to rank 0 -- what rank 0 produced itself stays put
        errs = exchange.all_gather_object(error, group, "FASTA gather (status of the ranks)")
        errors = ["rank %d: %s" % (r, e) for r, e in enumerate(errs) if e]
        if errors:
            raise RuntimeError("graph stage failed on " + "; ".join(errors))
        mine = {int(i): [_as_bytes(t)] + ([_as_bytes(extra["org"][i]), _as_bytes(extra["logs"][i])] if filtered else []) for i, t in texts.items()}
        if W > 1:
            if rank != 0:
                out = _pack_columns(mine, ncol)
            bufs = [out if (d == 0 and rank != 0) else np.zeros(0, np.uint8) for d in range(W)]
            got = exchange.all_to_all_bytes(bufs, device, group, "FASTA gather (per-partition transcripts to rank 0)")
            if rank == 0:
                for src, b in enumerate(got):
                    if src != 0:
                        cols.update(_unpack_columns(b, ncol))
    if rank != 0:
        return None
    with clock.stage("merge (rank 0)"):
        cols.update(mine)
        merged = {i: c[0] for i, c in cols.items()}
        single = "".join(">Single_%d\n%s\n" % (i, c) for i, c in enumerate(res.single_contigs))
        order = [merged[i] for i in range(len(names))]
        # the merge over the texts as they are (process_concatenated_fasta.py + faster_reps.py: post.finalize_texts, on the device when
        # there is a context); transcripts with characters outside ACGT go through the Python form
        try:
            final = post.finalize_texts([single] + order, double_stranded, ctx=ctx)
        except _lib.ShannonError as ex:
            if "non-ACGT" not in str(ex) and "empty line" not in str(ex):
                raise
            lines = single.splitlines(True)
            for a in order:
                lines += bytes(memoryview(a)).decode().splitlines(True)
            final = post.finalize(lines, double_stranded)
        parts = _Texts(names, order)
    out = {"partitions": parts, "final": final, "contigs": res.contigs, "n_k1mers": int(n_k1mers or 0),
           "extension": {k: getattr(res, k, None) for k in ("iterations", "n_walks", "total_steps", "wave_steps", "fresh_steps", "dense_rounds")}}
    if filtered:
        out["partitions_org"] = _Texts(names, [cols[i][1] for i in range(len(names))])
        out["filter_logs"] = _Texts(names, [cols[i][2] for i in range(len(names))])
        out["filter_fp_stats"] = dict(extra["stats"])
    elif extra is not None:
        out["filter_fp_note"] = extra["note"]
    return out


def _a2a_objects(recv, payload, group):
    """all-to-all of python objects via all_gather_object (small payloads only)."""
    W, rank = dist.get_world_size(group), dist.get_rank(group)
    everything = [None] * W
    dist.all_gather_object(everything, payload, group=group)
    for src in range(W):
        recv[src] = everything[src][rank]


def component_table(cc, group, clock=None, dev=None):
    """Component labelling on owner shards, the collectives around it.  cc: this rank's shard behind the steps of
    include/shannon_hip.h's shn_cc_* (GpuOps: the device kernels; the CPU tests: a numpy restatement) --
      cc.n                                     k1-mers of the shard
      cc.queries() -> (keys i64, roots i32, per destination rank)      what higher ranks are asked
      cc.answer(keys, roots, per source rank, base) -> edges i64 [2 E] pairs of global ids (base[r] + local root)
      cc.solve(edges, id_limit) -> (ids ascending, label of each)       the component graph, the same on every rank
      cc.labels(base_me, ids, labels) -> i64 [n]                        global label of every k1-mer of the shard
      cc.sizes(glabel, at_least) -> (labels, counts) numpy              what this rank holds of the larger components
      cc.shard(glabel, big labels ascending, their ranks) -> (keys i64, counts i32, per destination rank)
    Collectives: the shard sizes (all-gather), the queries (all-to-all), the edges (all-gather), the sizes of the large components
    (objects), the pairs of whole components (all-to-all).  Returns ((keys, counts) received: this rank's components, k1-mers of
    the job).  clock: the "labels: ..." stages and the collectives between them (Clock); called between two stages."""
    W, rank = dist.get_world_size(group), dist.get_rank(group)
    clock = clock or Clock()
    cdev = exchange.coll_device(dev, group)
    with clock.stage("labels: local components + queries"):
        n_loc = int(cc.n)
        qk, ql, per = cc.queries()
    with clock.collective("x:label queries"):
        nt = torch.tensor([n_loc], dtype=torch.int64, device=cdev)
        nts = [torch.zeros_like(nt) for _ in range(W)]
        dist.all_gather(nts, nt, group=group)
        sizes = [int(x.item()) for x in nts]
        base = [sum(sizes[:r]) for r in range(W)]
        n_glob = sum(sizes)
        rk, rl, rcl = exchange.all_to_all_pairs(qk, ql, per, group, name="component labelling: neighbour queries to the owners (all-to-all)")
        del qk, ql
    with clock.stage("labels: answers"):
        edges = cc.answer(rk, rl, rcl, base)
        del rk, rl
    with clock.collective("x:label edges"):
        ge, _ = _all_gather_var(edges, group, name="component labelling: edges between shards (all-gather)")
        del edges
    with clock.stage("labels: component graph"):
        ids, labels = cc.solve(ge, n_glob + 1)
        del ge
        glabel = cc.labels(base[rank], ids, labels)
        del ids, labels
        # the large components are balanced by size (largest first onto the least loaded rank, as shn_extend_sharded does on a
        # replicated table); everything else goes by the hash of its label.  A component of T k1-mers spread evenly has T / W of them
        # here: every rank reports what it holds of components above a quarter of that, every rank sums the same reports.
        T = max(1024, n_glob // (64 * W))
        mine = cc.sizes(glabel, max(32, T // (4 * W)))
    with clock.collective("x:label sizes"):
        parts = exchange.all_gather_object(mine, group, "component labelling: sizes of the large components")
    with clock.stage("labels: owners + shard"):
        tot = {}
        for lab, cnt in parts:
            for a, b in zip(np.asarray(lab).tolist(), np.asarray(cnt).tolist()):
                tot[a] = tot.get(a, 0) + b
        big = sorted((a for a, b in tot.items() if b >= T // 2), key=lambda a: (-tot[a], a))
        load = [0] * W
        own = {}
        for a in big:
            r = min(range(W), key=lambda q: (load[q], q))
            own[a] = r
            load[r] += tot[a]
        bl = sorted(own)
        sk, sc, send = cc.shard(glabel, np.asarray(bl, dtype=np.int64), np.asarray([own[a] for a in bl], dtype=np.uint8))
        del glabel
    with clock.collective("x:component exchange"):
        rk, rc, _ = exchange.all_to_all_pairs(sk, sc, send, group, name="component exchange (the k1-mers of whole components to their rank, all-to-all)")
        del sk, sc
    return (rk, rc), n_glob


class _GpuComponents(object):
    """the steps of component_table() on the device (device.ComponentShards = shn_cc_*), tensors on the rank's GPU"""

    def __init__(self, ops, owned, W, rank):
        self.ops, self.dev, self.n = ops, ops.device, len(owned)
        self.cc = ops._dev.ComponentShards(ops.ctx, owned, W, rank)

    def queries(self):
        per = self.cc.query_counts()
        nq = int(per.sum())
        qk = torch.empty(max(nq, 1), dtype=torch.int64, device=self.dev)
        ql = torch.empty(max(nq, 1), dtype=torch.int32, device=self.dev)
        self.cc.queries(qk.data_ptr(), ql.data_ptr())
        return qk, ql, per

    def answer(self, rk, rl, rcl, base):
        torch.cuda.synchronize()
        edges = torch.empty(2 * max(int(sum(rcl)), 1), dtype=torch.int64, device=self.dev)
        ne = self.cc.answer(rk.data_ptr(), rl.data_ptr(), rcl, base, edges.data_ptr())
        return edges[:2 * ne]

    def solve(self, ge, id_limit):
        torch.cuda.synchronize()
        E = int(ge.numel()) // 2
        ids = torch.empty(2 * max(E, 1), dtype=torch.int64, device=self.dev)
        labels = torch.empty(2 * max(E, 1), dtype=torch.int64, device=self.dev)
        nn = self.cc.solve(self.ops.ctx, ge.data_ptr(), E, id_limit, ids.data_ptr(), labels.data_ptr())
        return ids[:nn], labels[:nn]

    def labels(self, base_me, ids, labels):
        glabel = torch.empty(max(self.n, 1), dtype=torch.int64, device=self.dev)
        self.cc.labels(base_me, ids.data_ptr(), labels.data_ptr(), int(ids.numel()), glabel.data_ptr())
        return glabel

    def sizes(self, glabel, at_least):
        torch.cuda.synchronize()
        u, c = torch.unique(glabel[:self.n], return_counts=True)
        sel = c >= at_least
        return u[sel].cpu().numpy(), c[sel].cpu().numpy()

    def shard(self, glabel, big, big_owner):
        n_big = len(big)
        dbig = torch.as_tensor(big if n_big else np.zeros(1, np.int64), device=self.dev)
        dbo = torch.as_tensor(big_owner if n_big else np.zeros(1, np.uint8), device=self.dev)
        owner = torch.empty(max(self.n, 1), dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        self.cc.owners(glabel.data_ptr(), dbig.data_ptr(), dbo.data_ptr(), n_big, owner.data_ptr())
        sk = torch.empty(max(self.n, 1), dtype=torch.int64, device=self.dev)
        sc = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.dev)
        send = self.cc.shard(owner.data_ptr(), sk.data_ptr(), sc.data_ptr())
        return sk, sc, send

    def close(self):
        self.cc.close()


class GpuOps(RankOps):
    """Per-rank compute on the local GPU through the C ABI."""

    def __init__(self, ctx, d1, d2, store, K):
        from . import device
        self.ctx, self.d1, self.d2, self.store, self.K = ctx, d1, d2, store, K
        self.paired = d2 is not None
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._dev = device

    supports_strand_specific = True

    def n_reads(self):
        return len(self.d1)

    def _hard_cutoff(self, t):
        """`jellyfish dump -L` (shannon.py:441) on a table of REDUCED counts (the job's, not a rank's slice)"""
        if self.kmer_hard_cutoff <= 1:
            return t
        kept = t.filter_lower(self.kmer_hard_cutoff)
        t.close()
        return kept

    def _count(self):
        if self.strand_specific:         # forward counting of reads_1 and RC(reads_2): a table of plain (not canonical) k1-mers
            return self._dev.count_k1mers_strand_specific(self.ctx, self.d1, self.d2, self.K + 1)
        return self._dev.count_k1mers(self.ctx, [self.d1, self.d2] if self.paired else [self.d1], self.K + 1, True)

    @property
    def owner_labelling(self):
        """components labelled on the owner shards, no replicated table (SHN_OWNER_LABELS=0: the table all-gathered to every rank and
        labelled there -- the path of rounds 2-4, kept for comparison)"""
        return os.environ.get("SHN_OWNER_LABELS", "1") != "0"

    def _digest(self, name, table):
        """SHN_DIST_DIGEST=1 (diagnostics): a checksum of a table's sorted (key, count) pairs per stage, in self.digests"""
        if os.environ.get("SHN_DIST_DIGEST") != "1":
            return
        import hashlib
        k, c = table.download()
        o = np.argsort(k, kind="stable")
        h = hashlib.sha256(np.ascontiguousarray(k[o]).tobytes() + np.ascontiguousarray(c[o]).tobytes()).hexdigest()[:16]
        if not hasattr(self, "digests"):
            self.digests = {}
        self.digests[name] = (int(len(k)), h)

    def local_pairs(self, W, by_minimizer=False):
        t = self._count()
        self._digest("counted", t)
        n = len(t)
        dk = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        dc = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        per = (t.shard_by_minimizer if by_minimizer else t.shard)(W, dk.data_ptr(), dc.data_ptr())
        t.close()
        return dk, dc, per

    def owned_table(self, rk, rc):
        """the pairs this rank owns, equal keys summed"""
        torch.cuda.synchronize()
        t = self._hard_cutoff(self._dev.Table.from_pairs(self.ctx, rk.data_ptr(), rc.data_ptr(), rk.numel(), self.K + 1, not self.strand_specific))
        self._digest("owned", t)
        return t

    def component_table(self, owned, group):
        """owned: this rank's shard of the k1-mers (by minimizer).  Returns (a table of the whole components dealt to this rank,
        the number of k1-mers of the job): component_table() above with the device kernels (include/shannon_hip.h: shn_cc_*)."""
        W, rank = dist.get_world_size(group), dist.get_rank(group)
        n_loc = len(owned)
        with self.clock.stage("labels: local components + queries"):
            cc = _GpuComponents(self, owned, W, rank)
        try:
            pairs, n_glob = component_table(cc, group, self.clock, self.device)
        finally:
            cc.close()
        with self.clock.stage("table"):
            owned.close()
            rk, rc = pairs
            torch.cuda.synchronize()
            table = self._dev.Table.from_pairs(self.ctx, rk.data_ptr(), rc.data_ptr(), rk.numel(), self.K + 1, not self.strand_specific)
        self._digest("components", table)
        self.component_table_sizes = (int(n_loc), int(len(table)), int(n_glob))      # owned shard, walked table, the job (tests, bench)
        return table, n_glob

    def local_table(self):
        """one-rank job: the counted table itself (no export to pairs)"""
        return self._hard_cutoff(self._count())

    def reduce_pairs(self, rk, rc):
        torch.cuda.synchronize()
        t = self._hard_cutoff(self._dev.Table.from_pairs(self.ctx, rk.data_ptr(), rc.data_ptr(), rk.numel(), self.K + 1, not self.strand_specific))
        n = len(t)
        dk = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        dc = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        t.shard(1, dk.data_ptr(), dc.data_ptr())           # the reduced pairs stay on the device (a one-way "shard")
        t.close()
        return dk[:n], dc[:n]

    def table_from_pairs(self, gk, gc):
        torch.cuda.synchronize()
        t = self._dev.Table.from_pairs(self.ctx, gk.data_ptr(), gc.data_ptr(), gk.numel(), self.K + 1, not self.strand_specific)
        self._digest("gathered", t)
        return t

    graph_threads = 8

    @property
    def resident_rows(self):
        """a partition whose routed reads are all rows of this rank's resident input is handed to the graph stage by rows"""
        # (one_length: the duplicate search on the device takes read sets of one length, as in pipeline.py; -s: the driver excludes it)
        return self.unitigs is not None and graph_intake.rows_possible(self.store, self.d1, self.d2, self.paired, False) and self.one_length
    array_payload = True               # collect() returns (code rows, strand flags): travels as bytes, not as pickles

    def extension(self, table, partition_size, group=None, presharded=None):
        """replicated table -> walks AND contig stages sharded by connected component of the k1-mer graph; the accepted
        contigs + their connections (a few MB) are all-gathered and merged in the global walk order.
        presharded = the number of k1-mers of the job: `table` holds the whole components dealt to this rank already (component_table);
        the walks are the unsharded ones on it, everything after them as before."""
        from . import extension_correction as ec
        W, rank = dist.get_world_size(group), dist.get_rank(group)
        clock, cdev = self.clock, exchange.coll_device(self.device, group)

        class Gather(object):                     # the collectives of the sharded contig stage (waiting for the slowest rank included)
            world = W

            @staticmethod
            def all_gather(obj):
                with clock.collective("x:contig gathers"):
                    return exchange.all_gather_object(obj, group, "contig gathers (accepted contigs + connections of the shards)")

            @staticmethod
            def all_gather_arrays(arrays):
                with clock.collective("x:contig gathers"):
                    return exchange.all_gather_arrays(arrays, cdev, group, "contig gathers (candidates of the shards: seed weights, keys, offsets, text)")

            @staticmethod
            def all_reduce_max(v):
                t = torch.tensor([int(v)], dtype=torch.int64, device=cdev)
                with clock.collective("x:contig gathers"):
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
                return int(t.item())

        Gather.rank = rank
        # (a large, diverse table -- BASELINE configs[2] and beyond: 10^8+ k1-mers, 10^5+ candidate contigs -- takes the path
        # "sharded walks + one replicated GPU contig stage" inside run_correction; a few deep gene families per rank -- the
        # weak-scaling workload, 5 M k1-mers per family -- keep their contig stages sharded too: SHN_CONTIG_GPU=1 / 0 forces either)
        res = ec.run_correction(self.ctx, table, self.min_weight, self.min_length, partition_size, want_allowed=False, shard=None if presharded is not None else (W, rank),
                                gather=Gather, timings=clock.timings, table_size=presharded)
        table.close()
        return res

    def route(self, res, K, partition_size, part_vectors):
        from . import kmers_for_component as kfc, mbgraph_native
        self.unitigs, self.part_index = None, None
        # (which way collect() goes on this rank; the CLI puts it beside its stage times -- the timings dict itself holds seconds only)
        self.collect_path = "device" if self.collect_on_device else "host"
        gpu_graph = K <= 31 and os.environ.get("SHN_GRAPH_GPU", "1") != "0"
        part = kfc.kmers_for_component(self.ctx, res, self.d1, self.d2, K, partition_size, part_vectors=part_vectors, want_rows=False,
                                       timings=self.clock.timings, lazy_routes=True, lazy_graph_inputs=gpu_graph,
                                       strand_specific=self.strand_specific)
        names = list(part["new_components"])
        if gpu_graph and names:
            # the raw K-mer graphs of ALL partitions contracted on every rank (a tenth of a second at 111 partitions): every rank
            # needs every partition's K-mer count for the read caps, the owners need the unitigs
            self.unitigs = mbgraph_native.Unitigs(self.ctx, [part["new_components"][nm] for nm in names], K, flat_text=part.get("flat_text"))
            self.part_index = {nm: i for i, nm in enumerate(names)}
        return part

    def n_nodes(self, part, name, K):
        if self.unitigs is not None:
            return self.unitigs.n_kmers(self.part_index[name])
        return part["n_kmer_nodes"][name]

    @staticmethod
    def _split_mates(rows, halves):
        """code rows of one length as (codes, offsets, codes of the second mates or None).  halves: the rows hold reads_1[i] and
        reads_2[i] of a -s pair side by side (collect), both mates under the same offsets"""
        n, L2 = rows.shape
        L = L2 // 2 if halves else L2
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        return np.ascontiguousarray(rows[:, :L]).reshape(-1), off, (np.ascontiguousarray(rows[:, L:]).reshape(-1) if halves else None)

    @staticmethod
    def _as_ragged(data, halves=False):
        """a fixed-length piece (rows, flags) as a RaggedPiece; halves: see _split_mates"""
        if isinstance(data, exchange.RaggedPiece):
            return data
        b1, off, b2 = GpuOps._split_mates(data[0], halves)
        return exchange.RaggedPiece(b1, off, data[1], b2, off if halves else None)

    @staticmethod
    def _merge_ragged(pieces, halves=False):
        """_merge_pieces for pieces that carry lengths: one RaggedPiece in the order of the global indices (a stable sort of the
        indices, one gather of the reads' runs of codes per mate)"""
        gidx = np.concatenate([g for g, _ in pieces])
        ps = [GpuOps._as_ragged(d, halves) for _, d in pieces]
        if any(p.paired != ps[0].paired for p in ps):
            raise ValueError("GpuOps: pieces with and without second mates for one partition")

        def joined(codes, offs):
            base = np.concatenate([[0], np.cumsum([int(o[-1]) for o in offs])]).astype(np.uint64)
            return np.concatenate(codes), np.concatenate([offs[0][:1]] + [o[1:] + b for o, b in zip(offs, base)])
        one = len(ps) == 1
        c1, o1 = (ps[0].codes, ps[0].off) if one else joined([p.codes for p in ps], [p.off for p in ps])
        c2, o2 = (None, None) if not ps[0].paired else ((ps[0].codes2, ps[0].off2) if one else joined([p.codes2 for p in ps], [p.off2 for p in ps]))
        rc1 = ps[0].rc if one else np.concatenate([p.rc for p in ps])
        if len(gidx) > 1 and not bool((gidx[1:] > gidx[:-1]).all()):
            order = np.argsort(gidx, kind="stable")
            c1, o1 = _lib.gather_segments(c1, o1, order)
            if c2 is not None:
                c2, o2 = _lib.gather_segments(c2, o2, order)
            rc1 = np.ascontiguousarray(rc1[order])
        return exchange.RaggedPiece(c1, o1, rc1, c2, o2)

    @staticmethod
    def _merge_pieces(pieces, halves=False):
        """the pieces of one partition from their source ranks -> (code rows, strand flags) in the global strand-doubled order; a
        RaggedPiece (codes + offsets instead of rows) where a piece carries lengths.  halves: see _as_ragged."""
        pieces = [p for p in pieces if len(p[0])]
        if any(isinstance(d, exchange.RaggedPiece) for _, d in pieces):
            return GpuOps._merge_ragged(pieces, halves)
        if not pieces:
            return np.zeros((0, 1), np.uint8), np.zeros(0, np.uint8)
        one = len(pieces) == 1                                    # (no copy of a 100 MB piece)
        gidx = pieces[0][0] if one else np.concatenate([g for g, _ in pieces])
        rows = np.ascontiguousarray(pieces[0][1][0] if one else np.concatenate([d[0] for _, d in pieces]))
        rc1 = np.ascontiguousarray(pieces[0][1][1] if one else np.concatenate([d[1] for _, d in pieces]))
        if len(gidx) > 1 and not bool((gidx[1:] > gidx[:-1]).all()):      # (one source rank: already in order)
            order = np.argsort(gidx, kind="stable")
            rows = _lib.gather_rows(rows, order)
            rc1 = np.ascontiguousarray(rc1[order])
        return rows, rc1

    def graph_batch(self, part, names, owned, mine, K, paired, sample, seed):
        """multibridging.main + algorithm_SF for the owned partitions, as the single-GPU pipeline runs them: the received code rows
        become a resident read set of their own (row i forward = doubled index i, reverse strand = n + i), the distinct reads are
        found on the device (shn_mbgraph_run_rows), all components go through shn_sparse_flow in one call.  {partition: FASTA};
        None without unitigs (SHN_GRAPH_GPU=0, K > 31): graph() per partition then."""
        import threading
        from concurrent.futures import ThreadPoolExecutor
        from . import mbgraph_native
        if self.unitigs is None:
            return None
        up = threading.Lock()

        def one(i):
            pieces = mine.get(i, [])
            local = pieces[0][1] if (len(pieces) == 1 and isinstance(pieces[0][1], LocalRows)) else None
            merged = (np.zeros((0, 1), np.uint8), np.zeros(0, np.uint8)) if local is not None else self._merge_pieces(pieces, self.strand_specific and paired)
            ragged = merged if isinstance(merged, exchange.RaggedPiece) else None
            rows, rc1 = (np.zeros((0, 1), np.uint8), np.zeros(0, np.uint8)) if ragged is not None else merged
            def run(rb):
                if ragged is not None or (self.strand_specific and len(rows)):
                    # reads that carry their lengths, or -s rows: codes + offsets straight to the graph stage, as the one-process
                    # path hands them over (pipeline.py: gather_codes / gather_codes_ss -> run_partition_handle)
                    b1, o1, b2, o2, r1, r2 = self._ragged_args(ragged, paired) if ragged is not None else self._rows_args(rows, rc1, paired)
                    return mbgraph_native.run_partition_handle(rb, 0 if rb is None else len(rb) // (K + 1), K, b1, o1, b2, o2, ctx=self.ctx, enc=1,
                                                               rc1=r1, rc2=r2, unitigs=self.unitigs, part=i)
                if local is not None and len(local):
                    # this rank's own reads, named by their rows in its resident input (as pipeline.assemble_resident does)
                    return mbgraph_native.run_partition_rows(self.ctx, self.unitigs, i, self.d1, self.d2 if paired else None, self.store.r1,
                                                             self.store.r2 if paired else None, local.sel, rb, 0 if rb is None else len(rb) // (K + 1))
                if len(rows) == 0:
                    z, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
                    return mbgraph_native.run_partition_handle(rb, 0 if rb is None else len(rb) // (K + 1), K, z, o, z if paired else None,
                                                               o if paired else None, ctx=self.ctx, unitigs=self.unitigs, part=i)
                with up:
                    d = self._dev.Reads.from_codes(self.ctx, rows)
                n = len(rows)
                didx = (np.arange(n, dtype=np.int64) + np.where(rc1 != 0, n, 0)).astype(np.uint32)
                try:
                    return mbgraph_native.run_partition_rows(self.ctx, self.unitigs, i, d, d if paired else None, rows, rows if paired else None,
                                                             didx, rb, 0 if rb is None else len(rb) // (K + 1))
                finally:
                    d.close()
            return graph_intake.with_k1mer_rows(run, part, names[i])     # (rows: a partition holding a cycle of condensable edges)
        nthreads = max(1, min(len(owned), _lib.host_cpus()))
        graphs, futs = [], []
        try:
            with self.clock.stage("graph"):
                if nthreads > 1:
                    with ThreadPoolExecutor(max_workers=nthreads) as pool:
                        futs = [pool.submit(one, i) for i in owned]
                        graphs = [f.result() for f in futs]
                else:
                    for i in owned:
                        graphs.append(one(i))
            with self.clock.stage("sparse flow"):
                texts = mbgraph_native.sparse_flow_native(self.ctx, graphs, ["%s_%s" % (sample, names[i]) for i in owned], seed, raw=True) if owned else []
            return {i: txt for i, txt in zip(owned, texts)}
        finally:
            # whatever happened: the graphs built so far and the unitigs go back now (a failing partition must not leave them to
            # the garbage collector; the caller tells the other ranks before the gather, _gather_and_merge)
            for g in (graphs or [f.result() for f in futs if f.done() and not f.cancelled() and f.exception() is None]):
                g.close()
            self.unitigs.close()
            self.unitigs = None

    def _ragged_args(self, m, paired):
        """(b1, o1, b2, o2, rc1, rc2) of run_partition_handle(enc=1) for a merged RaggedPiece.  Double-stranded pairs: the second
        mates are the same stored reads on the other strand (pipeline.py: b2, o2 = b1, o1; rc2 = 1 - rc1); -s pairs: reads_2 as
        stored, read reversed (rc2 = 1)."""
        n = len(m)
        b1 = m.codes if len(m.codes) else np.zeros(1, np.uint8)
        if self.strand_specific:
            if not paired:
                return b1, m.off, None, None, np.zeros(n, np.uint8), None
            if not m.paired:
                raise ValueError("GpuOps: a -s pair's piece without its second mates")
            return b1, m.off, (m.codes2 if len(m.codes2) else np.zeros(1, np.uint8)), m.off2, np.zeros(n, np.uint8), np.ones(n, np.uint8)
        if not paired:
            return b1, m.off, None, None, m.rc, None
        return b1, m.off, b1, m.off, m.rc, (1 - m.rc).astype(np.uint8)

    def _rows_args(self, rows, rc1, paired):
        """_ragged_args for merged code rows of one length + strand flags.  -s: reads_1[i] and, for pairs, reads_2[i] side by side
        (collect), the second mate read on its reverse strand -- the pairs (reads_1[i], RC(reads_2[i])) of shannon.py:407-411"""
        ss = self.strand_specific and len(rows) > 0
        b1, o1, b2 = self._split_mates(rows, ss and paired)
        o2 = o1 if paired else None
        if ss:
            return b1, o1, b2, o2, np.zeros(len(rows), np.uint8), (np.ones(len(rows), np.uint8) if paired else None)
        b1 = b1 if b1.size else np.zeros(1, np.uint8)
        return b1, o1, (b1 if paired else None), o2, rc1, ((1 - rc1).astype(np.uint8) if paired else None)

    def filter_cover(self, part, seqs, part_of, n_parts):
        """--filter_FP, this rank's half: (what ALL routes of this rank's reads cover on the transcripts `seqs`, as the bitmap of
        filter_fp.coverage_bitmap; routes looked at / fragments placed).  A rank without reads or routes covers nothing."""
        from . import filter_fp as ffp
        stats = self.filter_fp_local = {}                 # (this rank's own counters: tests, diagnostics)
        rdev = part.get("routes_dev")
        if rdev is None or len(self.d1) == 0:
            return np.zeros((int(ffp.text_offsets(seqs)[-1]) + 63) // 64, dtype=np.uint64), stats
        return ffp.coverage_bitmap(self.ctx, seqs, part_of, n_parts, self.d1, self.d2, rdev[0], self.strand_specific, stats=stats), stats

    def filter_count(self, covers, t_off, word0):
        """--filter_FP, the owner's half: covered bases of every transcript from the bitmaps of all ranks (shn_filter_fp_count)"""
        from . import filter_fp as ffp
        return ffp.hits_from_bitmaps(self.ctx, covers, t_off, word0)

    @property
    def one_length(self):
        """both stored mates are code matrices of one common read length: the pieces travel as rows"""
        # (any 2-D array, not only graph_intake.is_code_matrix: a matrix of another dtype or layout still travels as rows)
        r1, r2 = getattr(self.store, "r1", None), getattr(self.store, "r2", None)
        return (isinstance(r1, np.ndarray) and r1.ndim == 2 and
                (not self.paired or (isinstance(r2, np.ndarray) and r2.ndim == 2 and r2.shape[1] == r1.shape[1])))

    @property
    def collect_on_device(self):
        """SHN_COLLECT_DEVICE: unset -- the reads of a piece that carries lengths are collected from the resident sets
        (shn_reads_collect), rows of one length from the host matrices as ever; 0 -- the host everywhere; 1 -- the device everywhere"""
        v = os.environ.get("SHN_COLLECT_DEVICE", "")
        return v[:1] == "1" if self.one_length else v[:1] != "0"

    @staticmethod
    def _host_take(src, idx):
        """reads idx of a host store (a code matrix or device.RaggedCodes) as (codes, offsets)"""
        if isinstance(src, np.ndarray):
            rows = np.ascontiguousarray(src[idx])
            return rows.reshape(-1), np.arange(len(idx) + 1, dtype=np.uint64) * np.uint64(src.shape[1])
        c, o = src.take(idx)
        return c[:int(o[-1])], o

    def collect(self, sel):
        """the reads of the doubled indices `sel` as they travel to a partition's owner.  Code matrices of one common length: stored
        code rows + strand flags of the first mates (second mates: same rows, opposite strand).  Anything else -- reads of
        different lengths, mates of two lengths: an exchange.RaggedPiece, the reads as stored with their lengths.
          double-stranded   doubled index d < n: read d of reads_1; d >= n: read d - n of reads_2 (reads_1 when single-end),
                            rc = (d >= n) -- what ReadStore._gather_ragged(idx, 1, False) gives;
          -s                reads_1[i], rc = 0; for pairs reads_2[i] as stored beside them (the owner reads them reversed)."""
        sel = np.asarray(sel, dtype=np.int64)
        n_sel, n = len(sel), len(self.d1)
        rows_out, dev = self.one_length, self.collect_on_device
        L = int(self.store.r1.shape[1]) if rows_out else 0
        zeros = np.zeros(n_sel, np.uint8)
        Reads = self._dev.Reads
        if self.strand_specific:
            # plain read indices: reads_1[i] as stored and, for pairs, reads_2[i] as stored beside it (the owner reads it reversed)
            if dev:
                c1, o1 = Reads.collect(self.d1, None, sel, zeros)
                c2, o2 = Reads.collect(self.d2, None, sel, zeros) if self.paired else (None, None)
            elif rows_out or self.store.ragged:
                c1, o1, _rc, enc = self.store.gather_codes_ss(sel, 1)
                if enc != 1:
                    raise ValueError("GpuOps: -s on the N-rank path needs the reads stored as codes")
                c2, o2 = self.store.gather_codes_ss(sel, 2)[:2] if self.paired else (None, None)
            else:
                c1, o1 = self._host_take(self.store.r1, sel)
                c2, o2 = self._host_take(self.store.r2, sel) if self.paired else (None, None)
            if not rows_out:
                return exchange.RaggedPiece(c1, o1, zeros, c2, o2)
            rows = c1[:n_sel * L].reshape(n_sel, L)
            if self.paired:
                rows = np.concatenate([rows, c2[:n_sel * L].reshape(n_sel, L)], axis=1)
            return (np.ascontiguousarray(rows), zeros)
        second = sel >= n
        if dev:
            codes, off = Reads.collect(self.d1, self.d2, np.where(second, sel - n, sel), (second if self.paired else zeros))
            rc1 = second.astype(np.uint8)
        elif rows_out or (self.store.ragged and n_sel):
            codes, off, rc1, _enc = self.store.gather_codes(sel, 1)
        else:
            if n_sel > 1 and not bool((sel[1:] >= sel[:-1]).all()):
                raise ValueError("GpuOps.collect: the doubled indices of a piece come in ascending order")
            f = int(np.searchsorted(sel, n))
            src2 = self.store.r1 if not self.paired else self.store.r2
            (ca, oa), (cb, ob) = self._host_take(self.store.r1, sel[:f]), self._host_take(src2, sel[f:] - n)
            codes, off, rc1 = np.concatenate([ca, cb]), np.concatenate([oa, ob[1:] + oa[-1]]), second.astype(np.uint8)
        if not rows_out:
            return exchange.RaggedPiece(codes, off, rc1)
        return (codes[:n_sel * L].reshape(n_sel, L), rc1)

    def graph(self, part, name, pieces, K, paired):
        """one partition without unitigs (graph_batch declined: SHN_GRAPH_GPU=0, K > 31): the pieces merged into the global
        strand-doubled order -- the reference's file order -- and handed to the graph stage as codes + offsets"""
        from . import mbgraph_native
        rb = part["k1mer_bytes"][name]                     # the partition's k1-mer file as fixed-width rows
        merged = self._merge_pieces(pieces, self.strand_specific and paired)
        b1, o1, b2, o2, r1, r2 = self._ragged_args(merged, paired) if isinstance(merged, exchange.RaggedPiece) else self._rows_args(*merged, paired)
        singles, comps, _log = mbgraph_native.run_partition_arrays(rb if len(rb) else np.zeros(1, np.uint8), len(rb) // (K + 1), K, b1, o1, b2, o2,
                                                                   ctx=self.ctx, enc=1, rc1=r1, rc2=r2)
        return singles, comps

    def sparse_flow(self, flat, ids, seed):
        from .pipeline import _sparse_flow_with_ids
        return _sparse_flow_with_ids(self.ctx, flat, ids, seed)
