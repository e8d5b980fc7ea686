"""End-to-end hot path in memory: reads -> (K+1)-mer table -> contigs/partitions -> per-partition
multibridged graph -> sparse-flow transcripts -> merged FASTA.  Mirrors the order of shannon.py
(394-647) and run_MB_SF_fn.py (210-254) without the file round trips between stages (the
reference's --inMem hand-off); `shannon.py` at the repo root adds the CLI and the OUT/ file tree.
"""
import functools
import os
import sys
import time
import numpy as np
from . import _lib, device, extension_correction as ec, graph_intake as gi, kmers_for_component as kfc, mbgraph, mbgraph_native, sparse_flow, post
from .sflow_waves import WaveScheduler


class Result(object):
    """.partitions {name: record}, .final {name: sequence}, .all_reconstructed (the lines of all_reconstructed.fasta; joined from
    the partitions' texts on first use), .extension, .timings ..."""
    _texts = None

    @property
    def all_reconstructed(self):
        if self.__dict__.get("_lines") is None and self._texts is not None:
            lines = []
            for t in self._texts:
                lines += (t if isinstance(t, str) else bytes(t).decode()).splitlines(True)
            self.__dict__["_lines"] = lines
        return self.__dict__.get("_lines")

    @all_reconstructed.setter
    def all_reconstructed(self, lines):
        self.__dict__["_lines"] = lines


class PartitionRecord(dict):
    """Record of one partition: n_reads_routed, n_k1mers, reconstructed_fasta as plain entries; `singles`, `components`
    and `log` (the tables of mbgraph.output_components) are exported from the native graph object on first access."""

    def __init__(self, n_reads_routed, n_k1mers, graph):
        dict.__init__(self, n_reads_routed=n_reads_routed, n_k1mers=n_k1mers)
        self.graph = graph

    def __missing__(self, key):
        if key == "reconstructed_fasta" and getattr(self, "fasta_raw", None) is not None:
            dict.__setitem__(self, key, bytes(self.fasta_raw).decode())
            return dict.__getitem__(self, key)
        if key in ("singles", "components", "log") and self.graph is not None:
            singles, comps, log = self.graph.tables()
            dict.update(self, singles=singles, components=comps, log=log)
            return dict.__getitem__(self, key)
        raise KeyError(key)


_POOLS = {}


def _graph_pool(n_threads):
    """the host threads of the graph stage, kept from call to call: every thread owns a stream and device workspaces of its own
    (shn_thread_ctx) that go with it -- a fresh pool per step created and freed them sixteen times a step"""
    from concurrent.futures import ThreadPoolExecutor
    pool = _POOLS.get(n_threads)
    if pool is None:
        pool = _POOLS[n_threads] = ThreadPoolExecutor(max_workers=n_threads, thread_name_prefix="shn-graph")
    return pool


def n_kmer_nodes(rows, K):
    """#distinct K-mers among the k1-mer rows = len(Node.nodes) after loading (multibridging.py:383)."""
    s = set()
    for km, _ in rows:
        s.add(km[:-1])
        s.add(km[1:])
    return len(s)


def assemble(ctx, reads1, reads2=None, K=25, partition_size=500, min_weight=3, min_length=75, overload=2, penalty=5,
             sample="shannon", seed=0, double_stranded=True, part_vectors=None, timings=None, hits_factory=None,
             native_graph=True, kmer_hard_cutoff=1, filter_fp=False, in_disk_dir=None, kallisto_cutoff=None, kallisto_reads=None):
    """reads1/reads2: lists of strings or uint8 code matrices (reads2 None = single-end).
    min_weight = the reference's hyp_min_weight (--kmer_soft_cutoff, shannon.py:243-247, 457); kmer_hard_cutoff = its
    jellyfish_kmer_cutoff (--kmer_hard_cutoff, `jellyfish dump -L`, shannon.py:237-241, 441).  filter_fp: --filter_FP, in_disk_dir:
    --inDisk, kallisto_cutoff: --kallisto_cutoff, kallisto_reads: the resident sets it quantifies against, see assemble_resident.
    Returns Result with .partitions {name: dict}, .all_reconstructed (lines), .final {name: seq}."""
    T = timings if timings is not None else {}
    paired = reads2 is not None

    def tick(name, t0):
        T[name] = T.get(name, 0.0) + time.time() - t0

    t0 = time.time()
    mk = (lambda r: device.Reads.from_strings(ctx, r)) if isinstance(reads1[0], str) else (lambda r: device.Reads.from_codes(ctx, r))
    d1 = mk(reads1)
    d2 = mk(reads2) if paired else None
    store = kfc.ReadStore(reads1, reads2)
    tick("upload+pack", t0)
    return assemble_resident(ctx, d1, d2, store, K, partition_size, min_weight, min_length, overload, penalty, sample, seed,
                             double_stranded, part_vectors, T, hits_factory, native_graph, kmer_hard_cutoff=kmer_hard_cutoff, filter_fp=filter_fp,
                             in_disk_dir=in_disk_dir, kallisto_cutoff=kallisto_cutoff, kallisto_reads=kallisto_reads)


class _Step(object):
    """What the parts of one step share.  The inputs, as assemble_resident got them: ctx, d1, d2, store, K, sample, seed,
    double_stranded, ss, paired, native_graph, graph_threads, hits_factory and the options partition_size, overload, penalty,
    part_vectors, keep_partitioning, filter_fp, in_disk_dir, kallisto_cutoff, kallisto_reads.  R: the Result, T: its timings.  What
    the front leaves behind: res (the extension's result); the middle: part, names, unitigs, single_text, gpu_unitigs."""

    def __init__(self, T, **inputs):
        self.__dict__.update(inputs)
        self.T, self.R = T, Result()
        self.res = self.part = self.names = self.unitigs = self.single_text = None
        self.gpu_unitigs = False

    def tick(self, name, t0):
        self.T[name] = self.T.get(name, 0.0) + time.time() - t0


def assemble_resident(ctx, d1, d2, store, K=25, partition_size=500, min_weight=3, min_length=75, overload=2, penalty=5,
                      sample="shannon", seed=0, double_stranded=True, part_vectors=None, timings=None, hits_factory=None,
                      native_graph=True, graph_threads=None, keep_partitioning=False, defer_back=False, kmer_hard_cutoff=1, filter_fp=False,
                      in_disk_dir=None, kallisto_cutoff=None, kallisto_reads=None):
    """Same as assemble() with the reads already packed in HBM (d1/d2: device.Reads).  graph_threads: partitions whose
    graph stage may run concurrently on host threads.  keep_partitioning: leave the partition stage's tables (partition ->
    contigs, routed read indices) on the result as `.partitioning` (tests/test_fullsize_gpu.py reads them).  defer_back: run count,
    extension, partitioning / routing and the unitig batch now and return a function that does the rest (see `_back`);
    defer_back="early": only count and extension now, partitioning / routing / unitigs with the rest (see `_middle`).
    filter_fp: --filter_FP (shannon.py:170-195, run_MB_SF_fn.py:110, 272-277) -- once the last sparse flow is done, every partition's
    transcripts are held against the read pairs routed to it in one device call (filter_fp.filter_texts) and the merge gets the
    texts without the transcripts the pairs do not cover; a record then holds reconstructed_fasta (filtered), reconstructed_org_fasta
    and filter_log.  Paired-end input only, as in the reference (single-end: R.filter_fp_note says so, nothing is filtered).
    in_disk_dir: --inDisk (shannon.py:39-40) -- right behind the routing every partition `name` gets <in_disk_dir>/<sample>_<name>algo_input/
    with reads.fasta (pairs: reads_1.fasta + reads_2.fasta; all routed reads) and k1mer.dict, formatted on the device from the routes
    and the contig text (kfc.write_in_disk); R.in_disk = {name: {file: bytes}}, the time under timings["inDisk"].  None: nothing
    of this runs.
    kallisto_cutoff: --kallisto_cutoff C (shannon.py:309-318, 609-614, filter_kallisto.py) -- behind the merge every final transcript
    is quantified against ALL read pairs (abundance.apply: DESIGN.md 3.10) and stays only if est_counts / eff_length * L >= C;
    R.final is then the filtered set (a dict), R.final_before_kallisto what the merge gave, R.abundance the table (with the text of
    abundance.tsv under "tsv" and of rec_before_kallisto.fasta under "before"), the time under timings["abundance"].  Paired-end
    input only (single-end: R.kallisto_note says so, nothing is filtered).  None: nothing of this runs; works together with filter_fp.
    kallisto_reads: (reads_1, reads_2), the resident sets --kallisto_cutoff quantifies against where they are not d1 / d2 -- the
    reference hands kallisto the ORIGINAL read files while everything else sees Quorum's corrected ones (shannon.py:378, 612; --quorum:
    quorum.apply).  None: d1 / d2."""
    if graph_threads is None:
        # partition threads: all the CPUs a small allowance grants (a cgroup quota of 16 CPUs: 16), a quarter of a whole machine
        cpus = _lib.host_cpus()
        graph_threads = int(os.environ.get("SHN_GRAPH_THREADS", 0)) or (max(4, cpus) if cpus <= 32 else min(64, cpus // 4))
    if hits_factory is None:
        from . import graph_seeds
        hits_factory = graph_seeds.hits_factory(ctx)
    # double_stranded=False: -s / --ss / --strand_specific.  shannon.py:394-424 then leaves single-end reads as they are and
    # reverse-complements the second mates, without doubling; from :427 on double_stranded is False in BOTH modes, so only the read
    # set differs: forward counting (d2: its reverse complements), routes of plain read indices, pairs (R1[i], RC(R2[i])) in the
    # graph stage; process_concatenated_fasta (:596) gets the user's flag.
    S = _Step(timings if timings is not None else {}, ctx=ctx, d1=d1, d2=d2, store=store, K=K, sample=sample, seed=seed,
              double_stranded=double_stranded, ss=not double_stranded, paired=d2 is not None, native_graph=native_graph,
              graph_threads=graph_threads, hits_factory=hits_factory, partition_size=partition_size, overload=overload, penalty=penalty,
              part_vectors=part_vectors, keep_partitioning=keep_partitioning, filter_fp=filter_fp, in_disk_dir=in_disk_dir,
              kallisto_cutoff=kallisto_cutoff, kallisto_reads=kallisto_reads)
    _front(S, min_weight, min_length, kmer_hard_cutoff)
    if defer_back == "early":
        # the step cut behind the extension: count + extension now, everything else in the returned function (two batches in flight:
        # the halves are then 1.0 s and 0.5 s of a configs[2] step instead of 1.15 s and 0.35 s)
        def rest(bctx=None):
            _middle(S, bctx if bctx is not None else ctx)
            return _back(S, bctx)
        return rest
    _middle(S, ctx)
    if defer_back:
        return functools.partial(_back, S)
    return _back(S)


def _front(S, min_weight, min_length, kmer_hard_cutoff):
    """count + extension"""
    t0 = time.time()
    table = (device.count_k1mers_strand_specific(S.ctx, S.d1, S.d2, S.K + 1) if S.ss else
             device.count_k1mers(S.ctx, [S.d1, S.d2] if S.paired else [S.d1], S.K + 1, both_strands=True))
    if kmer_hard_cutoff > 1:
        # `jellyfish dump -L N` (shannon.py:441): k1-mers counted fewer than N times never reach k1mer.dict_org -- no seed, no
        # extension step, no weight of a later stage sees them (the seed threshold min_weight is another matter: a k1-mer below
        # THAT is still walked over, extension_correction.py:229-233)
        kept = table.filter_lower(kmer_hard_cutoff)
        table.close()
        table = kept
    S.R.n_k1mers, S.R.n_windows = len(table), table.total
    S.tick("count", t0)
    t0 = time.time()
    S.res = ec.run_correction(S.ctx, table, min_weight, min_length, S.partition_size, want_allowed=not S.native_graph, timings=S.T,
                              want_weight_arrays=S.in_disk_dir is not None)
    table.close()
    S.R.extension = S.res
    S.tick("extension", t0)


def _middle(S, mctx):
    """partition + route + the unitig batch, on context mctx: the caller's, or -- defer_back="early" -- the back half's (the
    extension's result is on the host or in device buffers whose producers have been waited for by then).  These stages use the
    stage workspaces of mctx: beside another context's counting / extension only on a context with a set of its own
    (device.Context(own_workspaces=True))."""
    S.gpu_unitigs = S.native_graph and S.K <= 31 and os.environ.get("SHN_GRAPH_GPU", "1") != "0"
    # (reads kept as code matrices + GPU unitigs: the graph stage names a partition's reads by their place in the routes on the
    # device, _back's rows mode -- the routed lists are then fetched per partition, only by the forms that want them on the host)
    rows_likely = S.gpu_unitigs and gi.rows_possible(S.store, S.d1, S.d2, S.paired, S.ss)
    R, res = S.R, S.res
    t0 = time.time()
    S.part = kfc.kmers_for_component(mctx, res, S.d1, S.d2, S.K, S.partition_size, S.overload, S.penalty, True, S.part_vectors,
                                     want_rows=not S.native_graph, timings=S.T, lazy_graph_inputs=S.gpu_unitigs, strand_specific=S.ss,
                                     lazy_routes=rows_likely)
    S.tick("partition+route", t0)
    if S.in_disk_dir is not None:
        t0 = time.time()
        R.in_disk = kfc.write_in_disk(mctx, S.part, S.d1, S.d2, S.K, S.ss, S.sample, S.in_disk_dir, res.k1mer_keys, res.k1mer_weights)
        S.tick("inDisk", t0)
    if S.keep_partitioning:
        R.partitioning = S.part
    R.partitions = {}
    # reconstructed_single_contigs.fasta: one text (the native merge takes texts); its lines only for the Python forms of the back half
    raw, ids = getattr(res, "contig_raw", None), getattr(res, "single_ids", None)
    if raw is not None and ids is not None and len(ids) == len(res.single_contigs) and len(raw[2]) == len(res.contigs):
        S.single_text = _lib.fasta_records(raw[0], raw[1], raw[2][np.asarray(ids, dtype=np.int64)], "Single_")      # (bytes, from the contig stage's buffer)
    else:
        S.single_text = "".join([">Single_%d\n%s\n" % (i, c) for i, c in enumerate(res.single_contigs)])
    S.names = list(S.part["new_components"])
    S.unitigs = None
    if S.gpu_unitigs and S.names:
        # the raw K-mer graphs of all partitions, contracted to unitigs in one batch on the GPU
        t0 = time.time()
        S.unitigs = mbgraph_native.Unitigs(mctx, [S.part["new_components"][nm] for nm in S.names], S.K, flat_text=S.part.get("flat_text"))
        S.tick("graph unitigs (GPU)", t0)


def _back(S, bctx=None):
    """the host-bound half of the step -- graph stage, sparse flow, merge -- on context bctx (default: the caller's): with
    defer_back the caller may run it on another thread and context while it starts the next batch's counting / extension
    (bench.py --overlap); everything it touches on the device from then on is its own (forked graph contexts, LP batches)"""
    ctx = bctx if bctx is not None else S.ctx
    env = os.environ.get
    check_rows, debug_parts = env("SHN_GRAPH_CHECK"), env("SHN_DEBUG_PARTS")
    sflow_native = S.native_graph and env("SHN_SFLOW_NATIVE", "1") != "0"
    # the sparse flow of a partition right behind its graph, on the same thread (one algorithm_SF.py process per component in
    # the reference, run_MB_SF_fn.py:242-250): the small partitions are through theirs while the largest is still at its graph
    sflow_beside = sflow_native and len(S.names) > 1 and S.graph_threads > 1 and env("SHN_SFLOW_BESIDE", "1") != "0"
    wave, waves_max = int(env("SHN_SFLOW_WAVE", 0)), int(env("SHN_SFLOW_WAVES_MAX", 0))
    post_native = env("SHN_POST_NATIVE", "1") != "0"
    # the merge takes every text as a piece the moment it exists (post.PostStream: lines, upload, fingerprints beside the graph
    # stage; the order-dependent rules at the end).  (--filter_FP: the merge must not see a text before the filter has; the texts
    # go to it in one piece at the end)
    stream = sflow_beside and post_native and env("SHN_POST_GPU", "1") != "0" and env("SHN_POST_STREAM", "1") != "0" and not S.filter_fp
    # reads kept as code matrices + GPU unitigs: partitions name their reads by rows (SHN_GRAPH_ROWS=0: gather them on the host).
    # What this adds to _middle's rows_likely: the unitigs exist (gpu_unitigs AND a partition to build them of), and both mates
    # have one length (the duplicate search on the device takes read sets of one length).
    rows_mode = (S.unitigs is not None and gi.rows_possible(S.store, S.d1, S.d2, S.paired, S.ss) and
                 (not S.paired or S.store.r2.shape[1] == S.store.r1.shape[1]))

    stage = _GraphStage(S, ctx, rows_mode, check_rows, debug_parts, sflow_beside, wave, waves_max, stream)
    results, wall = stage.run()
    busy = sum(sum(tt.values()) for _, tt in results) or 1.0
    for name, (rec, tt) in zip(S.names, results):
        for k_, v in tt.items():                                      # wall time of the stage, split like the thread time
            S.T[k_] = S.T.get(k_, 0.0) + v * wall / busy
        S.R.partitions[name] = rec
    t0 = time.time()
    texts = _native_texts(S, ctx, sflow_beside) if sflow_native else _python_texts(S, ctx)
    S.tick("sparse flow", t0)
    if S.filter_fp:
        texts = apply_filter_fp(S, ctx, texts)
    t0 = time.time()
    merge(S, ctx, texts, stage.complete_stream(), sflow_native and post_native)
    S.tick("post", t0)
    apply_kallisto(S, ctx)
    S.R.timings = S.T
    return S.R


class _GraphStage(object):
    """The graph stage of one step: every partition's multibridged graph on the pool's threads and -- sflow_beside -- its sparse
    flow right behind it on the same thread, the texts going to the merge stream as pieces (piece 0 = the single contigs, piece
    1 + i = partition i)."""

    def __init__(self, S, ctx, rows_mode, check_rows, debug_parts, sflow_beside, wave, waves_max, stream):
        self.S, self.ctx, self.rows_mode, self.check_rows, self.sflow_beside = S, ctx, rows_mode, check_rows, sflow_beside
        self.index = {nm: i for i, nm in enumerate(S.names)}
        self.timeline = {} if debug_parts else None
        self.forms = {gi.ROWS_BY_PLACE: self._rows, gi.ROWS: self._rows, gi.GATHERED: self._gathered, gi.PYTHON: self._python}
        # (the few partitions with the most reads -- their graphs take longest -- each run their own sparse flow; all the others go
        # through calls over many of them, in waves: a call's cost is its dependent LP rounds, and a hundred small calls keep sixteen
        # threads waiting on a hundred times as many tiny batches)
        n_routed = {nm: len(S.part["routes"][nm]) for nm in S.names}
        big_cut = max(n_routed.values()) // 4 if S.names else 0
        # (at most four: when the partitions are of one size -- a component cut by gpmetis into a hundred parts -- "a quarter of the
        # largest" holds for all of them, and four hundred calls of their own were 225,000 tiny LP batches per step at --config 2p)
        self.big = set(sorted((nm for nm in S.names if n_routed[nm] >= max(1, big_cut)), key=lambda nm: -n_routed[nm])[:4]) if sflow_beside else set()
        small = [nm for nm in S.names if nm not in self.big]
        # With ONE call behind the last graph a hundred partitions of one size (bench.py --config 2p: 401 parts of two gpmetis
        # components) left all their sparse flow -- 890 dependent LP rounds, 1.3 s -- to be done after the graph stage with fifteen
        # threads idle.  (A component's answer does not depend on its call: its random costs are numbered inside its own graph.)  A
        # tenth of the partitions per wave, four waves in flight: a wave lasts as long as its ~800 dependent rounds whatever its size
        # (tools/sflow_waves_r06.sh at 2p, per step: a sixth / 3 in flight 4.49-4.61 s, 40 / 4: 4.31-4.34, 32 / 5: 4.37-4.45, 100 / 3: 4.71).
        self.waves = WaveScheduler(small, max(16, wave or (len(small) + 9) // 10), max(1, waves_max or 4),
                                   lambda names: self._sparse_flow(names, [self.waves.records[nm] for nm in names]))
        self.pstream, self.ps_failed, self.post_futs = None, [], []
        if stream:
            try:
                # room for the merge's text on the device: the transcripts are paths through the contigs' graph -- a few times the
                # accepted contigs' text (both strands, isoforms sharing exons); a text that outgrows it falls back to the one-piece merge
                raw = getattr(S.res, "contig_raw", None)
                cbytes = int(len(raw[0])) if raw is not None else sum(len(c) for c in S.res.contigs)
                self.pstream = post.PostStream(ctx, capacity=min(2 << 30, max(64 << 20, 8 * cbytes + len(S.single_text))))
            except _lib.ShannonError:
                self.pstream = None

    def post_piece(self, index, text):
        if self.pstream is None or self.ps_failed:
            return
        try:
            self.pstream.add(index, text)
        except _lib.ShannonError as ex:                   # (no room, a last line without its end, ...: the merge in one piece then)
            self.ps_failed.append(str(ex))

    def complete_stream(self):
        """the merge stream if it holds every piece; else None, the stream closed"""
        if self.pstream is not None and (self.ps_failed or len(self.pstream.keep) != len(self.S.names) + 1):
            self.pstream.close()
            self.pstream = None
        return self.pstream

    def _sparse_flow(self, names, recs):
        return mbgraph_native.sparse_flow_native(self.ctx, [rec.graph for rec in recs], ["%s_%s" % (self.S.sample, nm) for nm in names],
                                                 self.S.seed, raw=True, threaded=True)

    def run(self):
        """-> ([(record, thread timings)] in `names` order, the stage's wall time)"""
        S = self.S
        self.t0 = time.time()
        results, futs = [], {}
        try:
            if S.native_graph and len(S.names) > 1 and S.graph_threads > 1:
                # partitions are independent (one multibridging process each in the reference, run_MB_SF_fn.py:219-253): the
                # native stage releases the GIL, its GPU sections take turns
                pool = _graph_pool(S.graph_threads)
                # the partitions with the most routed reads first (the reference's size-sorted job list, shannon.py:546-551)
                by_size = sorted(S.names, key=lambda nm: -len(S.part["routes"][nm]))
                futs = {nm: pool.submit(self.one_partition, nm) for nm in by_size}
                if self.pstream is not None:
                    self.post_futs.append(pool.submit(self.post_piece, 0, S.single_text))
                results = [futs[nm].result() for nm in S.names]
                for f_ in list(self.post_futs):
                    f_.result()
            else:
                for nm in S.names:
                    results.append(self.one_partition(nm))
        except BaseException:
            # a partition failed: nothing of this step may still run on the pool's threads when the inputs go away below
            if futs:
                import concurrent.futures as _cf
                for f_ in list(futs.values()) + list(self.post_futs):
                    f_.cancel()
                _cf.wait(list(futs.values()) + list(self.post_futs))
            if self.pstream is not None:
                self.pstream.close()
            # ... and the graphs already built go back now (device + host memory), not when the collector finds them
            built = [f.result()[0] for f in futs.values() if f.done() and not f.cancelled() and f.exception() is None] or [r[0] for r in results]
            for rec in built:
                g = getattr(rec, "graph", None)
                if g is not None:
                    g.close()
            raise
        finally:
            if S.unitigs is not None:
                S.unitigs.close()
        wall = time.time() - self.t0
        if self.timeline is not None:
            for nm, (a, b, tt_, nr) in sorted(self.timeline.items(), key=lambda kv: -kv[1][1])[:12]:
                sys.stderr.write("[parts] %-16s start %6.2f end %6.2f  routed %8d  %s\n" % (nm, a, b, nr, {k: round(v, 2) for k, v in tt_.items()}))
            sys.stderr.write("[parts] stage wall %.2f s, %d partitions, %d threads, %.2f thread-seconds\n"
                             % (wall, len(S.names), S.graph_threads, sum(b - a for a, b, _t, _n in self.timeline.values())))
        return results, wall

    def one_partition(self, name):
        """multibridged graph of one partition (multibridging.main for `name`) and, sflow_beside, its sparse flow: a big partition's
        own call, a small one's with the wave this thread starts, if it starts one; returns its record + timings"""
        rec, tt = self.intake(name)
        if self.sflow_beside and getattr(rec, "graph", None) is not None:
            t1 = time.time()
            if name in self.big:
                rec.fasta_raw = self._sparse_flow([name], [rec])[0]
                self.post_piece(1 + self.index[name], rec.fasta_raw)
            else:
                wave = self.waves.finished(name, rec)
                for nm, txt in wave:
                    self.waves.records[nm].fasta_raw = txt
                if wave and self.pstream is not None:               # (their pieces on whatever threads are free)
                    pool = _graph_pool(self.S.graph_threads)
                    self.post_futs.extend([pool.submit(self.post_piece, 1 + self.index[nm], txt) for nm, txt in wave])
            tt["sparse flow"] = time.time() - t1
        if self.timeline is not None:
            self.timeline[name] = (tt.pop("_t0") - self.t0, time.time() - self.t0, dict(tt), len(self.S.part["routes"][name]))
        else:
            tt.pop("_t0", None)
        return rec, tt

    def intake(self, name):
        """the partition's reads, capped, to the graph stage in the form gi.choose_form names -> (record, timings)"""
        S, part = self.S, self.S.part
        tt = {"_t0": time.time()}
        n_kmers = S.unitigs.n_kmers(self.index[name]) if S.unitigs is not None else part["n_kmer_nodes"][name]
        cutoff = 10 * n_kmers + 1                                    # multibridging.py:26-30, 385-391
        rts, rdev = part["routes"][name], part.get("routes_dev")
        on_device = rdev is not None and name in rdev[1] and isinstance(rts, kfc.RouteView)
        n = min(len(rts), cutoff)
        form = gi.choose_form(S.native_graph, self.rows_mode, on_device, self.check_rows, S.ss, n)
        # (by place: the count is all the host needs)
        idx = n if form == gi.ROWS_BY_PLACE else (rts[:cutoff] if n else np.zeros(0, np.uint32))
        return self.forms[form](name, idx, tt), tt

    def _rows(self, name, idx, tt):
        """the reads named by their rows -- idx: an index array or, by place, the length of the prefix of the partition's routes on
        the device: distinct reads found on the device, their text decoded from the host matrices"""
        S, part = self.S, self.S.part
        rdev = part.get("routes_dev")                             # (the same list, still on the device: idx is a prefix of the partition's)
        routes = (rdev[0], rdev[1][name]) if (rdev is not None and name in rdev[1]) else None
        sel = idx if np.ndim(idx) == 0 else np.asarray(idx, dtype=np.uint32)

        def run(rb):
            return mbgraph_native.run_partition_rows(self.ctx, S.unitigs, self.index[name], S.d1, S.d2, S.store.r1, S.store.r2 if S.paired else None,
                                                     sel, rb if (rb is not None and len(rb)) else None, 0 if rb is None else len(rb) // (S.K + 1),
                                                     routes=routes)
        gh = gi.with_k1mer_rows(run, part, name, gi.k1mer_rows(part, name) if self.check_rows else None)
        tt["graph"] = time.time() - tt["_t0"]
        return PartitionRecord(len(part["routes"][name]), part["n_k1mer_rows"][name], gh)

    def _gathered(self, name, idx, tt):
        """the reads' codes gathered on the host, with strand flags (-s: reads_1[i] and RC(reads_2[i]))"""
        S, part, store = self.S, self.S.part, self.S.store
        if S.ss:
            b1, o1, rc1, enc = store.gather_codes_ss(idx, 1)
            b2, o2, rc2, _e = store.gather_codes_ss(idx, 2) if S.paired else (None, None, None, enc)
            assert _e == enc, "both mates' reads must be stored the same way (strings, code matrices or codes + offsets)"
        else:
            b1, o1, rc1, enc = store.gather_codes(idx, 1)
            if S.paired and rc1 is not None:
                # the second mates are the same stored rows read on the other strand (shannon.py:413-424)
                b2, o2, rc2 = b1, o1, (1 - rc1).astype(np.uint8)
            else:
                b2, o2, rc2, _e = store.gather_codes(idx, 2) if S.paired else (None, None, None, enc)
        tt["materialize reads"] = time.time() - tt["_t0"]
        t0 = time.time()
        # with GPU unitigs the k1-mer rows are only needed for a partition holding a cycle of condensable edges (built by
        # the sequential code) and for the development check SHN_GRAPH_CHECK=1
        given = gi.k1mer_rows(part, name) if (S.unitigs is None or self.check_rows) else None
        resident = (S.d1, S.d2, np.asarray(idx, dtype=np.uint32)) if (enc == 1 and len(idx) and not S.ss and not getattr(store, "ragged", False)) else None     # code matrices resident on the device

        def run(rb):
            return mbgraph_native.run_partition_handle(None if rb is None else (rb if len(rb) else np.zeros(1, np.uint8)),
                                                       0 if rb is None else len(rb) // (S.K + 1), S.K, b1, o1, b2, o2, ctx=self.ctx, enc=enc,
                                                       rc1=rc1, rc2=rc2, unitigs=S.unitigs, part=self.index[name], resident=resident)
        gh = gi.with_k1mer_rows(run, part, name, given)
        if enc == 1 and not S.ss:
            store.release(b1)
            if b2 is not None and b2 is not b1:
                store.release(b2)
        tt["graph"] = time.time() - t0
        return PartitionRecord(len(part["routes"][name]), part["n_k1mer_rows"][name], gh)

    def _python(self, name, idx, tt):
        """the Python mirror of the graph stage (mbgraph.run_partition) over the reads as strings"""
        S, part, store = self.S, self.S.part, self.S.store
        rows = part["k1mers"][name]
        if S.ss:
            r1 = [store._get(store.r1, int(d)) for d in idx]
            reads = [r1, [store._rc(store._get(store.r2, int(d))) for d in idx]] if S.paired else [r1]
        else:
            r1 = [store.mate1(int(d)) for d in idx]
            reads = [r1, [store.mate2(int(d)) for d in idx]] if S.paired else [r1]
        tt["materialize reads"] = time.time() - tt["_t0"]
        t0 = time.time()
        g, singles, comps = mbgraph.run_partition(rows, reads, S.K, S.paired, S.hits_factory)
        tt["graph"] = time.time() - t0
        return {"n_reads_routed": len(part["routes"][name]), "n_k1mers": len(rows), "singles": singles, "components": comps, "log": g.log}


def _native_texts(S, ctx, sflow_beside):
    """every partition's transcripts from the native sparse-flow stage (shn_sparse_flow): what the graph stage's threads left, or
    all components of all partitions in one call; the graphs stay native objects (exported to Python tables only if somebody asks
    a PartitionRecord for them)"""
    recs = [S.R.partitions[nm] for nm in S.names]
    if sflow_beside and all(getattr(rec, "fasta_raw", None) is not None for rec in recs):
        return [rec.fasta_raw for rec in recs]
    texts = mbgraph_native.sparse_flow_native(ctx, [rec.graph for rec in recs], ["%s_%s" % (S.sample, nm) for nm in S.names], S.seed, raw=True)
    for rec, txt in zip(recs, texts):
        rec.fasta_raw = txt                 # decoded when somebody reads ["reconstructed_fasta"]
    return texts


def _python_texts(S, ctx):
    """every partition's transcripts from the Python form of the sparse flow, over the tables of the records"""
    jobs = [(name, S.R.partitions[name]["singles"], S.R.partitions[name]["components"]) for name in S.names]
    flat = [(nd["nodes"], nd["edges"], nd["paths"]) for _, _, comps in jobs for nd in comps]
    # component c of partition p uses RNG stream id = its index within the partition (as one
    # algorithm_SF.py process per component, run_MB_SF_fn.py:242-250)
    ids = [c for _, _, comps in jobs for c in range(len(comps))]
    trs_flat = _sparse_flow_with_ids(ctx, flat, ids, S.seed) if flat else []
    k, texts = 0, []
    for name, singles, comps in jobs:
        sname = "%s_%s" % (S.sample, name)
        txt = ""
        for c in range(len(comps)):
            txt += sparse_flow.fasta_records(sname, str(c), trs_flat[k])
            k += 1
        txt += sparse_flow.single_nodes_fasta(sname, singles)
        S.R.partitions[name]["reconstructed_fasta"] = txt
        texts.append(txt)
    return texts


def apply_filter_fp(S, fctx, texts):
    """--filter_FP over the partitions' texts (in the order of `names` = the partition ids of the routes); sets the three
    entries of every record and returns the filtered texts"""
    R, part, names = S.R, S.part, S.names
    t0 = time.time()
    if not S.paired or S.d1 is None or S.d2 is None:
        R.filter_fp_note = ("--filter_FP: single-end input -- the reference sets the flag only for paired-end runs "
                            "(run_MB_SF_fn.py:110); nothing filtered")
        return texts
    from . import filter_fp as ffp
    stats = {}
    rdev = part.get("routes_dev")
    if rdev is not None:
        routes = rdev[0]
    else:                                   # (routes on the host only: one list of (partition, index) pairs)
        per = [np.asarray(part["routes"][nm], dtype=np.uint32) for nm in names]
        routes = (np.repeat(np.arange(len(names), dtype=np.uint32), [len(x) for x in per]),
                  np.concatenate(per) if per else np.zeros(0, np.uint32))
    out = ffp.filter_texts(fctx, texts, S.d1, S.d2, routes, S.ss, stats=stats)
    kept = []
    for name, org, (txt, log_) in zip(names, texts, out):
        rec = R.partitions[name]
        dict.__setitem__(rec, "reconstructed_org_fasta", org if isinstance(org, str) else bytes(org).decode())
        dict.__setitem__(rec, "reconstructed_fasta", txt)
        dict.__setitem__(rec, "filter_log", log_)
        if getattr(rec, "fasta_raw", None) is not None:
            rec.fasta_raw = txt.encode()
        kept.append(txt.encode())
    R.filter_fp_stats = stats
    S.tick("filter_FP", t0)
    return kept


def merge(S, ctx, texts, pstream, native):
    """all_reconstructed.fasta (the single contigs, then the partitions' texts) -> R.final: the streamed merge where pstream holds
    every piece, else -- native -- the native merge in one piece, else the Python form (post.finalize) over the lines"""
    R = S.R
    R._texts = [S.single_text] + list(texts)
    if native:
        try:
            R.final = (pstream.finish(S.double_stranded, lazy=True) if pstream is not None else
                       post.finalize_texts(R._texts, S.double_stranded, ctx=ctx, lazy=True))
            return
        except _lib.ShannonError as ex:
            if "non-ACGT" not in str(ex) and "empty line" not in str(ex):
                raise
            sys.stderr.write("[shannon_amd] the native merge declined the transcripts (%s): merging with the Python form "
                             "(post.finalize), about 2x slower\n" % str(ex)[:200])
            S.T["post fell back to python"] = S.T.get("post fell back to python", 0) + 1
    R.final = post.finalize(R.all_reconstructed, S.double_stranded)


def apply_kallisto(S, kctx):
    """--kallisto_cutoff on R.final (the merge's result)"""
    R = S.R
    if S.kallisto_cutoff is None:
        return
    k1, k2 = S.kallisto_reads if S.kallisto_reads is not None else (S.d1, S.d2)
    if not S.paired or k1 is None or k2 is None:
        R.kallisto_note = ("--kallisto_cutoff: single-end input is not built (the reference runs kallisto --single -l 200 -s 20, "
                           "filter_kallisto.py:25); nothing filtered")
        return
    t0 = time.time()
    from . import abundance
    kept, table, tsv, before = abundance.apply(kctx, R.final, k1, k2, S.ss, S.kallisto_cutoff)
    table["tsv"], table["before"] = tsv, before
    R.final_before_kallisto, R.final, R.abundance = R.final, kept, table
    S.tick("abundance", t0)


def _sparse_flow_with_ids(ctx, components, comp_ids, seed):
    gens = [sparse_flow.component_coroutine(nd, ed, pt, cid) for (nd, ed, pt), cid in zip(components, comp_ids)]
    results = [None] * len(gens)
    pending = {}
    for c, g in enumerate(gens):
        try:
            pending[c] = next(g)
        except StopIteration as stop:
            results[c] = stop.value
    while pending:
        order = sorted(pending)
        xs = sparse_flow.solve_batch(ctx, [pending[c] for c in order], seed)
        nxt = {}
        for c, x in zip(order, xs):
            try:
                nxt[c] = gens[c].send(sparse_flow.finish(pending[c], x))
            except StopIteration as stop:
                results[c] = stop.value
        pending = nxt
    return results
