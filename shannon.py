#!/usr/bin/env python3
"""shannon.py -- command line of the MI355X-native Shannon hot path.

Keeps the reference CLI (sreeramkannan/Shannon shannon.py:145-321) for the flags that drive the
hot path and produces the same products: OUT/shannon.fasta, OUT/log.txt, OUT/TEMP/ (shannon.py:
634-638).  Flags that only select external tools outside the path (--compare) are accepted
and reported as not built.

    python shannon.py -o OUT --single reads.fasta            [-K 25] [--partition 500]
    python shannon.py -o OUT --left r1.fasta --right r2.fasta [-s / --ss / --strand_specific]
    ... [--kmer_hard_cutoff N]   k1-mers counted fewer than N times are dropped (`jellyfish dump -L N`, shannon.py:237-241, 441; default 1)
    ... [--kmer_soft_cutoff N]   hyp_min_weight: seed threshold + hyperbola of the contig stage (shannon.py:243-247, 457; default 3)
    ... [--inDisk]               the reference's default mode (shannon.py:39-40): per partition TEMP/<sample>_<name>algo_input/ holds reads.fasta
                                 (pairs: reads_1.fasta + reads_2.fasta) and k1mer.dict, the hand-off to multibridging.py / algorithm_SF.py,
                                 written from the device (one-process runs)
    ... [--filter_FP]            paired-end runs: after a partition's sparse flow its read pairs are mapped back onto its transcripts and a
                                 transcript stays only if the pairs cover 90 % of its bases (shannon.py:170-195, filter_FP.py; the aligner is
                                 the rule of DESIGN.md "filter_FP", run on the GPU); per partition TEMP/<sample>_<name>algo_output/ then holds
                                 reconstructed.fasta (filtered), reconstructed_org.fasta and rec.log
                                 (with -p N as well: the ranks' coverage is merged at the partitions' owners, the result is the one-process one)
    ... [--kallisto_cutoff C]    FASTQ input only (a first read file whose name ends in `q`, or --fastq; --fasta turns it off), as in the
                                 reference (shannon.py:289-318): the final transcripts are quantified against all read pairs and one stays
                                 only if est_counts / eff_length * L >= C (shannon.py:609-614, filter_kallisto.py:8-21; kallisto itself is
                                 the rule of DESIGN.md 3.10, run on the GPU); TEMP/<sample>_allalgo_output/ then holds
                                 rec_before_kallisto.fasta and kallisto/abundance.tsv, OUT/shannon.fasta the filtered transcripts
                                 (paired-end, one-process runs; otherwise a NOTE and nothing is filtered)
    ... [--quorum]               FASTQ input only (the same gate as --kallisto_cutoff): the reads are error-corrected with their quality
                                 scores before anything is counted, as the reference does for every FASTQ run (shannon.py:289-299, 385-391;
                                 Quorum itself is the rule of DESIGN.md 3.11, run on the GPU).  Opt-in here: without the flag a FASTQ run is
                                 what it was.  TEMP/corrected_reads_1.fa + corrected_reads_2.fa (single-end: corrected_reads.fa) hold the
                                 corrected reads; everything downstream sees them, --kallisto_cutoff the original ones (shannon.py:378, 612)
                                 (one-process runs; with -p N / --gpus N a NOTE and nothing is corrected)
    python shannon.py -o OUT --left r1.fasta --right r2.fasta -p 8        # one rank per GPU (the reference's -p nJobs, shannon.py:527-566)

-p N / --gpus N: the reference fans its partitions out over nJobs processes (GNU parallel, shannon.py:527-566); here the N jobs
are N ranks, one per GPU of the node (torch.distributed over RCCL): this process -- which has made no GPU call -- starts them as
children (torch.distributed.run on 127.0.0.1) and returns their exit code; every rank ingests its slice of the reads, the k1-mer
buckets are exchanged once, partitions are dealt to the ranks, rank 0 merges and writes OUT/ (shannon_amd/distributed.py).
-p is capped at the number of GPUs the node shows (one GPU: the one-process path, partitions concurrently on host threads).
-p N takes reads of any lengths, trimmed reads and mates of two lengths included, as the one-process path does.
"""
import os, sys, time, json

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
VERSION = "0.1.0-mi355x"


def usage():
    print(__doc__)


def read_fasta(path):
    """2-line or multi-line FASTA/FASTQ (plain or .gz) -> list of sequences (upper case kept as in the file)."""
    import gzip
    seqs = []
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        first = f.readline()
        f.seek(0)
        if first.startswith("@"):
            lines = f.read().splitlines()
            return [lines[i + 1].strip() for i in range(0, len(lines) - 1, 4)]
        cur = None
        for line in f:
            if line.startswith(">"):
                if cur is not None:
                    seqs.append(cur)
                cur = ""
            elif cur is not None:
                cur += line.strip()
        if cur is not None:
            seqs.append(cur)
    return seqs


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, args):
    """start the n ranks as fresh child processes (torch.distributed.run, rendezvous on 127.0.0.1) and hand their exit code on;
    this parent makes no GPU call"""
    import subprocess
    env = dict(os.environ, SHN_CLI_RANKS="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL between processes needs it on this stack
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(args)
    return subprocess.call(cmd, env=env, cwd=os.getcwd())


def rank_main(out_dir, reads, K, partition_size, min_weight, min_length, double_stranded, ignored, noted, kmer_hard_cutoff=1, filter_fp=False):
    """one rank of an N-rank run: its slice of the reads (by index, contiguous), shannon_amd.distributed.assemble_distributed,
    rank 0 writes OUT/ (shannon.fasta, log.txt, TEMP/<sample>_allalgo_output/all_reconstructed.fasta and the contig files; the
    per-partition graph files stay with the ranks that owned the partitions; with --filter_FP the three files of every partition,
    TEMP/<sample>_<name>algo_output/reconstructed.fasta, reconstructed_org.fasta and rec.log)"""
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("SHN_CLI_BACKEND") == "gloo"
    if os.environ.get("SHN_CLI_LAUNCH_PROBE"):
        # CPU test of the launch (tests/test_cli_launcher.py): the ranks meet over gloo, rank 0 says what the launch resolved to;
        # nothing touches the GPU
        dist.init_process_group("gloo")
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        if rank == 0:
            print("launch probe: %d ranks met, K=%d, partition=%d, double_stranded=%s, reads=%s, out=%s, min_weight=%d, kmer_hard_cutoff=%d"
                  % (int(one.item()), K, partition_size, double_stranded, ",".join(os.path.basename(p) for p in reads), out_dir, min_weight,
                     kmer_hard_cutoff))
        dist.destroy_process_group()
        return 0
    dev_index = 0 if share else local
    torch.cuda.set_device(dev_index)
    if share:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
    import shannon_amd
    if os.environ.get("SHN_MALLOC_TUNE", "1") != "0":
        shannon_amd.malloc_tune()
    from shannon_amd import device, distributed, exchange, kmers_for_component as kfc, _lib
    sample = os.path.basename(os.path.normpath(out_dir))
    temp = os.path.join(out_dir, "TEMP")
    log = None
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        os.makedirs(temp)
        log = open(os.path.join(out_dir, "log.txt"), "w")

    def say(msg):
        if rank == 0:
            line = "%s: %s" % (time.asctime(), msg)
            print(line)
            log.write(line + "\n")
    say("Starting Shannon run (MI355X hot path %s, %d ranks)" % (VERSION, world))
    if ignored:
        say("WARNING: flags outside the hot path ignored: " + " ".join(ignored))
    for msg in noted:
        say("NOTE: " + msg)
    ctx = device.Context(dev_index)
    T = {}
    t0 = time.time()
    paired = len(reads) == 2
    # every rank ingests ITS share of the files (by bytes; distributed.ingest_rank_slice) -- the records [n r / W, n (r + 1) / W) of the
    # job, in the files' order, reads of different lengths included; files that cannot be shared out that way (.gz, multi-line
    # FASTA) are read whole on every rank as before
    ing_stats = {}
    cdev = exchange.coll_device(torch.device("cuda", dev_index), None)
    sl = distributed.ingest_rank_slice(reads, rank, world, None, cdev, stats=ing_stats, ragged=True)
    if sl is not None:
        qs, n = list(sl[0]), sl[1]
        lo, hi = rank * n // world, (rank + 1) * n // world
    else:
        mats = []
        for p in reads:
            try:
                _d, r = device.Reads.ingest(None, p)                # (the host codes only: the rank uploads its own slice below)
            except _lib.ShannonError as ex:
                if "unsupported" not in str(ex):
                    raise
                seqs = read_fasta(p)
                code = np.full(256, 4, np.uint8)
                for j, c in enumerate(b"ACGT"):
                    code[c] = j
                off = np.zeros(len(seqs) + 1, dtype=np.uint64)
                off[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
                flat = code[np.frombuffer("".join(seqs).encode(), dtype=np.uint8)]
                L = len(seqs[0]) if seqs else 0
                if all(len(x) == L for x in seqs):
                    r = flat.reshape(len(seqs), L) if seqs else np.zeros((0, 1), np.uint8)
                else:
                    r = device.RaggedCodes(flat, off)
            mats.append(r)
        if paired and len(mats[0]) != len(mats[1]):
            say("ERROR: --left and --right hold different numbers of reads")
            return 2
        n = len(mats[0])
        lo, hi = rank * n // world, (rank + 1) * n // world
        qs = [m[lo:hi] if isinstance(m, device.RaggedCodes) else np.ascontiguousarray(m[lo:hi]) for m in mats]
        del mats
    if any(isinstance(q, device.RaggedCodes) for q in qs):         # one kind of store for both mates
        qs = [q if isinstance(q, device.RaggedCodes) else device.RaggedCodes.from_matrix(q) for q in qs]
    q1, q2 = qs[0], (qs[1] if paired else None)
    T["ingest path"] = "byte share of the files" if sl is not None else "whole files on every rank"
    if ing_stats:
        T["ingest bytes scanned by this rank"] = ing_stats["bytes_scanned"]
        T["ingest bytes of the files"] = ing_stats["file_bytes"]

    def resident(q):
        return device.Reads.from_ragged(ctx, q.codes, q.off) if isinstance(q, device.RaggedCodes) else device.Reads.from_codes(ctx, q)
    d1 = resident(q1)
    d2 = resident(q2) if paired else None
    T["ingest"] = time.time() - t0
    bases = torch.tensor([q1.total_bases if isinstance(q1, device.RaggedCodes) else q1.size], dtype=torch.int64, device=cdev)
    dist.all_reduce(bases)
    say("Processed No of reads:%d, Avg. Read length: %.2f (every rank holds a slice of %d of them)" % (n, int(bases.item()) / max(1, n), hi - lo))
    ops = distributed.GpuOps(ctx, d1, d2, kfc.ReadStore(q1, q2), K)
    res = distributed.assemble_distributed(ops, K, partition_size, sample, 0, timings=T, double_stranded=double_stranded,
                                           min_weight=min_weight, min_length=min_length, kmer_hard_cutoff=kmer_hard_cutoff, filter_fp=filter_fp)
    T["collect path"] = getattr(ops, "collect_path", "host")
    rc = 0
    if rank == 0:
        say("%d K-mers loaded; %d contigs; %d partitions" % (res["n_k1mers"], len(res["contigs"]), len(res["partitions"])))
        ai = os.path.join(temp, sample + "_algo_input")
        os.makedirs(ai)
        with open(os.path.join(ai, "k1mer.dict_contig"), "w") as f:
            f.write("".join(c + "\n" for c in res["contigs"]))
        if "filter_logs" in res:
            # filter_FP.py:52-55: the filtered transcripts take the place of reconstructed.fasta, the sparse flow's stay beside them
            for name in res["partitions"]:
                base = os.path.join(temp, "%s_%s" % (sample, name))
                os.makedirs(base + "algo_output")
                kept, org = res["partitions"][name], res["partitions_org"][name]
                open(os.path.join(base + "algo_output", "reconstructed.fasta"), "w").write(kept)
                open(os.path.join(base + "algo_output", "reconstructed_org.fasta"), "w").write(org)
                open(os.path.join(base + "algo_output", "rec.log"), "w").write(res["filter_logs"][name])
                say("%s has completed: %d transcripts, %d after --filter_FP" % (base, org.count(">"), kept.count(">")))
            st = res["filter_fp_stats"]
            say("--filter_FP: %d of %d routed fragments placed as concordant pairs; %d of %d transcripts kept"
                % (st.get("placed", 0), st.get("routes", 0), st.get("kept", 0), st.get("transcripts", 0)))
        elif "filter_fp_note" in res:
            say("NOTE: " + res["filter_fp_note"])
        alld = os.path.join(temp, sample + "_allalgo_output")
        os.makedirs(alld)
        with open(os.path.join(alld, "all_reconstructed.fasta"), "w") as f:
            for name in res["partitions"]:
                f.write(res["partitions"][name])
        final = res["final"]
        if hasattr(final, "fasta"):
            with open(os.path.join(out_dir, "shannon.fasta"), "wb") as f:
                f.write(final.fasta())
        else:
            with open(os.path.join(out_dir, "shannon.fasta"), "w") as f:
                for name, seq in final.items():
                    f.write(">%s\n%s\n" % (name, seq))
        say("All partitions completed: %d transcripts reconstructed" % len(final))
        say("stage seconds (rank 0): " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in T.items()}))
        log.close()
        print("-------------------------------------------------")
        print(time.asctime() + ": Shannon Run Completed")
        print("-------------------------------------------------")
    dist.barrier()
    d1.close()
    if d2 is not None:
        d2.close()
    ctx.close()
    dist.destroy_process_group()
    return rc


class Options(object):
    """what the command line asked for (parse_args)"""


def parse_args(argv):
    """the flags of argv (argv[0] = the program) -> Options, or the exit code of a run that ends with the parsing (--help,
    --version, a flag without its value).  Prints the reference's OPTIONS lines; touches neither the GPU nor the file system."""
    K, partition_size, nJobs = 24, 500, 1                     # shannon.py:58,65,67
    out_dir, reads, double_stranded = None, [], True
    min_weight, min_length = 3, 75                            # hyp_min_weight, hyp_min_length: shannon.py:56-57
    kmer_hard_cutoff = 1                                      # jellyfish_kmer_cutoff: shannon.py:55
    i = 1
    ignored, noted = [], []
    takes_value = ("-o", "--single", "--left", "--right", "-K", "-p", "--gpus", "--partition", "--kmer_hard_cutoff", "--kmer_soft_cutoff", "--kallisto_cutoff")
    n_gpus = 0
    filter_fp = False
    in_disk = False
    fastq_flag, fasta_flag, kallisto_arg, kallisto_at = False, False, None, 0
    quorum_flag, quorum_at, quorum_i, kallisto_i = False, 0, 0, 0
    while i < len(argv):
        a = argv[i]
        if a in takes_value and i + 1 >= len(argv):
            print("ERROR: %s needs a value" % a)
            return 2
        if a in ("--help", "-h"):
            usage(); return 0
        if a == "--version":
            print(VERSION); return 0
        if a == "-o":
            out_dir = argv[i + 1]; i += 2; continue
        if a == "--single":
            reads = [argv[i + 1]]; i += 2; continue
        if a == "--left":
            reads = [argv[i + 1]] + reads[1:]; i += 2; continue
        if a == "--right":
            reads = reads[:1] + [argv[i + 1]]; i += 2; continue
        if a == "-K":
            K = int(argv[i + 1]); i += 2; continue
        if a == "-p":
            nJobs = int(argv[i + 1]); i += 2; continue
        if a == "--gpus":
            n_gpus = int(argv[i + 1]); i += 2; continue
        if a == "--partition":
            partition_size = int(argv[i + 1]); i += 2; continue
        if a == "--kmer_hard_cutoff":
            # shannon.py:237-241, 441: `jellyfish dump -L N` -- k1-mers counted fewer than N times never enter k1mer.dict_org
            kmer_hard_cutoff = int(argv[i + 1]); i += 2
            print("OPTIONS --kmer_hard_cutoff: Kmer hard cutoff set to " + str(kmer_hard_cutoff)); continue
        if a == "--kmer_soft_cutoff":
            # shannon.py:243-247, 457: hyp_min_weight -> run_correction's min_weight (the seed threshold, extension_correction.py:345,
            # and the hyperbola of the accept filter, :361)
            min_weight = int(argv[i + 1]); i += 2
            print("OPTIONS --kmer_soft_cutoff: Kmer soft cutoff set to " + str(min_weight)); continue
        if a in ("-s", "--ss", "--strand_specific"):
            # shannon.py:166-207, 407-411: no strand doubling; of a pair, RC(reads_2) stands for reads_2
            double_stranded = False; i += 1; continue
        if a in ("--inMem", "--fasta", "--fastq"):
            fastq_flag, fasta_flag = fastq_flag or a == "--fastq", fasta_flag or a == "--fasta"
            i += 1; continue
        if a == "--filter_FP":
            # shannon.py:170-174 (the reference refuses it with --inMem, :195, because it needs the read files; here the reads are resident)
            if not filter_fp:
                print("OPTIONS --filter_FP: False-positive filtering enabled")
            filter_fp = True; i += 1; continue
        if a == "--inDisk":
            # shannon.py:39-40, 186: the reference's default mode -- the partitions' reads*.fasta / k1mer.dict under TEMP/
            if not in_disk:
                print("OPTIONS --inDisk: In Memory mode disabled")
            in_disk = True; i += 1; continue
        if a == "--only_reads":
            noted.append("%s: the stages hand their data over in memory (the reference's --inMem contract); TEMP/ holds the per-stage "
                         "products but not reads{comp}.fasta / component*k1mers_allowed.dict (shannon_amd/reference_api.py writes those "
                         "when a single stage is driven through the reference's file interface)" % a)
            i += 1; continue
        if a == "--kallisto_cutoff":
            # shannon.py:309-318: what the flag means is known once all of argv is read (the read files' names, --fastq, --fasta)
            kallisto_arg, kallisto_at, kallisto_i = argv[i + 1], len(ignored), i; i += 2; continue
        if a == "--quorum":
            # shannon.py:289-299: like --kallisto_cutoff, what the flag means is known once all of argv is read
            if not quorum_flag:
                quorum_flag, quorum_at, quorum_i = True, len(ignored), i
            i += 1; continue
        if a == "--compare":
            ignored.append(a); i += 2; continue
        ignored.append(a); i += 1
    kallisto_cutoff = None
    # shannon.py:289-307: FASTQ by the first read file's last letter or --fastq; --fasta turns it off
    fastq = ((bool(reads) and reads[0][-1:] == "q") or fastq_flag) and not fasta_flag
    quorum = False
    if quorum_flag:
        if fastq:
            print("OPTIONS --quorum: read error correction with quality scores enabled")
            quorum = True
            if max(nJobs, n_gpus) > 1:
                noted.append("--quorum: the read error correction is built for one-process runs only; with -p N / --gpus N nothing is "
                             "corrected")
                quorum = False
        else:
            print("OPTIONS WARNING: --quorum NOT enabled. Option only works with fastq input.")
            # (among the ignored flags where it stood in argv; a --kallisto_cutoff that joins them below and stood behind it stays behind it)
            ignored.insert(quorum_at, "--quorum")
            if kallisto_arg is not None and kallisto_i > quorum_i:
                kallisto_at += 1
    if kallisto_arg is not None:
        if fastq:
            try:
                kallisto_cutoff = float(kallisto_arg)
            except ValueError:
                print("ERROR: --kallisto_cutoff needs a number, got %s" % kallisto_arg)
                return 2
            print("OPTIONS --kallisto_cutoff: Kallisto will be run to filter low expression transcripts below " + str(kallisto_cutoff))
            if len(reads) != 2:
                noted.append("--kallisto_cutoff: single-end input is not built (the reference runs kallisto --single -l 200 -s 20, "
                             "filter_kallisto.py:25); nothing is filtered")
                kallisto_cutoff = None
            elif max(nJobs, n_gpus) > 1:
                noted.append("--kallisto_cutoff: the abundance filter is built for one-process runs only; with -p N / --gpus N nothing is "
                             "filtered")
                kallisto_cutoff = None
        else:
            print("OPTIONS WARNING: --kallisto_cutoff NOT enabled. Option only works with fastq input.")
            ignored.insert(kallisto_at, "--kallisto_cutoff")
    if filter_fp and len(reads) != 2:
        # run_MB_SF_fn.py:110: `if '--filter_FP' in n_inp and paired_end`
        noted.append("--filter_FP: single-end input -- the reference applies the filter to paired-end runs only (run_MB_SF_fn.py:110); "
                     "nothing is filtered")
        filter_fp = False
    if in_disk and max(nJobs, n_gpus) > 1:
        noted.append("--inDisk: TEMP/<sample>_<comp>algo_input/reads*.fasta and k1mer.dict are written by one-process runs only; with "
                     "-p N / --gpus N the stages hand their data over in memory (shannon_amd/reference_api.py writes the files when a "
                     "single stage is driven through the reference's file interface)")
        in_disk = False
    o = Options()
    o.in_disk = in_disk
    o.K, o.partition_size, o.nJobs, o.n_gpus = K, partition_size, nJobs, n_gpus
    o.out_dir, o.reads, o.double_stranded = out_dir, reads, double_stranded
    o.min_weight, o.min_length, o.kmer_hard_cutoff = min_weight, min_length, kmer_hard_cutoff
    o.ignored, o.noted, o.filter_fp = ignored, noted, filter_fp
    o.kallisto_cutoff = kallisto_cutoff
    o.quorum = quorum
    return o


def main(argv):
    o = parse_args(argv)
    if isinstance(o, int):
        return o
    K, partition_size, nJobs, n_gpus = o.K, o.partition_size, o.nJobs, o.n_gpus
    out_dir, reads, double_stranded = o.out_dir, o.reads, o.double_stranded
    min_weight, min_length, kmer_hard_cutoff = o.min_weight, o.min_length, o.kmer_hard_cutoff
    ignored, noted, filter_fp = o.ignored, o.noted, o.filter_fp
    if out_dir is None or not reads:
        print("ERROR: need -o OUT and --single F or --left F1 --right F2")
        print("Try running python shannon.py --help for a short manual")
        return 2
    if os.path.exists(out_dir) and os.listdir(out_dir):
        print("ERROR: output directory is not empty")              # shannon.py:255-257
        return 2
    if K + 1 > 32:
        print("ERROR: K+1 must be <= 32"); return 2
    # ---- ranks (shannon.py:527-566: the reference's nJobs processes).  Decided and started before anything touches the GPU:
    # torch.cuda.device_count() does not initialise it, and a process that has must never be replaced or forked into ranks.
    in_rank = "WORLD_SIZE" in os.environ and "RANK" in os.environ and os.environ.get("SHN_CLI_RANKS") == "1"
    if not in_rank:
        want = n_gpus if n_gpus > 0 else nJobs
        if want > 1:
            import torch
            have = torch.cuda.device_count()
            share = os.environ.get("SHN_CLI_BACKEND") == "gloo"          # (development / tests: several ranks on ONE GPU, collectives over gloo)
            ranks = want if share else min(want, max(1, have))
            if ranks > 1:
                return launch_ranks(ranks, argv[1:])
            if n_gpus > 1:
                print("NOTE: --gpus %d asked for, the node shows %d GPU(s): one process" % (n_gpus, have))
    if in_rank:
        return rank_main(out_dir, reads, K, partition_size, min_weight, min_length, double_stranded, ignored, noted, kmer_hard_cutoff, filter_fp)
    os.makedirs(out_dir, exist_ok=True)
    sample = os.path.basename(os.path.normpath(out_dir))
    temp = os.path.join(out_dir, "TEMP")
    os.makedirs(temp)
    log = open(os.path.join(out_dir, "log.txt"), "w")

    def say(msg):
        line = "%s: %s" % (time.asctime(), msg)
        print(line)
        log.write(line + "\n")

    import shannon_amd
    if os.environ.get("SHN_MALLOC_TUNE", "1") != "0":
        shannon_amd.malloc_tune()                              # (this program owns its process)
    from shannon_amd import device, pipeline, _lib
    say("Starting Shannon run (MI355X hot path %s)" % VERSION)
    if ignored:
        say("WARNING: flags outside the hot path ignored: " + " ".join(ignored))
    if nJobs != 1:
        noted.append("-p %d: one GPU in use -- the partitions run concurrently on host threads and the GPU inside this process (with several "
                     "GPUs, -p N / --gpus N is N ranks)" % nJobs)
    for msg in noted:
        say("NOTE: " + msg)
    ctx = device.Context(0)
    T = {}
    paired = len(reads) == 2
    # the files straight into HBM (shn_reads_ingest / shn_reads_ingest_ragged: 2-line FASTA / 4-line FASTQ, reads of any lengths,
    # bases outside ACGT kept and marked); only what that refuses (multi-line FASTA, malformed records) is read record by record
    import time as _t
    import numpy as np
    t0 = _t.time()
    sets, got = None, []
    try:
        for p in reads:                                        # (a list built step by step: what was ingested before a refusal is closed below)
            got.append(device.Reads.ingest(ctx, p))
        if len(set(len(g[0]) for g in got)) == 1:
            sets, r = [g[0] for g in got], [g[1] for g in got]
            if any(isinstance(x, device.RaggedCodes) for x in r):      # one mate file ragged, the other not: both as flat codes + offsets
                r = [x if isinstance(x, device.RaggedCodes) else
                     device.RaggedCodes(x.reshape(-1), np.arange(x.shape[0] + 1, dtype=np.uint64) * np.uint64(x.shape[1])) for x in r]
    except _lib.ShannonError as ex:
        if "unsupported" not in str(ex):
            raise
    if sets is None:
        for g in got:                                          # ingested but declined (mate files of different sizes): free the device copies
            g[0].close()
        r = [read_fasta(p) for p in reads]
    T["ingest path"] = "device" if sets is not None else "python"
    T["ingest"] = _t.time() - t0
    avg_len = (sum(len(x) for x in r[0]) / max(1, len(r[0]))) if sets is None else (r[0].total_bases / max(1, len(r[0])) if isinstance(r[0], device.RaggedCodes) else r[0].shape[1])
    say("Processed No of reads:%d, Avg. Read length: %.2f (read files through the %s ingest)" % (len(r[0]), avg_len, T["ingest path"]))
    corrected = None
    if o.quorum and sets is None:
        say("NOTE: --quorum: the read files did not go through the device ingest (multi-line FASTA, mate files of different sizes); "
            "nothing is corrected")
    elif o.quorum:
        # shannon.py:385-391: corrected_reads*.fa take the place of the read files for everything but kallisto (:378, 612)
        from shannon_amd import quorum
        try:
            corrected, r, qst = quorum.apply(ctx, sets, reads, host=r, timings=T)
        except _lib.ShannonError as ex:
            if "needs FASTQ text" not in str(ex):
                raise
            say("NOTE: --quorum: the read files hold no quality lines (FASTA text behind --fastq or a name that ends in q); nothing is corrected")
    try:
        if corrected is not None:
            t0 = _t.time()
            written = quorum.write_fasta(ctx, corrected, temp)
            T["quorum files"] = _t.time() - t0
            say("--quorum: k %d, quality %d, anchor count %d, %d substitutions in a window of %d: %d of %d reads anchored, %d changed, %d substitutions, "
                "%d stopped directions, %d window reverts; table of %d k-mers from %d high-quality windows; %s (%d bytes)"
                % (quorum.K, quorum.MIN_QUALITY, quorum.ANCHOR_COUNT, quorum.MAX_SUBS, quorum.WINDOW, qst["anchored"], sum(len(c) for c in corrected),
                   qst["changed"], qst["substitutions"], qst["stopped"], qst["reverts"], qst["table"], qst["windows"], " ".join(sorted(written)),
                   sum(written.values())))
            tm, tb = ctx.timers(), ctx.timer_bytes()                        # (HIP events around the launches, the bytes their sites price)
            say("quorum kernels: " + json.dumps({k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)}
                                                 for k, v in sorted(tm.items()) if k.startswith("quorum.")}))
        if sets is not None:
            from shannon_amd import kmers_for_component as kfc
            use = corrected if corrected is not None else sets
            R = pipeline.assemble_resident(ctx, use[0], use[1] if paired else None, kfc.ReadStore(r[0], r[1] if paired else None), K=K,
                                           partition_size=partition_size, min_weight=min_weight, min_length=min_length, sample=sample, seed=0,
                                           double_stranded=double_stranded, timings=T, kmer_hard_cutoff=kmer_hard_cutoff,
                                           filter_fp=filter_fp, in_disk_dir=temp if o.in_disk else None, kallisto_cutoff=o.kallisto_cutoff,
                                           kallisto_reads=(sets[0], sets[1] if paired else None) if corrected is not None else None)
        else:
            R = pipeline.assemble(ctx, r[0], r[1] if paired else None, K=K, partition_size=partition_size, min_weight=min_weight,
                                  min_length=min_length, sample=sample, seed=0, double_stranded=double_stranded, timings=T,
                                  kmer_hard_cutoff=kmer_hard_cutoff, filter_fp=filter_fp, in_disk_dir=temp if o.in_disk else None,
                                  kallisto_cutoff=o.kallisto_cutoff)
    finally:
        for c in corrected or ():                       # (nothing behind the pipeline reads the corrected sets)
            c.close()
    if o.in_disk:
        say("--inDisk: reads*.fasta and k1mer.dict of %d partitions under %s (%d bytes)"
            % (len(R.in_disk), temp, sum(sum(f.values()) for f in R.in_disk.values())))
    say("%d K-mers loaded; %d contigs; %d partitions" % (R.n_k1mers, len(R.extension.contigs), len(R.partitions)))
    # TEMP tree: the per-stage products of the reference (shannon.py:496-513, 584-595)
    from shannon_amd import extension_correction as ec, mbgraph
    ai = os.path.join(temp, sample + "_algo_input")
    os.makedirs(ai)
    ec.write_outputs(R.extension, temp, os.path.join(ai, "k1mer.dict"))
    for name, p in R.partitions.items():
        base = os.path.join(temp, "%s_%s" % (sample, name))
        for sub in ("algo_output", "intermediate"):
            os.makedirs(base + sub)
        mbgraph.write_files(p["singles"], p["components"], base + "intermediate")
        open(os.path.join(base + "algo_output", "reconstructed.fasta"), "w").write(p["reconstructed_fasta"])
        if "filter_log" in p:
            # filter_FP.py:52-55: the filtered transcripts take the place of reconstructed.fasta, the sparse flow's stay beside them
            open(os.path.join(base + "algo_output", "reconstructed_org.fasta"), "w").write(p["reconstructed_org_fasta"])
            open(os.path.join(base + "algo_output", "rec.log"), "w").write(p["filter_log"])
            say("%s has completed: %d transcripts, %d after --filter_FP" % (base, p["reconstructed_org_fasta"].count(">"),
                                                                           p["reconstructed_fasta"].count(">")))
            continue
        say("%s has completed: %d transcripts" % (base, p["reconstructed_fasta"].count(">")))
    if filter_fp:
        st = getattr(R, "filter_fp_stats", {})
        say("--filter_FP: %d of %d routed fragments placed as concordant pairs; %d of %d transcripts kept"
            % (st.get("placed", 0), st.get("routes", 0), st.get("kept", 0), st.get("transcripts", 0)))
    alld = os.path.join(temp, sample + "_allalgo_output")
    os.makedirs(alld)
    open(os.path.join(alld, "all_reconstructed.fasta"), "w").write("".join(R.all_reconstructed))
    if getattr(R, "abundance", None) is not None:
        # shannon.py:611-614: the merged transcripts move to rec_before_kallisto.fasta, `kallisto quant -o <dir>/kallisto` leaves
        # abundance.tsv there, what filter_using_kallisto keeps becomes the final FASTA
        ab = R.abundance
        os.makedirs(os.path.join(alld, "kallisto"))
        open(os.path.join(alld, "rec_before_kallisto.fasta"), "w").write(ab["before"])
        open(os.path.join(alld, "kallisto", "abundance.tsv"), "w").write(ab["tsv"])
        say("--kallisto_cutoff %s: %d of %d fragments mapped, %d classes, %d EM rounds, L %s; %d of %d transcripts kept"
            % (o.kallisto_cutoff, ab["mapped"], ab["fragments"], ab["classes"], ab["rounds"], repr(ab["L"]), ab["kept"], len(ab["names"])))
        tm, tb = ctx.timers(), ctx.timer_bytes()                    # (HIP events around the launches, the bytes their sites price)
        say("abundance kernels: " + json.dumps({k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)}
                                                for k, v in sorted(tm.items()) if k.startswith("abundance.")}))
    if hasattr(R.final, "fasta"):                                   # (the native merge's buffers: the file's text without a string per record)
        with open(os.path.join(out_dir, "shannon.fasta"), "wb") as f:
            f.write(R.final.fasta())
    else:
        with open(os.path.join(out_dir, "shannon.fasta"), "w") as f:
            for name, seq in R.final.items():
                f.write(">%s\n%s\n" % (name, seq))
    say("All partitions completed: %d transcripts reconstructed" % len(R.final))
    say("stage seconds: " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in T.items()}))
    log.close()
    ctx.close()
    print("-------------------------------------------------")
    print(time.asctime() + ": Shannon Run Completed")
    print("-------------------------------------------------")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
