"""Quantify a set of transcripts against single-end or paired reads: the quantifier of --kallisto_cutoff as a command of its own
(filter_kallisto.py:23-31 -- `kallisto index` + `kallisto quant`, with `--single -l 200 -s 20` for one read file).

    python -m shannon_amd.quant TRANSCRIPTS.fasta -o DIR (--single R[,R..] | --left R1[,R1..] --right R2[,R2..]) [-s] [--cutoff C]
                                [-l MEAN] [--sd SD] [-b B [--seed S]] [--gpus N]

Paired reads go through abundance.quantify, unchanged: abundance.tsv is what a --kallisto_cutoff run writes for the
same transcripts and pairs.  Single reads go through abundance.quantify_single.  Written into DIR:

    abundance.tsv    abundance.abundance_tsv of the table: kallisto's header, the floats written with repr
    quant_log.txt    reads or pairs, mapped, classes, EM rounds, L, and the abundance.* kernel groups' times and priced bytes
    filtered.fasta   with --cutoff C: abundance.decide on the text of abundance.tsv and of TRANSCRIPTS.fasta

With -b B (bootstrap replicates of the abundances under the 64-bit seed S, 0 unless given: DESIGN.md 3.14) also:

    bs_abundance_<b>.tsv   b = 0..B-1: abundance.abundance_tsv of replicate b's table (kallisto's --plaintext layout)
    bootstrap_summary.tsv  target_id est_counts bs_mean bs_sd bs_min bs_max, the floats written with repr
    quant_log.txt          one more line: B, the seed, the smallest and the largest round count of the replicates

abundance.tsv and filtered.fasta are byte for byte those of the run without -b.

A sample in several lane files (comma-separated; a value that names an existing file is one file) and / or on N ranks (--gpus N: one
process per GPU, started as fresh children; SHN_CLI_BACKEND=gloo puts them all on GPU 0): every lane's -- every rank's slice of every
lane's -- compatibility classes are built on their own, a lane loaded and closed before the next, and the class sets are merged on the
device (abundance.merge_classes).  Every file above is byte for byte that of the one-process run on the concatenated
files; quant_log.txt gains a line: parts, lists in, classes out, the abundance.merge group.  One file (or pair) without --gpus is the run
it always was: no merge.

    targets       (names, sequences) of the FASTA text; a duplicate id, an empty id or an empty sequence raises QuantError
    load_reads    a read file -> a resident device.Reads (the device ingest, else record by record)
    quantify_files  the whole step in one process (lane files: _quantify_lanes)
    launch_ranks, rank_main  --gpus N: the parent starts the ranks and makes no GPU call; a rank's work, rank 0 writes the files
    main          the command: 0 done, 2 a usage error (with a message)

`targets` and the argument checks of `main` need neither the library nor a GPU."""
import json
import os
import re
import sys

USAGE = ("usage: python -m shannon_amd.quant TRANSCRIPTS.fasta -o DIR (--single R[,R..] | --left R1[,R1..] --right R2[,R2..]) [-s] [--cutoff C] [-l MEAN] "
         "[--sd SD] [-b B [--seed S]] [--gpus N]\n"
         "  TRANSCRIPTS.fasta  the transcripts to quantify (2-line or multi-line FASTA; the id is the header's first token)\n"
         "  -o DIR             where abundance.tsv, quant_log.txt and filtered.fasta go\n"
         "  --single R         single-end reads (FASTA or FASTQ)\n"
         "  --left R1 --right R2  paired reads, mates in the same order\n"
         "  R,R,..             a sample in several lane files: comma-separated, --left and --right lane by lane (a value that names an\n"
         "                     existing file is one file)\n"
         "  -s                 strand-specific: single reads are placed forward only, pairs as (R1, RC(R2)) only\n"
         "  --cutoff C         also write filtered.fasta: the transcripts with est_counts / eff_length * L >= C\n"
         "  -l MEAN, --sd SD   single-end only: mean and standard deviation of the fragment-length model (200, 20)\n"
         "  -b B               also B >= 1 bootstrap replicates: bs_abundance_<b>.tsv and bootstrap_summary.tsv\n"
         "  --seed S           with -b: the seed of the resampling, an integer in 0 .. 2^64 - 1 (0)\n"
         "  --gpus N           N >= 1 ranks, one per GPU, each on its share of every lane's reads (1: this process)\n")


class QuantError(Exception):
    """an input the command refuses (exit code 2)"""


def targets(fasta_text):
    """(names, sequences) of a FASTA text in file order (compare.records: the id is the header's first token, the sequence lines
    joined and upper-cased).  Refused: an id that occurs twice, a header without an id, a record without a sequence.  Nothing is
    refused for length or content: a short transcript or one with a base outside ACGT gets est_counts 0."""
    from . import compare
    names, seqs, seen = [], [], set()
    for name, seq in compare.records(fasta_text):
        if not name:
            raise QuantError("a header without a target id")
        if name in seen:
            raise QuantError("target id %s occurs twice" % name)
        if not seq:
            raise QuantError("target %s has no sequence" % name)
        seen.add(name)
        names.append(name)
        seqs.append(seq)
    return names, seqs


def _read_records(path):
    """the sequences of a FASTA (2-line or multi-line) or 4-line FASTQ file, record by record"""
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
                    seqs.append("".join(cur))
                cur = []
            elif cur is not None:
                cur.append(line.strip())
        if cur is not None:
            seqs.append("".join(cur))
    return seqs


def load_reads(ctx, path):
    """a read file as a resident set: device.Reads.ingest (2-line FASTA / 4-line FASTQ of any lengths); what that declines
    (multi-line FASTA, malformed records) is read record by record, as shannon.py does"""
    from . import device, _lib
    try:
        return device.Reads.ingest(ctx, path, want_codes=False)[0]
    except _lib.ShannonError as ex:
        if "unsupported" not in str(ex):
            raise
    return device.Reads.from_strings(ctx, _read_records(path))


def quantify_files(fasta, out_dir, single=None, left=None, right=None, strand_specific=False, cutoff=None, mean=None, sd=None, ctx=None, bootstraps=None,
                   seed=0):
    """The command's work: the table of the transcripts of `fasta` under the reads of `single`, or the pairs of `left` / `right`,
    written into out_dir (the module's head says what).  Returns the table with "L", "paired" and, with a cutoff, "kept"; with bootstraps=B, the
    replicates' columns (abundance.quantify)."""
    from . import abundance, device, _lib
    with open(fasta) as f:
        fasta_text = f.read()
    names, seqs = targets(fasta_text)
    paired = single is None
    if not isinstance(left if paired else single, str):       # lane files: every lane's classes, merged
        return _quantify_lanes(fasta_text, names, seqs, out_dir, _lanes(single, left, right), paired, strand_specific, cutoff, mean, sd, ctx, bootstraps, seed)
    own = ctx is None
    if own:
        ctx = device.Context(0)
    sets = []
    try:
        for p in ([left, right] if paired else [single]):
            sets.append(load_reads(ctx, p))
        if paired and len(sets[0]) != len(sets[1]):
            raise QuantError("%s holds %d reads, %s holds %d: not mates of each other" % (left, len(sets[0]), right, len(sets[1])))
        ctx.timer_reset()
        if paired:
            table = abundance.quantify(ctx, names, seqs, sets[0], sets[1], strand_specific, bootstraps=bootstraps, seed=seed)
            table["L"] = abundance.fragment_bases(sets[0], sets[1])
        else:
            table = abundance.quantify_single(ctx, names, seqs, sets[0], strand_specific, abundance.MODEL_MEAN if mean is None else mean,
                                              abundance.MODEL_SD if sd is None else sd, bootstraps=bootstraps, seed=seed)
            n = len(sets[0])
            table["L"] = int(_lib.lib().shn_reads_total_bases(sets[0].h)) / n if n else 0.0      # (shannon.py:613 with one file)
        tm, tb = ctx.timers(), ctx.timer_bytes()
    finally:
        for d in sets:
            d.close()
        if own:
            ctx.close()
    return _write_outputs(out_dir, table, fasta_text, paired, strand_specific, cutoff, mean, sd, bootstraps, tm, tb)


def _write_outputs(out_dir, table, fasta_text, paired, strand_specific, cutoff, mean, sd, bootstraps, tm, tb, merge_line=None):
    """the files of a finished table (with "L") into out_dir; tm / tb: the context's timers and priced bytes; merge_line: the log's
    line of a run whose classes were merged.  Returns the table with "paired" and, with a cutoff, "kept"."""
    from . import abundance
    names = table["names"]
    table["paired"] = paired
    tsv = abundance.abundance_tsv(table)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "abundance.tsv"), "w") as f:
        f.write(tsv)
    log = ["%s: %d of %d mapped, %d classes, %d EM rounds, L %s" % ("pairs" if paired else "reads", table["mapped"], table["fragments"], table["classes"],
                                                                      table["rounds"], repr(table["L"]))]
    if not paired:
        log.append("single-end: %s, fragment-length model mean %s sd %s" % ("forward only" if strand_specific else "both orientations",
                                                                           repr(float(abundance.MODEL_MEAN if mean is None else mean)),
                                                                           repr(float(abundance.MODEL_SD if sd is None else sd))))
    if cutoff is not None:
        kept_text = abundance.decide(tsv, fasta_text, float(cutoff), table["L"])
        with open(os.path.join(out_dir, "filtered.fasta"), "w") as f:
            f.write(kept_text)
        table["kept"] = sum(1 for line in kept_text.splitlines() if line.startswith(">"))
        log.append("--cutoff %s: %d of %d transcripts kept" % (repr(float(cutoff)), table["kept"], len(names)))
    if bootstraps is not None:
        for b in range(table["bootstraps"]):
            with open(os.path.join(out_dir, "bs_abundance_%d.tsv" % b), "w") as f:
                f.write(abundance.abundance_tsv(abundance.replicate_table(table, b)))
        with open(os.path.join(out_dir, "bootstrap_summary.tsv"), "w") as f:
            f.write(abundance.bootstrap_summary_tsv(table))
        log.append("-b %d --seed %d: EM rounds of the replicates %d .. %d" % (table["bootstraps"], table["seed"], min(table["bs_rounds"]),
                                                                               max(table["bs_rounds"])))
    if merge_line is not None:
        log.append(merge_line)
    log.append("abundance kernels: " + json.dumps({k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)}
                                                    for k, v in sorted(tm.items()) if k.startswith("abundance.")}))
    with open(os.path.join(out_dir, "quant_log.txt"), "w") as f:
        f.write("".join(l + "\n" for l in log))
    return table


def _as_list(v):
    return [v] if isinstance(v, str) else list(v)


def _lanes(single, left, right):
    """the lanes of a run as tuples of paths: (file,) per single-end lane, (left, right) per paired one"""
    if single is not None:
        return [(p,) for p in _as_list(single)]
    left, right = _as_list(left), _as_list(right)
    if len(left) != len(right):
        raise QuantError("--left lists %d files, --right %d: every lane needs both mates" % (len(left), len(right)))
    return list(zip(left, right))


def _not_mates(lane, paths, n1, n2):
    return QuantError("lane %d: %s holds %d reads, %s holds %d: not mates of each other" % (lane, paths[0], n1, paths[1], n2))


def _merge_line(table, ranks, tm, tb):
    g = tm.get("abundance.merge")
    return "merge: %d parts%s, %d lists in, %d classes out; abundance.merge %s" % (
        table["parts"], " (%d ranks)" % ranks if ranks > 1 else "", table["lists"], table["classes"],
        json.dumps({"ms": round(g[0], 4), "regions": g[1], "bytes": tb.get("abundance.merge", 0)} if g else {}))


def _quantify_lanes(fasta_text, names, seqs, out_dir, lanes, paired, strand_specific, cutoff, mean, sd, ctx, bootstraps, seed):
    """quantify_files for a sample in several lane files, in one process: a lane is loaded, its classes are built and it is closed
    before the next one is touched -- the device holds one lane's reads at a time -- then abundance.quantify_classes.  L: the bases of
    all lanes over the fragments of all lanes, both as integers."""
    from . import abundance, device, _lib
    tally = {"bases": 0, "fragments": 0}

    def load(p):
        return load_reads(ctx, p) if os.path.getsize(p) else device.Reads.from_strings(ctx, [])

    def resident_lanes():
        for i, paths in enumerate(lanes):
            sets = []
            try:
                for p in paths:
                    sets.append(load(p))
                if paired and len(sets[0]) != len(sets[1]):
                    raise _not_mates(i + 1, paths, len(sets[0]), len(sets[1]))
                tally["bases"] += sum(int(_lib.lib().shn_reads_total_bases(d.h)) for d in sets)
                tally["fragments"] += len(sets[0])
                yield tuple(sets)
            finally:
                for d in sets:
                    d.close()
    own = ctx is None
    if own:
        ctx = device.Context(0)
    gen = resident_lanes()
    try:
        ctx.timer_reset()
        table = abundance.quantify_parts(ctx, names, seqs, gen, strand_specific, mean=abundance.MODEL_MEAN if mean is None else mean,
                                         sd=abundance.MODEL_SD if sd is None else sd, bootstraps=bootstraps, seed=seed)
        tm, tb = ctx.timers(), ctx.timer_bytes()
    finally:
        gen.close()
        if own:
            ctx.close()
    table["L"] = tally["bases"] / tally["fragments"] if tally["fragments"] else 0.0
    return _write_outputs(out_dir, table, fasta_text, paired, strand_specific, cutoff, mean, sd, bootstraps, tm, tb, _merge_line(table, 1, tm, tb))


# ---------------------------------------------------------------------------------------------------------------- N ranks
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, args):
    """start the n ranks as fresh child processes (torch.distributed.run on 127.0.0.1 with a free port, as shannon.py's launch_ranks;
    the children run this module) and hand their exit code on; this parent makes no GPU call"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SHN_CLI_RANKS="1")
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL between processes needs it on this stack
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "shannon_amd.quant"] + list(args)
    return subprocess.call(cmd, env=env, cwd=os.getcwd())


def _rank_slice(ctx, paths, rank, world, cdev, lane):
    """this rank's records [n r / W, n (r + 1) / W) of a lane's files as resident sets: by bytes of the files
    (distributed.ingest_rank_slice -- a collective: every rank calls it for every lane), else whole files sliced by index"""
    import numpy as np
    from . import device, distributed, _lib
    try:
        sl = distributed.ingest_rank_slice(list(paths), rank, world, None, cdev, ragged=True)
    except _lib.ShannonError as ex:
        if "different numbers of reads" in str(ex):                 # (every rank sees the same counts: all raise together)
            raise QuantError("lane %d: %s and %s are not mates of each other: %s" % (lane, paths[0], paths[-1], ex))
        raise
    if sl is not None:
        qs = list(sl[0])
    else:
        whole = []
        for p in paths:
            try:
                whole.append(device.Reads.ingest(None, p)[1] if os.path.getsize(p) else [])
            except _lib.ShannonError as ex:
                if "unsupported" not in str(ex):
                    raise
                whole.append(_read_records(p))
        if len(whole) == 2 and len(whole[0]) != len(whole[1]):
            raise _not_mates(lane, paths, len(whole[0]), len(whole[1]))
        n = len(whole[0])
        qs = [w[rank * n // world:(rank + 1) * n // world] for w in whole]
    sets = []
    try:
        for q in qs:
            if len(q) == 0:
                sets.append(device.Reads.from_strings(ctx, []))
            elif isinstance(q, list):
                sets.append(device.Reads.from_strings(ctx, q))
            elif isinstance(q, device.RaggedCodes):
                sets.append(device.Reads.from_ragged(ctx, q.codes, q.off))
            else:
                sets.append(device.Reads.from_codes(ctx, np.ascontiguousarray(q)))
    except Exception:
        for d in sets:
            d.close()
        raise
    return sets


def rank_main(o):
    """one rank of `--gpus N`: its slice of every lane's records, the classes of each slice, all ranks' classes to rank 0
    (exchange.all_gather_arrays; mapped, fragment and base counts as integers), which merges them in (lane, rank) order, runs
    abundance.quantify_classes and writes the files.  A rank whose own work fails still takes part in the later lanes' collectives
    and tells the others before the classes travel: all ranks end with 2 together."""
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("SHN_CLI_BACKEND") == "gloo"
    lanes = _lanes(o.get("single"), o.get("left"), o.get("right"))
    paired = "single" not in o
    if os.environ.get("SHN_CLI_LAUNCH_PROBE"):
        # CPU test of the launch: the ranks meet over gloo, rank 0 says what the launch resolved to; nothing touches the GPU
        dist.init_process_group("gloo")
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        if rank == 0:
            print("launch probe: %d ranks met, %d %s lanes, out=%s" % (int(one.item()), len(lanes), "paired" if paired else "single-end", o["out_dir"]))
        dist.destroy_process_group()
        return 0
    dev_index = 0 if share else local
    torch.cuda.set_device(dev_index)
    if share:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
    from . import abundance, device, exchange, _lib
    ss, mean, sd = o["strand_specific"], o.get("mean"), o.get("sd")
    mean, sd = abundance.MODEL_MEAN if mean is None else mean, abundance.MODEL_SD if sd is None else sd
    ctx = device.Context(dev_index)
    rc = 0
    try:
        with open(o["fasta"]) as f:
            fasta_text = f.read()
        names, seqs = targets(fasta_text)
        cdev = exchange.coll_device(torch.device("cuda", dev_index), None)
        ctx.timer_reset()
        parts, err = [], None
        for i, paths in enumerate(lanes):
            sets = _rank_slice(ctx, paths, rank, world, cdev, i + 1)       # (what this raises, every rank raises)
            try:
                if err is None:
                    cl = abundance.classes(ctx, seqs, sets[0], sets[1], ss) if paired else abundance.classes_single(ctx, seqs, sets[0], ss)
                    cl["bases"] = sum(int(_lib.lib().shn_reads_total_bases(d.h)) for d in sets)
                    parts.append(cl)
            except Exception as ex:
                err = "rank %d, lane %d: %s" % (rank, i + 1, ex)
            finally:
                for d in sets:
                    d.close()
        errs = [e for e in exchange.all_gather_object(err, name="quant: the ranks' status") if e]
        if errs:
            raise QuantError("; ".join(errs))
        u64 = lambda xs: np.array(list(xs), dtype=np.uint64)
        cat = lambda k, dt: np.concatenate([np.asarray(p[k], dtype=dt) for p in parts]) if parts else np.zeros(0, dt)
        mine = (u64(len(p["n_c"]) for p in parts), u64(len(p["members"]) for p in parts), u64(len(p["hist"]) for p in parts),
                cat("class_off", np.uint64), cat("members", np.uint32), cat("n_c", np.uint64), cat("hist", np.uint64),
                u64(x for p in parts for x in (p["mapped"], p["fragments"], p["bases"])))
        got = exchange.all_gather_arrays(mine, cdev, name="quant: the ranks' classes")
        status = None
        if rank == 0:
            try:
                by_rank = [_unpack_parts(g) for g in got]
                ordered = [by_rank[r][i] for i in range(len(lanes)) for r in range(world)]
                table = abundance.quantify_classes(ctx, names, seqs, ordered, paired, mean, sd, o.get("bootstraps"), o.get("seed", 0))
                bases, frags = sum(p["bases"] for p in ordered), sum(p["fragments"] for p in ordered)
                table["L"] = bases / frags if frags else 0.0
                tm, tb = ctx.timers(), ctx.timer_bytes()
                t = _write_outputs(o["out_dir"], table, fasta_text, paired, ss, o.get("cutoff"), o.get("mean"), o.get("sd"), o.get("bootstraps"), tm, tb,
                                   _merge_line(table, world, tm, tb))
                _say(t)
            except Exception as ex:
                status = "rank 0: %s" % ex
        status = exchange.all_gather_object(status, name="quant: the ranks' status")[0]
        if status:
            raise QuantError(status)
    except QuantError as ex:
        if rank == 0:
            sys.stderr.write("%s\n" % ex)
        rc = 2
    finally:
        ctx.close()
        dist.destroy_process_group()
    return rc


def _unpack_parts(arrays):
    """a rank's classes as they travelled (rank_main) -> its class dicts, one per lane, each with its reads' bases"""
    n_cls, n_mem, n_bins, class_off, members, n_c, hist, ints = arrays
    out, a_off, a_mem, a_cls, a_bin = [], 0, 0, 0, 0
    for i in range(len(n_cls)):
        c, e, b = int(n_cls[i]), int(n_mem[i]), int(n_bins[i])
        out.append({"class_off": class_off[a_off:a_off + c + 1], "members": members[a_mem:a_mem + e], "n_c": n_c[a_cls:a_cls + c],
                    "hist": hist[a_bin:a_bin + b], "mapped": int(ints[3 * i]), "fragments": int(ints[3 * i + 1]), "bases": int(ints[3 * i + 2])})
        a_off, a_mem, a_cls, a_bin = a_off + c + 1, a_mem + e, a_cls + c, a_bin + b
    return out


def _split_lanes(value):
    """a value of --single / --left / --right: the name of an existing file is one file (a string, as ever); anything else is split at
    commas into lane files (a list)"""
    if os.path.isfile(value) or "," not in value:
        return value
    return value.split(",")


def parse_args(argv):
    """argv (the program's name first) -> a dict of quantify_files' arguments (+ "gpus" when N > 1 ranks are asked for), or a message (a
    usage error)"""
    takes = {"-o": "out_dir", "--single": "single", "--left": "left", "--right": "right", "--cutoff": "cutoff", "-l": "mean", "--sd": "sd",
             "-b": "bootstraps", "--seed": "seed", "--gpus": "gpus"}
    o = {"strand_specific": False}
    rest = []
    a = list(argv[1:])
    while a:
        x = a.pop(0)
        if x == "-s":
            o["strand_specific"] = True
        elif x in takes:
            if not a:
                return "%s needs a value" % x
            if takes[x] in o:
                return "%s given twice" % x
            o[takes[x]] = a.pop(0)
        elif x.startswith("-"):
            return "unknown option %s" % x
        else:
            rest.append(x)
    if len(rest) != 1:
        return "one TRANSCRIPTS.fasta is needed, %d given" % len(rest)
    o["fasta"] = rest[0]
    if "out_dir" not in o:
        return "-o DIR is needed"
    if "single" in o and ("left" in o or "right" in o):
        return "--single and --left / --right exclude each other"
    if "single" not in o and not ("left" in o and "right" in o):
        return "reads are needed: --single R, or --left R1 and --right R2"
    if "single" not in o and ("mean" in o or "sd" in o):
        return "-l / --sd belong to single-end input: the fragment lengths of pairs are measured"
    for k in ("cutoff", "mean", "sd"):
        if k in o:
            try:
                o[k] = float(o[k])
            except ValueError:
                return "%s is not a number" % o[k]
            if o[k] != o[k] or o[k] in (float("inf"), float("-inf")):
                return "%s is not a finite number" % o[k]
    if "sd" in o and not o["sd"] > 0.0:
        return "--sd must be above 0"
    if "seed" in o and "bootstraps" not in o:
        return "--seed belongs to -b B: without replicates nothing is drawn"
    for k, flag, lo, hi in (("bootstraps", "-b", 1, (1 << 32) - 1), ("seed", "--seed", 0, (1 << 64) - 1)):
        if k in o:
            if not re.fullmatch("-?[0-9]+", o[k]):
                return "%s %s is not an integer" % (flag, o[k])
            o[k] = int(o[k], 10)
            if not lo <= o[k] <= hi:
                return "%s %d is outside %d .. %d" % (flag, o[k], lo, hi)
    if "gpus" in o:
        if not re.fullmatch("-?[0-9]+", o["gpus"]):
            return "--gpus %s is not an integer" % o["gpus"]
        o["gpus"] = int(o["gpus"], 10)
        if o["gpus"] < 1:
            return "--gpus %d: at least 1" % o["gpus"]
        if o["gpus"] == 1:
            del o["gpus"]                                         # (one process: today's run)
    if not os.path.isfile(o["fasta"]):
        return "%s: no such file" % o["fasta"]
    for k in ("single", "left", "right"):
        if k in o:
            o[k] = _split_lanes(o[k])
            for p in ([o[k]] if isinstance(o[k], str) else o[k]):
                if not os.path.isfile(p):
                    return "%s: no such file" % p
    if "left" in o and len(_as_list(o["left"])) != len(_as_list(o["right"])):
        return "--left lists %d files, --right %d: every lane needs both mates" % (len(_as_list(o["left"])), len(_as_list(o["right"])))
    return o


def _say(t):
    print("%d of %d %s mapped, %d classes, %d EM rounds%s" % (t["mapped"], t["fragments"], "pairs" if t["paired"] else "reads", t["classes"], t["rounds"],
                                                          "; %d of %d transcripts kept" % (t["kept"], len(t["names"])) if "kept" in t else ""))


def main(argv):
    """python -m shannon_amd.quant ...; 0 done, 2 a usage error or a refused input (a message on stderr); with --gpus N > 1 the exit code
    of the ranks"""
    o = parse_args(argv)
    if isinstance(o, str):
        sys.stderr.write("%s\n%s" % (o, USAGE))
        return 2
    # ---- ranks.  Decided and started before anything touches the GPU: torch.cuda.device_count() does not initialise it, and a
    # process that has must never be replaced or forked into ranks.
    if "WORLD_SIZE" in os.environ and "RANK" in os.environ and os.environ.get("SHN_CLI_RANKS") == "1":
        return rank_main(o)
    want = o.pop("gpus", 1)
    if want > 1:
        try:
            with open(o["fasta"]) as f:
                targets(f.read())                               # (refused here, before any process is started)
        except QuantError as ex:
            sys.stderr.write("%s\n" % ex)
            return 2
        import torch
        have = torch.cuda.device_count()
        share = os.environ.get("SHN_CLI_BACKEND") == "gloo"       # (development / tests: several ranks on ONE GPU, collectives over gloo)
        ranks = want if share else min(want, max(1, have))
        if ranks < want:
            print("NOTE: --gpus %d asked for, the node shows %d GPU(s): %s" % (want, have, "%d ranks" % ranks if ranks > 1 else "one process"))
        if ranks > 1:
            return launch_ranks(ranks, argv[1:])                  # (a rank learns the number that was decided here from its environment)
    try:
        t = quantify_files(**o)                                 # (the transcripts are checked before the device is touched)
    except QuantError as ex:
        sys.stderr.write("%s\n" % ex)
        return 2
    _say(t)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
