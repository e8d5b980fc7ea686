"""Correct the reads of a sample with their quality scores: the step of --quorum (shannon.py:289-299, 385-391; the rule of DESIGN.md
3.11) as a command of its own -- a sample in several lane files, on N ranks, and optionally trimmed.

    python -m shannon_amd.correct -o DIR (--single R[,R..] | --left R1[,R1..] --right R2[,R2..])
           [-k 24] [-q 5] [--anchor 3] [--window 10] [--errors 3] [--trim [--min_len M]] [--gpus N]

Written into DIR (which must be empty or absent):

    corrected_reads_1.fa, corrected_reads_2.fa   paired input (single-end: corrected_reads.fa): 2-line FASTA, record i named >i_1 /
                      >i_2 (>i), i counting the records of the sample, lanes in the order given; formatted on the device
    correct_log.txt   the parameters; per lane its reads, high-quality bases and high-quality windows; the size of the table of the
                      whole sample; the five counters of DESIGN.md 3.11; with --trim the five of rule 7; the quorum.* kernel groups

Without --trim the files are byte for byte the TEMP/corrected_reads*.fa of `shannon.py --quorum` on the concatenated lanes.  The device
holds one lane's reads at a time, so the lanes are read twice: pass 1 adds every lane's table of high-quality windows to the running
one (quorum.add_tables), pass 2 corrects every lane against the finished table and writes.  --trim cuts every read to the span its
walks vouch for and drops what is shorter than M (rules 6 and 7).  --gpus N: N ranks, started as quant starts them, each on its
slice of every lane's records; the ranks' tables are summed at their owners and replicated, every rank writes its own stretch, rank 0
puts the stretches together.  Every file but the log's kernel line is byte for byte that of the one-process run.

    parse_args   the command line -> the options, or a message (neither the library nor a GPU is needed)
    run          the work of one rank (of the only one)
    main         0 done, 2 a usage error or a refused input (a message on stderr)"""
import json
import os
import re
import sys

USAGE = ("usage: python -m shannon_amd.correct -o DIR (--single R[,R..] | --left R1[,R1..] --right R2[,R2..]) [-k 24] [-q 5] [--anchor 3] [--window 10] "
         "[--errors 3] [--trim [--min_len M]] [--gpus N]\n"
         "  -o DIR             where corrected_reads*.fa and correct_log.txt go (empty or absent)\n"
         "  --single R         single-end reads, FASTQ text (.gz too)\n"
         "  --left R1 --right R2  paired reads, mates in the same order\n"
         "  R,R,..             a sample in several lane files: comma-separated, --left and --right lane by lane (a value that names an\n"
         "                     existing file is one file)\n"
         "  -k K               length of the trusted k-mers, 15 .. 32 (24)\n"
         "  -q Q               a base is high-quality from this quality on, 0 .. 93 (5)\n"
         "  --anchor A         a window the table holds A times or more is an anchor, A >= 1 (3)\n"
         "  --window W --errors E  a walk that would make more than E substitutions within W bases sets them back and ends, W >= 1, E 0 .. 4 (10, 3)\n"
         "  --trim             cut every read to the span its walks vouch for; drop a read (a pair) whose span (either span) is below M\n"
         "  --min_len M        with --trim: M >= 1 (K)\n"
         "  --gpus N           N >= 1 ranks, one per GPU, each on its share of every lane's reads (1: this process)\n")

FILES_PAIRED, FILES_SINGLE = ("corrected_reads_1.fa", "corrected_reads_2.fa"), ("corrected_reads.fa",)


class CorrectError(Exception):
    """an input the command refuses (exit code 2)"""


def _split_lanes(value):
    """as quant._split_lanes, but always a list: the name of an existing file is one lane"""
    if os.path.isfile(value) or "," not in value:
        return [value]
    return value.split(",")


def parse_args(argv):
    """argv (the program's name first) -> a dict of the options, or a message (a usage error).  Keys: out_dir, single or left + right
    (lists of lane files), k, q, anchor, window, errors, trim, min_len, gpus."""
    takes = {"-o": "out_dir", "--single": "single", "--left": "left", "--right": "right", "-k": "k", "-q": "q", "--anchor": "anchor", "--window": "window",
             "--errors": "errors", "--min_len": "min_len", "--gpus": "gpus"}
    o = {"trim": False}
    a = list(argv[1:])
    while a:
        x = a.pop(0)
        if x == "--trim":
            o["trim"] = True
        elif x in takes:
            if not a:
                return "%s needs a value" % x
            if takes[x] in o:
                return "%s given twice" % x
            o[takes[x]] = a.pop(0)
        else:
            return "unknown option %s" % x if x.startswith("-") else "unexpected argument %s" % x
    if "out_dir" not in o:
        return "-o DIR is needed"
    if "single" in o and ("left" in o or "right" in o):
        return "--single and --left / --right exclude each other"
    if "single" not in o and not ("left" in o and "right" in o):
        return "reads are needed: --single R, or --left R1 and --right R2"
    from . import quorum as qd                                 # (its numbers only: nothing is loaded)
    for key, flag, dflt, lo, hi in (("k", "-k", qd.K, 15, 32), ("q", "-q", qd.MIN_QUALITY, 0, 93), ("anchor", "--anchor", qd.ANCHOR_COUNT, 1, (1 << 31) - 1),
                                    ("window", "--window", qd.WINDOW, 1, (1 << 31) - 1), ("errors", "--errors", qd.MAX_SUBS, 0, 4),
                                    ("min_len", "--min_len", None, 1, (1 << 31) - 1), ("gpus", "--gpus", 1, 1, 1 << 16)):
        if key in o:
            if not re.fullmatch("-?[0-9]+", o[key]):
                return "%s %s is not an integer" % (flag, o[key])
            o[key] = int(o[key], 10)
            if not lo <= o[key] <= hi:
                return "%s %d is outside %d .. %d" % (flag, o[key], lo, hi)
        elif dflt is not None:
            o[key] = dflt
    if "min_len" in o and not o["trim"]:
        return "--min_len belongs to --trim: without it nothing is cut"
    if o["trim"]:
        o.setdefault("min_len", o["k"])
    for key in ("single", "left", "right"):
        if key in o:
            o[key] = _split_lanes(o[key])
            for p in o[key]:
                if not os.path.isfile(p):
                    return "%s: no such file" % p
    if "left" in o and len(o["left"]) != len(o["right"]):
        return "--left lists %d files, --right %d: every lane needs both mates" % (len(o["left"]), len(o["right"]))
    if os.path.exists(o["out_dir"]) and (not os.path.isdir(o["out_dir"]) or os.listdir(o["out_dir"])):
        return "%s: the output directory is not empty" % o["out_dir"]
    return o


def lanes_of(o):
    """the lanes of a run as tuples of paths: (file,) per single-end lane, (left, right) per paired one"""
    return [(p,) for p in o["single"]] if "single" in o else list(zip(o["left"], o["right"]))


def _not_mates(lane, paths, n1, n2):
    return CorrectError("lane %d: %s holds %d reads, %s holds %d: not mates of each other" % (lane, paths[0], n1, paths[1], n2))


# ---------------------------------------------------------------------------------------------------- a rank's records of a lane
class _Solo(object):
    """the collectives of a run of one process"""
    rank, world, cdev = 0, 1, None

    def gather(self, obj, name):
        return [obj]


class _Ranks(object):
    def __init__(self, rank, world, cdev):
        self.rank, self.world, self.cdev = rank, world, cdev

    def gather(self, obj, name):
        from . import exchange
        return exchange.all_gather_object(obj, name="correct: " + name)


def _whole_text(path):
    from . import quorum
    return quorum._text_of(path)


def _count_records(text):
    """(records of a read file's text, offset of the first)"""
    import ctypes as C
    from . import _lib
    first, cnt, n_idx = C.c_uint64(), C.c_uint64(), C.c_uint64()
    B = len(text)
    _lib.check(_lib.lib().shn_text_records_in_range(text.ctypes.data if B else None, B, 0, B, 0, C.byref(first), C.byref(cnt), 1 << 62, None, 0, C.byref(n_idx)))
    return int(cnt.value), int(first.value)


def _skip(text, start, k):
    import ctypes as C
    from . import _lib
    off = C.c_uint64()
    _lib.check(_lib.lib().shn_text_skip_records(text.ctypes.data if len(text) else None, len(text), int(start), int(k), 0, C.byref(off)))
    return int(off.value)


def locate_lane(comm, paths, lane):
    """Where this rank's records [n r / W, n (r + 1) / W) of a lane's files lie: ([(path, a, b) per file], n records of the lane,
    index of the rank's first record).  By bytes of the files (distributed.ingest_rank_slice, a collective: every rank calls this for
    every lane, and what it raises every rank raises); files that cannot be shared out that way (.gz) are read whole on every rank
    and the records are located in the text (shn_text_skip_records).  One process: the whole files."""
    from . import _lib
    rank, world = comm.rank, comm.world
    if world > 1:
        from . import distributed
        spans = []
        try:
            sl = distributed.ingest_rank_slice(list(paths), rank, world, None, comm.cdev, ragged=True, text_spans=spans)
        except _lib.ShannonError as ex:
            if "different numbers of reads" in str(ex):
                raise CorrectError("lane %d: %s and %s are not mates of each other: %s" % (lane, paths[0], paths[-1], ex))
            raise
        if sl is not None:
            n = sl[1]
            return [(p, a, b) for p, (a, b) in zip(paths, spans)], n, rank * n // world
    where, counts = [], []
    for p in paths:
        text = _whole_text(p)
        try:
            n, first = _count_records(text) if len(text) else (0, 0)
        except _lib.ShannonError as ex:
            raise CorrectError("lane %d: %s: %s" % (lane, p, ex))
        counts.append(n)
        if world == 1:
            where.append((p, 0, len(text)))
        else:
            a = _skip(text, first, rank * n // world) if n else 0
            b = _skip(text, a, (rank + 1) * n // world - rank * n // world) if n else 0
            where.append((p, a, b))
        del text
    if len(counts) == 2 and counts[0] != counts[1]:
        raise _not_mates(lane, paths, counts[0], counts[1])
    return where, counts[0], rank * counts[0] // world


def open_lane(ctx, where, q):
    """the rank's records of a lane as resident sets with their high-quality masks, both from the same stretch of text:
    (sets, masks).  FASTA text raises CorrectError with the message of shn_reads_quality_mask ("needs FASTQ text")."""
    from . import device, quorum, _lib
    sets, masks = [], []
    try:
        for path, a, b in where:
            if b <= a:
                sets.append(device.Reads.from_strings(ctx, []))
                masks.append(None)
                continue
            text = _whole_text(path)[a:b]
            try:
                sets.append(device.Reads.ingest(ctx, text, want_codes=False)[0])
                masks.append(quorum.hq_mask(ctx, sets[-1], text, q))
            except _lib.ShannonError as ex:
                raise CorrectError("%s: %s" % (path, ex))
        if len(set(len(s) for s in sets)) != 1:
            raise CorrectError("%s and %s: %d and %d records in this rank's stretch" % (where[0][0], where[-1][0], len(sets[0]), len(sets[-1])))
    except Exception:
        close_all(sets, masks)
        raise
    return sets, masks


def close_all(*lists):
    for things in lists:
        for x in things:
            if x is not None:
                x.close()


# ------------------------------------------------------------------------------------------------------ the tables of all ranks
def replicate_table(ctx, table, k, comm):
    """The sum of all ranks' tables, the same on every rank: the pairs go to their owners (Table.shard, one all-to-all),
    the owners sum by key, the owned pairs are all-gathered and every rank builds the table.  A count is held at (2^32 - 1) // W
    before it travels, so an owner's 32-bit sum cannot wrap.  table: this rank's (None: it saw no read); it is closed."""
    import numpy as np
    import torch
    from . import device, exchange
    W = comm.world
    n = len(table) if table is not None else 0
    dk = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    dc = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    per = table.shard(W, dk.data_ptr(), dc.data_ptr()) if n else np.zeros(W, dtype=np.uint64)
    if table is not None:
        table.close()
    cap = ((1 << 32) - 1) // W                                       # (W >= 2: the cap fits a signed 32-bit number; a count of 2^31 or more reads as negative)
    dc = torch.where(dc < 0, torch.full_like(dc, cap), torch.clamp(dc, max=cap))
    rk, rcn, _ = exchange.all_to_all_pairs(dk[:n], dc[:n], per, name="correct: trusted k-mers to their owners (all-to-all)")
    torch.cuda.synchronize()
    owned = device.Table.from_pairs(ctx, rk.data_ptr() if rk.numel() else None, rcn.data_ptr() if rk.numel() else None, rk.numel(), k, True)
    del rk, rcn, dk, dc
    keys, cnts = owned.download()
    owned.close()
    got = exchange.all_gather_arrays((keys, cnts), comm.cdev, name="correct: the owners' trusted k-mers (all-gather)")
    gk = torch.from_numpy(np.concatenate([g[0] for g in got]).view(np.int64)).cuda()
    gc = torch.from_numpy(np.concatenate([g[1] for g in got]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return device.Table.from_pairs(ctx, gk.data_ptr() if gk.numel() else None, gc.data_ptr() if gk.numel() else None, gk.numel(), k, True)


def _empty_table(ctx, k):
    from . import device
    return device.Table.from_pairs(ctx, None, None, 0, k, True)


# --------------------------------------------------------------------------------------------------------------- the work
def run(o, ctx, comm=None, timings=None):
    """The command's work on one rank: pass 1 (the lanes' tables, added up; on N ranks summed and replicated), pass 2 (every lane
    corrected against the table, trimmed if asked, written).  Returns the summary dict on rank 0 (None elsewhere).  A rank whose
    own work fails goes on taking part in the collectives; all ranks raise CorrectError together.  timings (dict): seconds of
    "ingest 1", "mask", "table", "add tables", "replicate", "ingest 2", "correct", "trim", "write", "join"."""
    import time
    from . import quorum, _lib
    comm = comm or _Solo()
    rank, world = comm.rank, comm.world
    lanes = lanes_of(o)
    paired = "single" not in o
    names = FILES_PAIRED if paired else FILES_SINGLE
    k, out_dir = o["k"], o["out_dir"]
    T = timings if timings is not None else {}

    def lap(name, since):
        T[name] = T.get(name, 0.0) + time.time() - since
        return time.time()

    # ---- pass 1: the table of the sample
    err, running, located, lane_figs = None, None, [], []
    for i, paths in enumerate(lanes):
        where, n, first = locate_lane(comm, paths, i + 1)              # (what this raises, every rank raises)
        located.append((where, n, first))
        figs = [0, 0, 0]                                               # this rank's reads, high-quality bases, high-quality windows
        if err is None and any(b > a for _p, a, b in where):
            sets, masks, t = [], [], None
            try:
                t0 = time.time()
                sets, masks = open_lane(ctx, where, o["q"])
                t0 = lap("ingest 1 + mask", t0)
                t = quorum.trusted_table(ctx, sets, masks, k)
                t0 = lap("table", t0)
                figs = [sum(len(s) for s in sets), sum(m.n_hq for m in masks), t.total]
                if running is None:
                    running, t = t, None
                else:
                    both = quorum.add_tables(ctx, running, t)
                    running.close()
                    running = both
                lap("add tables", t0)
            except (CorrectError, _lib.ShannonError) as ex:
                err = "%slane %d: %s" % ("rank %d, " % rank if world > 1 else "", i + 1, ex)
            finally:
                close_all(sets, masks, [t])
        lane_figs.append(figs)
    try:
        errs = [e for e in comm.gather(err, "the ranks' status after pass 1") if e]
        if errs:
            raise CorrectError("; ".join(errs))
        t0 = time.time()
        if world > 1:
            table = replicate_table(ctx, running, k, comm)
        else:
            table = running if running is not None else _empty_table(ctx, k)
        running = None
        lap("replicate", t0)
    except Exception:
        if running is not None:
            running.close()
        raise
    try:
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
        comm.gather(None, "the output directory is there")
        # ---- pass 2: every lane corrected against the table
        stats = dict.fromkeys(quorum.STAT_NAMES, 0)
        tstats = dict.fromkeys(quorum.TRIM_NAMES, 0)
        written_before, parts, err = 0, [], None
        n_parts = len(lanes) * world
        for i, (where, n, first) in enumerate(located):
            sets, masks, fixed, spans, out = [], [], [], [], None
            n_mine = 0
            try:
                if err is None and any(b > a for _p, a, b in where):      # (a rank without a record of the lane writes empty parts)
                    t0 = time.time()
                    sets, masks = open_lane(ctx, where, o["q"])
                    close_all(masks)
                    masks = []
                    t0 = lap("ingest 2", t0)
                    for r in sets:
                        got = quorum.correct(ctx, r, table, k, o["anchor"], o["window"], o["errors"], spans=o["trim"])
                        fixed.append(got[0])
                        if o["trim"]:
                            spans.append(got[2])
                        for name in quorum.STAT_NAMES:
                            stats[name] += got[1][name]
                    t0 = lap("correct", t0)
                    out = fixed
                    if o["trim"]:
                        out, ts = quorum.trim(ctx, fixed, spans, o["min_len"])
                        for name in quorum.TRIM_NAMES:
                            tstats[name] += ts[name]
                        lap("trim", t0)
                    n_mine = len(out[0])
            except (CorrectError, _lib.ShannonError) as ex:
                err = "%slane %d: %s" % ("rank %d, " % rank if world > 1 else "", i + 1, ex)
                n_mine = 0
            # the names of this part's records go on from the records all earlier (lane, rank) parts wrote
            counts = [int(c) for c in comm.gather(n_mine, "records of the lane's parts")]
            e0 = written_before + sum(counts[:rank])
            written_before += sum(counts)
            try:
                if err is None:
                    t0 = time.time()
                    suffix = "" if n_parts == 1 else ".part.%d.%d" % (i, rank)
                    if out is None:
                        for nm in names:
                            open(os.path.join(out_dir, nm + suffix), "wb").close()
                    else:
                        quorum.write_fasta(ctx, out, out_dir, first_name=e0, suffix=suffix)
                    lap("write", t0)
            except (_lib.ShannonError, OSError) as ex:
                err = "%slane %d: %s" % ("rank %d, " % rank if world > 1 else "", i + 1, ex)
            finally:
                close_all(sets, masks, fixed, spans, out if out is not None and out is not fixed else [])
        tm, tb = ctx.timers(), ctx.timer_bytes()
    finally:
        table_size = len(table)
        table.close()
    everyone = comm.gather((err, lane_figs, stats, tstats), "the ranks' status and counters")
    errs = [e[0] for e in everyone if e[0]]
    status = None
    if rank == 0 and not errs:
        try:
            t0 = time.time()
            sizes = _join_parts(out_dir, names, len(lanes), world) if n_parts > 1 else {nm: os.path.getsize(os.path.join(out_dir, nm)) for nm in names}
            lap("join", t0)
            for e in everyone[1:]:
                for name in quorum.STAT_NAMES:
                    stats[name] += e[2][name]
                for name in quorum.TRIM_NAMES:
                    tstats[name] += e[3][name]
            figs = [[sum(e[1][i][j] for e in everyone) for j in range(3)] for i in range(len(lanes))]
            summary = dict(stats, table=table_size, windows=sum(f[2] for f in figs), hq_bases=sum(f[1] for f in figs), reads=sum(f[0] for f in figs),
                           records=written_before, files=sizes, paired=paired, ranks=world)
            if o["trim"]:
                summary.update(tstats)
            _write_log(o, lanes, figs, summary, tm, tb)
        except OSError as ex:
            status = "rank 0: %s" % ex
    if world > 1:
        status = comm.gather(status, "rank 0's status")[0]
    if errs or status:
        if rank == 0:
            _remove_outputs(out_dir)
        raise CorrectError("; ".join(errs) if errs else status)
    return summary if rank == 0 else None


def _join_parts(out_dir, names, n_lanes, world):
    """the (lane, rank) parts of every output file one after the other, in that order; the parts go.  {file name: bytes}"""
    import shutil
    sizes = {}
    for nm in names:
        with open(os.path.join(out_dir, nm), "wb") as dst:
            for i in range(n_lanes):
                for r in range(world):
                    part = os.path.join(out_dir, "%s.part.%d.%d" % (nm, i, r))
                    with open(part, "rb") as src:
                        shutil.copyfileobj(src, dst, 1 << 24)
                    os.remove(part)
            sizes[nm] = dst.tell()
    return sizes


def _remove_outputs(out_dir):
    """a refused run leaves nothing behind: what it wrote under out_dir goes, and out_dir if that empties it"""
    if not os.path.isdir(out_dir):
        return
    for f in os.listdir(out_dir):
        if f.startswith("corrected_reads") or f == "correct_log.txt":
            os.remove(os.path.join(out_dir, f))
    if not os.listdir(out_dir):
        os.rmdir(out_dir)


def counters_line(s):
    """the five counters as shannon.py's --quorum line words them"""
    return ("%d of %d reads anchored, %d changed, %d substitutions, %d stopped directions, %d window reverts"
            % (s["anchored"], s["reads"], s["changed"], s["substitutions"], s["stopped"], s["reverts"]))


def _write_log(o, lanes, figs, s, tm, tb):
    log = ["parameters: k %d, quality %d, anchor count %d, %d substitutions in a window of %d%s"
           % (o["k"], o["q"], o["anchor"], o["errors"], o["window"], ", trimmed with min_len %d" % o["min_len"] if o["trim"] else "")]
    for i, (paths, f) in enumerate(zip(lanes, figs)):
        log.append("lane %d: %s: %d reads, %d high-quality bases, %d high-quality windows" % (i + 1, " ".join(paths), f[0], f[1], f[2]))
    log.append("table: %d k-mers from %d high-quality windows" % (s["table"], s["windows"]))
    log.append("corrected: " + counters_line(s))
    if o["trim"]:
        log.append("trimmed: %d reads kept, %d of them trimmed, %d bases cut from kept reads, %d reads with a span below %d, %d pairs dropped"
                   % (s["kept"], s["trimmed"], s["bases_cut"], s["below_min"], o["min_len"], s["pairs_dropped"]))
    log.append("files: " + ", ".join("%s (%d bytes)" % (nm, s["files"][nm]) for nm in sorted(s["files"])) + "; %d records each" % s["records"])
    log.append("quorum kernels: " + json.dumps({k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)}
                                                 for k, v in sorted(tm.items()) if k.startswith("quorum.")}))
    with open(os.path.join(o["out_dir"], "correct_log.txt"), "w") as f:
        f.write("".join(l + "\n" for l in log))


def _say(s):
    print("corrected: %s; table of %d k-mers from %d high-quality windows%s; %s"
          % (counters_line(s), s["table"], s["windows"],
             "; trimmed: %d reads kept, %d pairs dropped" % (s["kept"], s["pairs_dropped"]) if "kept" in s else "", " ".join(sorted(s["files"]))))


# ---------------------------------------------------------------------------------------------------------------- N ranks
def launch_ranks(n, args):
    """start the n ranks as fresh child processes (quant.launch_ranks; the children run this module); this parent makes no GPU call"""
    import subprocess
    from . import quant
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SHN_CLI_RANKS="1")
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL between processes needs it on this stack
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(quant._free_port()), "-m", "shannon_amd.correct"] + list(args)
    return subprocess.call(cmd, env=env, cwd=os.getcwd())


def rank_main(o):
    """one rank of `--gpus N` (quant.rank_main's frame): the process group, this rank's context, run(); rank 0 prints"""
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("SHN_CLI_BACKEND") == "gloo"
    if os.environ.get("SHN_CLI_LAUNCH_PROBE"):
        # CPU test of the launch: the ranks meet over gloo, rank 0 says what the launch resolved to; nothing touches the GPU
        dist.init_process_group("gloo")
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        if rank == 0:
            print("launch probe: %d ranks met, %d %s lanes, k %d, trim %s, out=%s" % (int(one.item()), len(lanes_of(o)), "single-end" if "single" in o else "paired",
                                                                                      o["k"], o["min_len"] if o["trim"] else "off", o["out_dir"]))
        dist.destroy_process_group()
        return 0
    dev_index = 0 if share else local
    torch.cuda.set_device(dev_index)
    if share:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
    from . import device, exchange
    ctx = device.Context(dev_index)
    rc = 0
    try:
        ctx.timer_reset()
        s = run(o, ctx, _Ranks(rank, world, exchange.coll_device(torch.device("cuda", dev_index), None)))
        if rank == 0:
            _say(s)
    except CorrectError as ex:
        if rank == 0:
            sys.stderr.write("%s\n" % ex)
        rc = 2
    finally:
        ctx.close()
        dist.destroy_process_group()
    return rc


def main(argv):
    """python -m shannon_amd.correct ...; 0 done, 2 a usage error or a refused input (a message on stderr); with --gpus N > 1 the exit
    code of the ranks"""
    o = parse_args(argv)
    if isinstance(o, str):
        sys.stderr.write("%s\n%s" % (o, USAGE))
        return 2
    # ---- ranks.  Decided and started before anything touches the GPU (quant.main)
    if "WORLD_SIZE" in os.environ and "RANK" in os.environ and os.environ.get("SHN_CLI_RANKS") == "1":
        return rank_main(o)
    want = o.pop("gpus", 1)
    if want > 1:
        import torch
        have = torch.cuda.device_count()
        share = os.environ.get("SHN_CLI_BACKEND") == "gloo"       # (development / tests: several ranks on ONE GPU, collectives over gloo)
        ranks = want if share else min(want, max(1, have))
        if ranks < want:
            print("NOTE: --gpus %d asked for, the node shows %d GPU(s): %s" % (want, have, "%d ranks" % ranks if ranks > 1 else "one process"))
        if ranks > 1:
            return launch_ranks(ranks, argv[1:])
    from . import device
    ctx = device.Context(0)
    try:
        ctx.timer_reset()
        s = run(o, ctx)
    except CorrectError as ex:
        sys.stderr.write("%s\n" % ex)
        return 2
    finally:
        ctx.close()
    _say(s)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
