"""--filter_FP: drop the transcripts of a partition that its read pairs do not cover (filter_FP.py, run_MB_SF_fn.py:110,
272-277; shannon.py:170-195).

The reference maps a partition's pairs onto its reconstructed.fasta with `hisat --no-spliced-alignment --no-discordant`, keeps
the properly paired alignments (`samtools view -f 0x2`), and write_filtered_tr (filter_FP.py:7-25) keeps a transcript when at
least 90 % of its bases have depth.  Here the aligner is a stated rule ("filter_FP") run on the device for all
partitions at once (csrc/filter_fp.hip, shn_filter_fp_hits); the decision and the three products -- reconstructed.fasta,
reconstructed_org.fasta, rec.log -- are the reference's, made on the host:

    coverage_hits   covered bases of every transcript (the device call)
    decide          filter_FP.py:23, in IEEE double as written there
    filter_text     one partition's FASTA text + hits -> (kept FASTA text, rec.log text)
    filter_texts    the partitions' texts -> [(kept text, log text)] through one device call

`decide`, `records` and `filter_text` need neither the library nor a GPU.
"""
import numpy as np

THRESH = 0.9          # filter_FP.py:10
MAX_SPAN = 500        # hisat's default -X (maximum fragment length of a concordant pair); SHN_FILTER_FP_MAX_SPAN
SEED = 15             # seed length of the mapping (SHN_FILTER_FP_SEED): a read shorter than this is never placed


def decide(hits, lens):
    """filter_FP.py:23 -- keep transcript j iff hits[j] >= lens[j] * 0.9, the product evaluated in double."""
    return [int(h) >= int(n) * THRESH for h, n in zip(hits, lens)]


def _as_str(text):
    if isinstance(text, str):
        return text
    return bytes(text).decode()


def records(text):
    """(names, sequences) of a FASTA text as write_filtered_tr reads it (filter_FP.py:18-21): a line whose first token starts
    with '>' names what follows (the token without the '>'), the first token of every other line is a sequence of its own."""
    names, seqs, name = [], [], ""
    for line in _as_str(text).split("\n"):
        fields = line.strip().split()
        if not fields:
            continue
        if fields[0][0] == ">":
            name = fields[0][1:]
            continue
        names.append(name)
        seqs.append(fields[0])
    return names, seqs


def filter_text(text, hits):
    """One partition: (kept FASTA text, rec.log text) -- what write_filtered_tr (filter_FP.py:7-25) writes to out_tr_file and
    log_file when transcript j has hits[j] lines in the depth file.  A kept record is '>' + first token of its header + the
    sequence; the log holds name, hits, length of every transcript, tab separated."""
    return _filter_records(*records(text), hits=hits)


def _filter_records(names, seqs, hits):
    if len(hits) != len(seqs):
        raise ValueError("filter_text: %d hit counts for %d transcripts" % (len(hits), len(seqs)))
    keep = decide(hits, [len(s) for s in seqs])
    out, log = [], []
    for name, seq, h, k in zip(names, seqs, hits, keep):
        log.append("%s\t%d\t%d\n" % (name, int(h), len(seq)))
        if k:
            out.append(">%s\n%s\n" % (name, seq))
    return "".join(out), "".join(log)


def coverage_hits(ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span=MAX_SPAN, stats=None):
    """hits[j] = bases of transcript j covered by the best concordant placements of the pairs routed to partition part_of[j].
    seqs: the transcripts (str); d1 / d2: device.Reads of the mates as the user gave them; routes: a
    kmers_for_component.Routes (the routing's result on the device) or (partition ids, fragment / doubled read indices) on the
    host.  A transcript shorter than SEED bases cannot hold a read and is handed over empty (its hits are 0 whatever it is made
    of -- the header quirk record `Bases` of the single nodes is one); any other transcript must be ACGT.
    stats (a dict, optional) receives routes looked at / fragments placed."""
    from . import _lib
    seqs = [s if len(s) >= SEED else "" for s in seqs]
    n_tr = len(seqs)
    t_off = np.zeros(n_tr + 1, dtype=np.uint64)
    if n_tr:
        t_off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    joined = "".join(seqs).encode()
    text = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)
    t_part = np.ascontiguousarray(part_of, dtype=np.uint32) if n_tr else np.zeros(1, np.uint32)
    if n_tr and len(t_part) != n_tr:
        raise ValueError("coverage_hits: part_of has %d entries for %d transcripts" % (len(t_part), n_tr))
    hits = np.zeros(max(n_tr, 1), dtype=np.uint32)
    st = np.zeros(2, dtype=np.uint64)
    if hasattr(routes, "h"):
        rh, pid, frag, n_host = routes.h, None, None, 0
    else:
        pid = np.ascontiguousarray(routes[0], dtype=np.uint32)
        frag = np.ascontiguousarray(routes[1], dtype=np.uint32)
        if len(pid) != len(frag):
            raise ValueError("coverage_hits: the two columns of the routes differ in length")
        rh, n_host = None, len(pid)
    _lib.check(_lib.lib().shn_filter_fp_hits(ctx.h, text.ctypes.data, t_off.ctypes.data, t_part.ctypes.data, n_tr, int(n_parts), d1.h, d2.h, rh,
                                             pid.ctypes.data if n_host else None, frag.ctypes.data if n_host else None, n_host,
                                             1 if strand_specific else 0, int(max_span), hits.ctypes.data, st.ctypes.data))
    if stats is not None:
        stats["routes"] = stats.get("routes", 0) + int(st[0])
        stats["placed"] = stats.get("placed", 0) + int(st[1])
    return hits[:n_tr]


def filter_texts(ctx, texts, d1, d2, routes, strand_specific, max_span=MAX_SPAN, stats=None):
    """texts[p] = the FASTA text of partition p (str, bytes or a uint8 array; p = the partition id of the routes).  One device
    call for all partitions; returns [(kept text, log text)] in the same order.  stats: see coverage_hits, plus transcripts
    kept / total."""
    parsed = [records(t) for t in texts]
    seqs, part_of = [], []
    for p, (_names, ss) in enumerate(parsed):
        seqs += ss
        part_of += [p] * len(ss)
    hits = coverage_hits(ctx, seqs, part_of, len(texts), d1, d2, routes, strand_specific, max_span, stats)
    out, at = [], 0
    for names, ss in parsed:
        out.append(_filter_records(names, ss, hits[at:at + len(ss)].tolist()))
        at += len(ss)
    if stats is not None:
        stats["transcripts"] = stats.get("transcripts", 0) + len(seqs)
        stats["kept"] = stats.get("kept", 0) + sum(o[0].count(">") for o in out)
    return out
