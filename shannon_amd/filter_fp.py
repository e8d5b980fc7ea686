"""--filter_FP: drop the transcripts of a partition that its read pairs do not cover (filter_FP.py, run_MB_SF_fn.py:110,
272-277; shannon.py:170-195).

The reference maps a partition's pairs onto its reconstructed.fasta with `hisat --no-spliced-alignment --no-discordant`, keeps
the properly paired alignments (`samtools view -f 0x2`), and write_filtered_tr (filter_FP.py:7-25) keeps a transcript when at
least 90 % of its bases have depth.  Here the aligner is a stated rule ("filter_FP") run on the device for all
partitions at once (csrc/filter_fp.hip, shn_filter_fp_hits); the decision and the three products -- reconstructed.fasta,
reconstructed_org.fasta, rec.log -- are the reference's, made on the host:

    coverage_hits   covered bases of every transcript (the device call)
    coverage_bitmap / hits_from_bitmaps   its two halves, for routes that lie on several ranks (distributed.filter_owned_texts)
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


def _prepare(seqs, part_of, routes, who):
    """What both device calls take: the transcripts one after the other (one shorter than SEED bases handed over empty), t_off,
    t_part, and the routes as a handle or as two host columns -> (text, t_off, t_part, n_tr, routes handle, pid, frag, n_host)."""
    seqs = [s if len(s) >= SEED else "" for s in seqs]
    n_tr = len(seqs)
    t_off = np.zeros(n_tr + 1, dtype=np.uint64)
    if n_tr:
        t_off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    joined = "".join(seqs).encode()
    text = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)
    t_part = np.ascontiguousarray(part_of, dtype=np.uint32) if n_tr else np.zeros(1, np.uint32)
    if n_tr and len(t_part) != n_tr:
        raise ValueError("%s: part_of has %d entries for %d transcripts" % (who, len(t_part), n_tr))
    if hasattr(routes, "h"):
        rh, pid, frag, n_host = routes.h, None, None, 0
    else:
        pid = np.ascontiguousarray(routes[0], dtype=np.uint32)
        frag = np.ascontiguousarray(routes[1], dtype=np.uint32)
        if len(pid) != len(frag):
            raise ValueError("%s: the two columns of the routes differ in length" % who)
        rh, n_host = None, len(pid)
    return text, t_off, t_part, n_tr, rh, pid, frag, n_host


def _device_call(fn, ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span, stats, out_of, who):
    from . import _lib
    text, t_off, t_part, n_tr, rh, pid, frag, n_host = _prepare(seqs, part_of, routes, who)
    out = out_of(n_tr, t_off)
    st = np.zeros(2, dtype=np.uint64)
    _lib.check(getattr(_lib.lib(), fn)(ctx.h, text.ctypes.data, t_off.ctypes.data, t_part.ctypes.data, n_tr, int(n_parts), d1.h, d2.h, rh,
                                       pid.ctypes.data if n_host else None, frag.ctypes.data if n_host else None, n_host,
                                       1 if strand_specific else 0, int(max_span), out.ctypes.data, st.ctypes.data))
    if stats is not None:
        stats["routes"] = stats.get("routes", 0) + int(st[0])
        stats["placed"] = stats.get("placed", 0) + int(st[1])
    return out, n_tr, t_off


def coverage_hits(ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span=MAX_SPAN, stats=None):
    """hits[j] = bases of transcript j covered by the best concordant placements of the pairs routed to partition part_of[j].
    seqs: the transcripts (str); d1 / d2: device.Reads of the mates as the user gave them; routes: a
    kmers_for_component.Routes (the routing's result on the device) or (partition ids, fragment / doubled read indices) on the
    host.  A transcript shorter than SEED bases cannot hold a read and is handed over empty (its hits are 0 whatever it is made
    of -- the header quirk record `Bases` of the single nodes is one); any other transcript must be ACGT.
    stats (a dict, optional) receives routes looked at / fragments placed."""
    hits, n_tr, _t_off = _device_call("shn_filter_fp_hits", ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span, stats,
                                      lambda n_tr, t_off: np.zeros(max(n_tr, 1), dtype=np.uint32), "coverage_hits")
    return hits[:n_tr]


def text_offsets(seqs):
    """t_off of the layout coverage_bitmap marks: the transcripts one after the other, one shorter than SEED bases empty"""
    t_off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        t_off[1:] = np.cumsum([len(s) if len(s) >= SEED else 0 for s in seqs], dtype=np.uint64)
    return t_off


def coverage_bitmap(ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span=MAX_SPAN, stats=None):
    """The first half of coverage_hits for a share of the routes (shn_filter_fp_cover): one bit per base of the text laid out by
    text_offsets(seqs) -- bit g & 63 of word g >> 6 is set iff base g lies under a best concordant placement of a fragment THESE
    routes name.  The OR of the bitmaps of all shares of a job's routes, counted by hits_from_bitmaps, is coverage_hits of the
    job: a fragment's placements depend on the fragment and its partition's transcripts alone.  Arguments as coverage_hits."""
    cover, _n_tr, t_off = _device_call("shn_filter_fp_cover", ctx, seqs, part_of, n_parts, d1, d2, routes, strand_specific, max_span, stats,
                                       lambda n_tr, t_off: np.zeros(max((int(t_off[-1]) + 63) // 64, 1), dtype=np.uint64), "coverage_bitmap")
    return cover[:(int(t_off[-1]) + 63) // 64]


def hits_from_bitmaps(ctx, covers, t_off, word0=0):
    """hits[j] = bits set among the bases [t_off[j], t_off[j + 1]) in the OR of the bitmaps covers[c] (2-D uint64, one bitmap a row);
    row word w holds the text positions 64 (word0 + w) .. + 63, t_off is absolute and every transcript lies inside the rows' window.
    Bits of the first and last word that belong to neighbours outside [t_off[0], t_off[-1]) are not counted.
    ctx: a device.Context (shn_filter_fp_count) or None: the same in numpy, the mirror the tests hold the kernel against."""
    covers = np.ascontiguousarray(covers, dtype=np.uint64)
    if covers.ndim != 2:
        raise ValueError("hits_from_bitmaps: covers must be 2-D (one bitmap a row), got %d-D" % covers.ndim)
    t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
    n_tr = len(t_off) - 1
    n_covers, n_words = covers.shape
    if ctx is not None:
        from . import _lib
        hits = np.zeros(max(n_tr, 1), dtype=np.uint32)
        _lib.check(_lib.lib().shn_filter_fp_count(ctx.h, covers.ctypes.data if covers.size else None, n_covers, n_words, int(word0),
                                                  t_off.ctypes.data, n_tr, hits.ctypes.data))
        return hits[:n_tr]
    if n_covers == 0 or int(t_off.min()) < 64 * word0 or int(t_off.max()) > 64 * (word0 + n_words):
        raise ValueError("hits_from_bitmaps: no bitmap, or a transcript outside the window of the bitmaps")
    bits = np.unpackbits(np.bitwise_or.reduce(covers, axis=0).view(np.uint8), bitorder="little")        # (bit g - 64 word0 = base g)
    rel = (t_off - np.uint64(64 * word0)).astype(np.int64)
    return np.array([int(bits[rel[j]:rel[j + 1]].sum()) for j in range(n_tr)], dtype=np.uint32)


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
