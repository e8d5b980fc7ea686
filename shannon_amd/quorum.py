"""--quorum: quality-aware read error correction in front of the counting (shannon.py:289-299, 385-391).

The reference runs Quorum on every FASTQ input and hands corrected_reads*.fa to everything but kallisto.  Here Quorum is a stated
rule run on the device (csrc/quorum.hip, the quality bits by csrc/ingest.hip):

    hq_mask        the quality lines of a FASTQ text as one resident bit per base of its read set (shn_reads_quality_mask)
    trusted_table  the canonical k-mers of all high-quality windows of the run's read sets, with counts (shn_quorum_table)
    correct        a NEW resident read set with the substitutions of the rule, and the five counters (shn_quorum_correct)
    apply          the whole step on the read sets of a run: corrected sets, corrected host codes for kfc.ReadStore, stats
    write_fasta    corrected_reads*.fa from the device, through the record formatter of --inDisk

and what the command python -m shannon_amd.correct adds:

    add_tables     the key-wise sum of two trusted tables: the table of a sample is the sum of its lanes' (its ranks') tables
    correct(.., spans=True)  also the span [lo, hi) of every read that its walks vouch for (rule 6; shn_quorum_correct_spans)
    trim           rule 7: the kept reads (pairs) cut to their spans as NEW resident sets, and the five counters (shn_reads_slice)

The defaults are Quorum's documented ones (k = 24, quality 5, anchor count 3) and its "3 errors in a window of 10"."""
import ctypes as C
import os
import time
import numpy as np
from . import _lib, device

K, MIN_QUALITY, ANCHOR_COUNT, WINDOW, MAX_SUBS = 24, 5, 3, 10, 3
STAT_NAMES = ("anchored", "changed", "substitutions", "stopped", "reverts")
TRIM_NAMES = ("kept", "trimmed", "bases_cut", "below_min", "pairs_dropped")
COUNT_CAP = (1 << 31) - 1           # what a count is held at before two tables are added (shn_quorum_add_tables)


class QMask(object):
    """the high-quality bits of a read set, resident (one bit per base, in the layout of the set's mask of bases outside ACGT)"""

    def __init__(self, ctx, h, reads):
        self.ctx, self.h, self.reads = ctx, h, reads         # (the set is kept alive: the mask names it)

    @property
    def n_hq(self):
        return int(_lib.lib().shn_qmask_n_hq(self.h))

    def download(self):
        """the mask's 64-bit words (uint64; 64 bases per word, the first base in the highest bit, every read on its own word)"""
        out = np.zeros(max(int(_lib.lib().shn_qmask_n_words(self.h)), 1), dtype=np.uint64)
        _lib.check(_lib.lib().shn_qmask_download(self.ctx.h, self.h, out.ctypes.data))
        return out[:int(_lib.lib().shn_qmask_n_words(self.h))]

    def close(self):
        if self.h:
            _lib.lib().shn_qmask_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _text_of(source):
    if isinstance(source, str):
        if source.endswith(".gz"):
            import gzip
            with gzip.open(source, "rb") as f:
                return np.frombuffer(f.read(), dtype=np.uint8)
        return np.memmap(source, dtype=np.uint8, mode="r") if os.path.getsize(source) else np.zeros(0, np.uint8)
    if isinstance(source, (bytes, bytearray, memoryview)):
        return np.frombuffer(source, dtype=np.uint8)
    return np.ascontiguousarray(source, dtype=np.uint8)


def hq_mask(ctx, reads, source, min_quality=MIN_QUALITY, fmt=0):
    """QMask of `reads` (device.Reads) from the FASTQ text it was ingested from (a path, .gz too, or the text as bytes / uint8).
    FASTA text, or text whose records are not those of the set, raises ShannonError."""
    text = _text_of(source)
    h = C.c_void_p()
    _lib.check(_lib.lib().shn_reads_quality_mask(ctx.h, reads.h, text.ctypes.data if len(text) else None, len(text), int(fmt), int(min_quality),
                                                 C.byref(h)))
    return QMask(ctx, h, reads)


def trusted_table(ctx, read_sets, masks, k=K):
    """device.Table of can(w) of every high-quality window of every read of read_sets (rule 1); masks[i] belongs to read_sets[i]"""
    if len(read_sets) != len(masks):
        raise ValueError("trusted_table: %d read sets, %d masks" % (len(read_sets), len(masks)))
    sets = (C.c_void_p * max(len(read_sets), 1))(*[r.h for r in read_sets])
    ms = (C.c_void_p * max(len(masks), 1))(*[m.h for m in masks])
    h = C.c_void_p()
    _lib.check(_lib.lib().shn_quorum_table(ctx.h, sets, ms, len(read_sets), int(k), C.byref(h)))
    return device.Table(ctx, h)


def add_tables(ctx, a, b):
    """a NEW device.Table: the key-wise sum of two trusted tables of one k (c(x) of rule 1 is a sum over reads, so the table of a
    sample is the sum of its parts' tables).  Counts are held at COUNT_CAP before they are added -- the rule reads c >= 1 and c >= A
    only, and a 32-bit sum must not wrap; `total` is the 64-bit sum of the two totals.  a and b stay as they are."""
    h = C.c_void_p()
    _lib.check(_lib.lib().shn_quorum_add_tables(ctx.h, a.h, b.h, C.byref(h)))
    return device.Table(ctx, h)


class QSpans(object):
    """per read of a set the span [lo, hi) its walks vouch for (rule 6), resident"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    @classmethod
    def from_array(cls, ctx, lo_hi):
        """from a host array [n, 2] of (lo, hi)"""
        a = np.ascontiguousarray(lo_hi, dtype=np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        _lib.check(_lib.lib().shn_qspans_create(ctx.h, a.ctypes.data if len(a) else None, len(a), C.byref(h)))
        return cls(ctx, h)

    def __len__(self):
        return int(_lib.lib().shn_qspans_count(self.h))

    def download(self):
        """uint32 [n, 2]: (lo, hi) of every read"""
        out = np.zeros((max(len(self), 1), 2), dtype=np.uint32)
        _lib.check(_lib.lib().shn_qspans_download(self.ctx.h, self.h, out.ctypes.data))
        return out[:len(self)]

    def close(self):
        if self.h:
            _lib.lib().shn_qspans_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def correct(ctx, reads, table, k=K, anchor_count=ANCHOR_COUNT, window=WINDOW, max_subs=MAX_SUBS, spans=False):
    """(a new device.Reads with the rule's substitutions, {counter: value}); `reads` stays resident and unchanged.  spans=True: a
    third value, the QSpans of the reads (rule 6) -- the corrected set and the counters are those of the call without it."""
    h = C.c_void_p()
    st = np.zeros(5, dtype=np.uint64)
    if spans:
        sp = C.c_void_p()
        _lib.check(_lib.lib().shn_quorum_correct_spans(ctx.h, reads.h, table.h, int(k), int(anchor_count), int(window), int(max_subs), C.byref(h),
                                                       C.byref(sp), st.ctypes.data))
        return device.Reads(ctx, h, fixed_len=reads.fixed_len), dict(zip(STAT_NAMES, (int(v) for v in st))), QSpans(ctx, sp)
    _lib.check(_lib.lib().shn_quorum_correct(ctx.h, reads.h, table.h, int(k), int(anchor_count), int(window), int(max_subs), C.byref(h),
                                             st.ctypes.data))
    return device.Reads(ctx, h, fixed_len=reads.fixed_len), dict(zip(STAT_NAMES, (int(v) for v in st)))


def slice_reads(ctx, reads, spans, keep=None):
    """a NEW ragged device.Reads: bases [lo, hi) of every read of `reads` (keep: a handle of shn_qspans_keep -- of the kept ones only),
    in order (shn_reads_slice); `reads` stays as it is"""
    h = C.c_void_p()
    _lib.check(_lib.lib().shn_reads_slice(ctx.h, reads.h, spans.h, keep, C.byref(h)))
    return device.Reads(ctx, h)


def trim(ctx, sets, spans, min_len=K):
    """rule 7 on one set, or on the two mate sets of a run: (new resident sets of the kept reads cut to their spans, {counter:
    value} for TRIM_NAMES).  A read is kept when its span holds min_len bases or more, a pair when both mates are; the new sets are
    ragged and stay aligned read for read.  sets and spans stay as they are."""
    if len(sets) not in (1, 2) or len(sets) != len(spans):
        raise ValueError("trim: %d read sets, %d span arrays" % (len(sets), len(spans)))
    keep = C.c_void_p()
    st = np.zeros(5, dtype=np.uint64)
    paired = len(sets) == 2
    _lib.check(_lib.lib().shn_qspans_keep(ctx.h, sets[0].h, spans[0].h, sets[1].h if paired else None, spans[1].h if paired else None, int(min_len),
                                          C.byref(keep), st.ctypes.data))
    out = []
    try:
        for r, sp in zip(sets, spans):
            out.append(slice_reads(ctx, r, sp, keep))
    except Exception:
        for c in out:
            c.close()
        raise
    finally:
        _lib.lib().shn_qkeep_destroy(keep)
    return out, dict(zip(TRIM_NAMES, (int(v) for v in st)))


def host_codes(reads, like=None):
    """the reads of a resident set as the ingest leaves them on the host: a code matrix [n, L] for a set of one known length,
    device.RaggedCodes otherwise (`like`: the host codes of the set this one was corrected from -- their kind is kept)"""
    n = len(reads)
    codes, off = device.Reads.collect(reads, None, np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
    if isinstance(like, device.RaggedCodes) or reads.fixed_len is None:
        return device.RaggedCodes(codes, off)
    return np.ascontiguousarray(codes.reshape(n, reads.fixed_len))


def apply(ctx, read_sets, sources, host=None, k=K, min_quality=MIN_QUALITY, anchor_count=ANCHOR_COUNT, window=WINDOW, max_subs=MAX_SUBS,
          timings=None):
    """The step on the read sets of a run (one set, or the two mates): (corrected sets, corrected host codes, stats).
    sources[i]: the FASTQ text (or path) of read_sets[i]; host[i]: the host codes of read_sets[i] as the ingest gave them (their
    kind -- matrix or RaggedCodes -- is the kind of the corrected ones).  The originals stay resident and unchanged (they are what
    --kallisto_cutoff quantifies against).  stats: the five counters summed over the sets, "table" (distinct k-mers), "windows"
    (high-quality windows), "hq_bases"; the time under timings["quorum"], its four parts under "quorum: mask" (the quality lines,
    parsed on the host), "quorum: table", "quorum: correct" and "quorum: host codes" (the corrected reads back on the host)."""
    t0 = time.time()
    masks, out = [], []
    table = None
    T = timings if timings is not None else {}

    def lap(name, since):
        T["quorum: " + name] = T.get("quorum: " + name, 0.0) + time.time() - since
        return time.time()
    try:
        t = t0
        for r, src in zip(read_sets, sources):
            masks.append(hq_mask(ctx, r, src, min_quality))
        t = lap("mask", t)
        table = trusted_table(ctx, read_sets, masks, k)
        t = lap("table", t)
        stats = dict.fromkeys(STAT_NAMES, 0)
        stats.update(table=len(table), windows=table.total, hq_bases=sum(m.n_hq for m in masks))
        for r in read_sets:
            c, st = correct(ctx, r, table, k, anchor_count, window, max_subs)
            out.append(c)
            for name in STAT_NAMES:
                stats[name] += st[name]
        t = lap("correct", t)
        codes = [host_codes(c, host[i] if host is not None else None) for i, c in enumerate(out)]
        lap("host codes", t)
    except Exception:
        for c in out:
            c.close()
        raise
    finally:
        for m in masks:
            m.close()
        if table is not None:
            table.close()
    if timings is not None:
        timings["quorum"] = timings.get("quorum", 0.0) + time.time() - t0
    return out, codes, stats


def write_fasta(ctx, read_sets, out_dir, first_name=0, suffix=""):
    """corrected_reads_1.fa + corrected_reads_2.fa (one set: corrected_reads.fa) under out_dir, all reads in order, formatted on the
    device by the record formatter of --inDisk (record i named first_name + i, the mates _1 / _2); returns {file name: bytes}.
    suffix: appended to the file names on disk (a part of a file that the caller puts together), not to the names returned."""
    from . import kmers_for_component as kfc
    n = len(read_sets[0])
    paired = len(read_sets) == 2
    if n == 0:                                                  # (no record: nothing for the device to format)
        names = ("corrected_reads_1.fa", "corrected_reads_2.fa") if paired else ("corrected_reads.fa",)
        for name in names:
            open(os.path.join(out_dir, name + suffix), "wb").close()
        return dict.fromkeys(names, 0)
    # a route d < n names read d of the first set as it is, n + d read d of the second set as it is (the doubled mode's table)
    routes = kfc.Routes.from_arrays(ctx, np.zeros(2 * n if paired else n, np.uint32), np.arange(2 * n if paired else n, dtype=np.uint32),
                                    reads=(read_sets[0], read_sets[1] if paired else None))
    got = {}
    try:
        if paired:
            got["corrected_reads_1.fa"] = routes.fasta_file(os.path.join(out_dir, "corrected_reads_1.fa" + suffix), 0, n, kfc.READS_DOUBLED, 1, first_name)
            got["corrected_reads_2.fa"] = routes.fasta_file(os.path.join(out_dir, "corrected_reads_2.fa" + suffix), n, n, kfc.READS_DOUBLED, 2, first_name)
        else:
            got["corrected_reads.fa"] = routes.fasta_file(os.path.join(out_dir, "corrected_reads.fa" + suffix), 0, n, kfc.READS_DOUBLED, 0, first_name)
    finally:
        routes.close()
    return got
