"""--compare: a finished assembly against a reference transcriptome (shannon.py:157-162, 620-622, 646-647; run_MB_SF_fn.py:283-302;
tester.py:135-167, 269-317).

The reference copies REF.fasta beside the assembly, runs BLAT of every known transcript against every reconstructed one
(parallel_blat_python.py -> reconstr_per.txt) and reads the PSL lines twice: tester.analyzer_blat_noExp (how much of every known
transcript its best reconstructed transcript recovers, how many come back to 90 %) and tester.false_positive (what every
reconstructed transcript matches).  Here BLAT is a stated rule run on the device (csrc/compare.hip,
shn_compare_rows); the two analyses are the reference's, made on the host from the rule's rows:

    records         (name, sequence) of a FASTA text as the rule reads it
    rows            the rule's rows for two record lists (the device call)
    psl_lines       the rows as the 21-column lines `blat -noHead` writes
    analyze         tester.analyzer_blat_noExp on such lines -> the text of reconstr_log.txt
    false_positive  tester.false_positive -> (the text of reconstr_rev_log.txt, rec, tot)
    compare_texts   the three texts of the comparison of two FASTA texts
    compare         the whole step on a finished output directory

    python -m shannon_amd.compare OUT REF.fasta [-s] [--chain]

--chain (chain=True): the chained form of the rule -- a pair's diagonals joined into one multi-block row (shn_compare_chains), so a
transcript that differs from the known one by a skipped exon or an indel is credited with all its pieces, as BLAT's lines are.

`records`, `psl_lines`, `analyze` and `false_positive` need neither the library nor a GPU."""
import collections
import ctypes as C
import os
import sys
import numpy as np

SEED = 16             # SHN_COMPARE_SEED: a pair of transcripts that shares no 16-mer is never looked at
MIN_MATCHES = 30      # SHN_COMPARE_MIN_MATCHES: BLAT's default -minScore

Rows = collections.namedtuple("Rows", "i j strand matches mismatches q_start q_end t_start")
Rows.__doc__ = """the rule's rows as eight uint32 arrays of one length, ordered by i, then j: query (reference transcript) and target
(reconstructed transcript) by their index in the record lists, strand 0 '+' / 1 '-', matches, mismatches, the segment on the query
[q_start, q_end) and where it starts on the target's forward strand"""


ChainRows = collections.namedtuple("ChainRows", Rows._fields + ("q_num_insert", "q_base_insert", "t_num_insert", "t_base_insert", "block_count", "block_off",
                                                               "block_size", "block_q_start", "block_t_start"))
ChainRows.__doc__ = """the chained rule's rows: Rows' eight columns -- matches and mismatches summed over the row's blocks, q_start of the first
block, q_end of the last, t_start of the whole chain on the target's forward strand -- then per row PSL's four gap columns and the
block count, and the blocks of all rows: row r's are block_off[r] .. block_off[r + 1] - 1 (uint64, rows + 1 entries), in chain
order, each with its size, where it starts on the query and where on the target's forward strand"""


def records(text):
    """[(name, sequence)] of a FASTA text in file order: a line that starts with '>' opens a record named by the first token behind
    the '>' ('' if there is none); the first tokens of the lines that follow, joined and upper-cased, are its sequence.  Blank lines
    and lines in front of the first header are skipped."""
    if not isinstance(text, str):
        text = bytes(text).decode()
    out = []
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0][0] == ">":
            out.append([t[0][1:], []])
        elif out:
            out[-1][1].append(t[0].upper())
    return [(name, "".join(parts)) for name, parts in out]


def _text_of(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    joined = "".join(seqs).encode()
    return (np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)), off


def rows(ctx, ref_records, rec_records, strand_specific=False, min_matches=MIN_MATCHES, stats=None, chain=False):
    """Rows of the reference transcripts ref_records (the queries) against the reconstructed ones rec_records (the targets), both
    [(name, sequence)]; strand_specific: the targets are taken forward only.  stats (a dict, optional) receives the call's
    counts: rows, candidates (diagonals scored), hits (16-mer hits at the start of a run), records (of the index).
    chain: the chained form -- a ChainRows; stats also receives blocks, groups ((query, target, orientation) triples chained) and
    multi_block_rows."""
    from . import _lib
    L = _lib.lib()
    q_text, q_off = _text_of([s for _n, s in ref_records])
    t_text, t_off = _text_of([s for _n, s in rec_records])
    h = C.c_void_p()
    _lib.check((L.shn_compare_chains if chain else L.shn_compare_rows)(ctx.h, q_text.ctypes.data, q_off.ctypes.data, len(ref_records), t_text.ctypes.data,
                                                                      t_off.ctypes.data, len(rec_records), 1 if strand_specific else 0, int(min_matches),
                                                                      C.byref(h)))
    try:
        sizes = np.zeros(4, dtype=np.uint64)
        _lib.check(L.shn_cmprows_sizes(h, sizes.ctypes.data))
        n = int(sizes[0])
        out = np.zeros((8, max(n, 1)), dtype=np.uint32)
        _lib.check(L.shn_cmprows_export(h, out.ctypes.data if n else None))
        if chain:
            csizes = np.zeros(3, dtype=np.uint64)
            _lib.check(L.shn_cmprows_chain_sizes(h, csizes.ctypes.data))
            nb = int(csizes[0])
            gaps = np.zeros((5, max(n, 1)), dtype=np.uint32)
            boff = np.zeros(n + 1, dtype=np.uint64)
            blocks = np.zeros((3, max(nb, 1)), dtype=np.uint32)
            _lib.check(L.shn_cmprows_chain_export(h, gaps.ctypes.data, boff.ctypes.data, blocks.ctypes.data))
    finally:
        L.shn_cmprows_destroy(h)
    if stats is not None:
        stats.update(rows=n, candidates=int(sizes[1]), hits=int(sizes[2]), records=int(sizes[3]))
        if chain:
            stats.update(blocks=nb, groups=int(csizes[1]), multi_block_rows=int(csizes[2]))
    if not chain:
        return Rows(*(out[f, :n].copy() for f in range(8)))
    return ChainRows(*([out[f, :n].copy() for f in range(8)] + [gaps[f, :n].copy() for f in range(5)] + [boff] + [blocks[f, :nb].copy() for f in range(3)]))


def psl_lines(r, ref_records, rec_records):
    """The rows as PSL lines without a head (no newline at their ends): matches, misMatches, six columns of 0 (repMatches, nCount,
    the four gap columns: a row is one ungapped block), strand, qName, qSize, qStart, qEnd, tName, tSize, tStart, tEnd, then the one
    block: blockCount 1, blockSizes, qStarts, tStarts.  A ChainRows gives multi-block lines: the gap columns as counted, tEnd where
    the chain's last base on the forward strand lies, blockCount and the three comma-terminated lists in chain order."""
    out = []
    if isinstance(r, ChainRows):
        cols = [a.tolist() for a in r]
        off, size, bq, bt = cols[13], cols[14], cols[15], cols[16]
        for k, (i, j, o, m, mm, q0, q1, t0, qn, qb, tn, tb, nb) in enumerate(zip(*cols[:13])):
            qn_, qs = ref_records[i]
            tn_, ts = rec_records[j]
            b = range(off[k], off[k + 1])
            t1 = max(bt[x] + size[x] for x in b)
            out.append("\t".join(str(x) for x in (m, mm, 0, 0, qn, qb, tn, tb, "-" if o else "+", qn_, len(qs), q0, q1, tn_, len(ts), t0, t1, nb,
                                                   "".join("%d," % size[x] for x in b), "".join("%d," % bq[x] for x in b),
                                                   "".join("%d," % bt[x] for x in b))))
        return out
    for i, j, o, m, mm, q0, q1, t0 in zip(*(a.tolist() for a in r)):
        qn, qs = ref_records[i]
        tn, ts = rec_records[j]
        out.append("\t".join(str(x) for x in (m, mm, 0, 0, 0, 0, 0, 0, "-" if o else "+", qn, len(qs), q0, q1, tn, len(ts), t0, t0 + q1 - q0, 1,
                                               "%d," % (q1 - q0), "%d," % q0, "%d," % t0)))
    return out


def analyze(lines):
    """tester.analyzer_blat_noExp (tester.py:135-167) on PSL lines: per reference transcript -- in the order of their first
    appearance in the lines -- the reconstructed transcript with the most matches (a later line takes over only with strictly
    more), as name, best target, matches, qSize, tSize; then the average of matches / qSize and the number of reference transcripts
    with matches >= 0.9 * qSize (the product in double).  The text of reconstr_log.txt; no newline behind its last line."""
    best = {}
    for line in lines:
        t = line.split()
        org, rec, rec_len, tr_len, rec_tr_len = t[9], t[13], int(t[0]), int(t[10]), int(t[14])
        if rec_len > best.get(org, [None, 0])[1]:
            best[org] = [rec, rec_len, tr_len, rec_tr_len]
    perf, n90, out = 0, 0, []
    for org, z in best.items():
        out.append("%s\t%s\t%s\t%s\t%s\n" % (org, z[0], z[1], z[2], z[3]))
        if z[1] >= 0.9 * z[2]:
            n90 += 1
        perf += float(z[1]) / float(z[2])
    if best:
        out.append("#Average fractional contig of transcripts retrived:\t" + str(perf / len(best)) + "\n")
    else:
        out.append("#Average fractional contig of transcripts retrived:\t" + str(perf) + "  best_rec=0\n")
    out.append("# of transcripts at greater than 90%:\t" + str(n90))
    return "".join(out)


def false_positive(rec_records, lines):
    """tester.false_positive (tester.py:269-317) on the reconstructed records and PSL lines: (the text of reconstr_rev_log.txt, rec,
    tot).  Per reconstructed transcript, in FASTA order: the line with the most matches (matchSize, qSize, tSize, qName) and the
    line with the greatest matchSize / qSize -- both with >=, so of equals the LAST line stays; a transcript no line names keeps 0, 0,
    its length and an empty name.  rec counts the transcripts with a line of matchSize >= 0.9 * min(qSize, tSize) (or * tSize), tot
    the headers.  A record without a sequence line has no entry but counts in tot; records of one name share an entry whose length
    is their sum.  A line that names a transcript without an entry is a KeyError, as there."""
    code, length, matches, att, att2, ratio = {}, {}, {}, {}, {}, {}
    tot = 0
    for name, seq in rec_records:
        tot += 1
        if not seq:
            continue
        length[name] = length.get(name, 0) + len(seq)
        code[name], matches[name], ratio[name] = 0, 0, 0
        att[name] = [0, 0, length[name], ""]
        att2[name] = [0, 0, length[name], ""]
    rec = 0
    for line in lines:
        t = line.strip().split()
        q_name, q_size, t_name, t_size, m = t[9], int(t[10]), t[13], int(t[14]), int(t[0])
        if m >= matches.get(t_name, 0):
            matches[t_name] = m
            att[t_name] = [m, q_size, t_size, q_name]
        if float(m) / float(q_size) >= ratio.get(t_name, 0):
            att2[t_name] = [m, q_size, t_size, q_name]
            ratio[t_name] = float(m) / float(q_size)
        if m >= 0.9 * min(q_size, t_size):
            if code[t_name] == 0:
                rec += 1
                code[t_name] = 1
        if m >= 0.9 * t_size:
            if code[t_name] == 0:
                rec += 1
            code[t_name] = 2
    out = ["\t".join(str(x) for x in [name] + att[name] + att2[name]) + "\n" for name in code]
    return "".join(out), rec, tot


class CompareError(Exception):
    """the output directory is not a finished run (exit code 2 of the command)"""


def compare_texts(ctx, ref_text, rec_text, strand_specific=False, chain=False):
    """The comparison of two FASTA texts: ({file name: text} for reconstr_per.txt, reconstr_log.txt and reconstr_rev_log.txt,
    {"rows", "candidates", "hits", "records", "rec", "tot"}; chain: the chained rule, and "blocks", "groups", "multi_block_rows")"""
    ref_records, rec_records = records(ref_text), records(rec_text)
    st = {}
    lines = psl_lines(rows(ctx, ref_records, rec_records, strand_specific, stats=st, chain=chain), ref_records, rec_records)
    rev, rec, tot = false_positive(rec_records, lines)
    st.update(rec=rec, tot=tot)
    return {"reconstr_per.txt": "".join(l + "\n" for l in lines), "reconstr_log.txt": analyze(lines), "reconstr_rev_log.txt": rev}, st


def compare(out_dir, ref_fasta, strand_specific=False, ctx=None, chain=False):
    """The reference's comparison on a finished output directory OUT (shannon.py:620-622, 646-647; run_MB_SF_fn.py:283-302):
    OUT/shannon.fasta against ref_fasta.  Writes, under OUT/TEMP/<sample>_allalgo_output/, reference.fasta (a copy of ref_fasta),
    reconstr_per.txt (the PSL lines), reconstr_log.txt and reconstr_rev_log.txt, and OUT/compare_log.txt (reconstr_log.txt once
    more: the reference moves it there last); prints `rec,tot` as tester.py:313 does.  Nothing else of OUT changes.
    Returns {"rows", "candidates", "hits", "records", "rec", "tot", "log"}.  A missing OUT/shannon.fasta raises CompareError.
    chain: the chained rule -- the same files under the same content rules from multi-block lines, and one more line printed in front
    of `rec,tot`: how many rows hold more than one block."""
    from . import device
    final = os.path.join(out_dir, "shannon.fasta")
    if not os.path.isfile(final):
        raise CompareError("%s: no such file -- --compare works on the output directory of a finished run" % final)
    with open(ref_fasta) as f:
        ref_text = f.read()
    with open(final) as f:
        rec_text = f.read()
    own = ctx is None
    if own:
        ctx = device.Context(0)
    try:
        texts, st = compare_texts(ctx, ref_text, rec_text, strand_specific, chain)
    finally:
        if own:
            ctx.close()
    sample = os.path.basename(os.path.normpath(os.path.abspath(out_dir)))
    alld = os.path.join(out_dir, "TEMP", sample + "_allalgo_output")
    os.makedirs(alld, exist_ok=True)
    for name, text in [("reference.fasta", ref_text)] + sorted(texts.items()):
        with open(os.path.join(alld, name), "w") as f:
            f.write(text)
    with open(os.path.join(out_dir, "compare_log.txt"), "w") as f:
        f.write(texts["reconstr_log.txt"])
    if chain:
        print("rows with more than one block: %d of %d" % (st["multi_block_rows"], st["rows"]))
    print("%d,%d" % (st["rec"], st["tot"]))
    st["log"] = texts["reconstr_log.txt"]
    return st


def main(argv):
    """python -m shannon_amd.compare OUT REF.fasta [-s] [--chain]; 0 done, 2 usage or an OUT that is no finished run"""
    args = [a for a in argv[1:] if a not in ("-s", "--chain")]
    if len(args) != 2 or any(a.startswith("-") for a in args):
        sys.stderr.write("usage: python -m shannon_amd.compare OUT REF.fasta [-s] [--chain]\n"
                         "  OUT        the output directory of a finished run (holds shannon.fasta)\n"
                         "  REF.fasta  the known transcripts\n"
                         "  -s         the run was strand-specific: no reverse complements\n"
                         "  --chain    join a pair's diagonals into one multi-block line (skipped exons, indels)\n")
        return 2
    if not os.path.isfile(args[1]):
        sys.stderr.write("%s: no such file\n" % args[1])
        return 2
    try:
        compare(args[0], args[1], strand_specific="-s" in argv[1:], chain="--chain" in argv[1:])
    except CompareError as ex:
        sys.stderr.write("%s\n" % ex)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
