"""python -m shannon_amd.correct: the brute force of rules 6 and 7 and of the rules they stand on (3.11, rules 2-5),
in plain Python over strings and lists, and the inputs of the tests.

Written from the rules' text and on its own: quorum_cases.brute_correct walks a read to the right and to the left; here there is ONE
walk, to the right, and the leftward direction is that walk on the read's reverse complement (the table holds canonical k-mers, so
"x is in the table" does not change under reverse complement; a substitution of c at base p is the substitution of its complement at
base L - 1 - p).  tests/test_correct.py holds the two against each other on every scenario.

A read is (bases, qualities); a table is {canonical k-mer: count} (quorum_cases.brute_table: rule 1 is not repeated here)."""
import os
import random

import quorum_cases as qc

ACGT = "ACGT"
TRIM_NAMES = ("kept", "trimmed", "bases_cut", "below_min", "pairs_dropped")


def rc_n(s):
    """reverse complement of a string over ACGTN"""
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def walk_right(seq, start, k, table, w, e):
    """Rules 3 and 4 from the anchor window seq[start:start + k] to the right.  Returns (steps vouched for, {position: new base},
    stopped 0/1, reverted 0/1, the positions set back).  Step d looks at base start + k + d of the read as it was."""
    def present(x):
        return table.get(min(x, qc.revcomp(x)), 0) >= 1
    cur = seq[start:start + k]
    n_steps = len(seq) - start - k
    subs = []                                                    # (step, position, new base), in place so far
    for d in range(n_steps):
        p = start + k + d
        r = seq[p]
        if r in ACGT and present(cur[1:] + r):
            cur = cur[1:] + r
            continue
        cand = [c for c in ACGT if c != r and present(cur[1:] + c)]
        if len(cand) > 1:
            nx = seq[p + 1] if d + 1 < n_steps else "N"
            cand = [c for c in cand if nx in ACGT and present(cur[2:] + c + nx)]
            if len(cand) != 1:
                cand = []
        if not cand:
            return d, {s[1]: s[2] for s in subs}, 1, 0, []
        recent = [s for s in subs if d - w < s[0] < d]
        if len(recent) >= e:
            left = [s for s in subs if s not in recent]
            return min([s[0] for s in recent] + [d]), {s[1]: s[2] for s in left}, 1, 1, sorted(s[1] for s in recent)
        subs.append((d, p, cand[0]))
        cur = cur[1:] + cand[0]
    return n_steps, {s[1]: s[2] for s in subs}, 0, 0, []


def brute_read(bases, table, k=qc.K, a=qc.A, w=qc.W, e=qc.E):
    """rules 2-6 on one read: {"text": the corrected read, "lo", "hi": its span, "anchored", "substitutions", "stopped", "reverts",
    "reverted_right": positions a window revert of the rightward walk set back, "reverted_left": of the leftward walk}"""
    b = qc.norm(bases)
    L = len(b)
    out = {"text": b, "lo": 0, "hi": 0, "anchored": 0, "substitutions": 0, "stopped": 0, "reverts": 0, "reverted_right": [], "reverted_left": []}
    i0 = None
    for i in range(L - k + 1):
        win = b[i:i + k]
        if "N" not in win and table.get(min(win, qc.revcomp(win)), 0) >= a:
            i0 = i
            break
    if i0 is None:
        return out
    ef, subs_f, stop_f, nrev_f, rev_f = walk_right(b, i0, k, table, w, e)
    m = rc_n(b)                                                   # the leftward walk: rightward on the reverse complement
    eb, subs_m, stop_b, nrev_b, rev_m = walk_right(m, L - i0 - k, k, table, w, e)
    t = list(b)
    for p, c in subs_f.items():
        t[p] = c
    for p, c in subs_m.items():
        t[L - 1 - p] = qc.COMP[c]
    out.update(text="".join(t), lo=i0 - eb, hi=i0 + k + ef, anchored=1, substitutions=len(subs_f) + len(subs_m), stopped=stop_f + stop_b,
               reverts=nrev_f + nrev_b, reverted_right=rev_f, reverted_left=sorted(L - 1 - p for p in rev_m))
    return out


def brute_run(files, k=qc.K, q=qc.Q, a=qc.A, w=qc.W, e=qc.E, trim=False, min_len=None, table=None):
    """The command on the read files of a sample (files: one list of reads, or the two mates'): {"files": the output files' records as
    lists of strings, "reads": brute_read of every read per file, "stats": the five counters + "table" and "windows", "trim": the five
    counters of rule 7 (with trim), "kept": indices of the kept reads (pairs)}.  table: rule 1's, if the caller has it."""
    table = qc.brute_table(files, k, q) if table is None else table
    reads = [[brute_read(bases, table, k, a, w, e) for bases, _ql in f] for f in files]
    stats = {name: sum(r.get(name, 0) for f in reads for r in f) for name in ("anchored", "substitutions", "stopped", "reverts")}
    stats["changed"] = sum(1 for f, rs in zip(files, reads) for (bases, _ql), r in zip(f, rs) if r["text"] != qc.norm(bases))
    stats["table"], stats["windows"] = len(table), sum(table.values())
    n = len(files[0])
    res = {"reads": reads, "stats": stats, "table": table}
    if not trim:
        res["files"] = [[r["text"] for r in f] for f in reads]
        res["kept"] = list(range(n))
        return res
    M = k if min_len is None else min_len
    own = [[r["hi"] - r["lo"] >= M for r in f] for f in reads]
    kept = [i for i in range(n) if all(o[i] for o in own)]
    tr = dict.fromkeys(TRIM_NAMES, 0)
    tr["below_min"] = sum(1 for o in own for x in o if not x)
    tr["pairs_dropped"] = n - len(kept) if len(files) == 2 else 0
    out = []
    for f in reads:
        rec = []
        for i in kept:
            r = f[i]
            rec.append(r["text"][r["lo"]:r["hi"]])
            tr["kept"] += 1
            if r["hi"] - r["lo"] < len(r["text"]):
                tr["trimmed"] += 1
                tr["bases_cut"] += len(r["text"]) - (r["hi"] - r["lo"])
        out.append(rec)
    res.update(files=out, kept=kept, trim=tr)
    return res


def fasta_of(records, mate=0, first=0):
    """the text of corrected_reads*.fa for these records: >i_1 / >i_2 (mate 0: >i)"""
    return "".join(">%d%s\n%s\n" % (first + i, "_%d" % mate if mate else "", s) for i, s in enumerate(records))


def expected_texts(res):
    """{file name: text} of a brute_run"""
    if len(res["files"]) == 2:
        return {"corrected_reads_1.fa": fasta_of(res["files"][0], 1), "corrected_reads_2.fa": fasta_of(res["files"][1], 2)}
    return {"corrected_reads.fa": fasta_of(res["files"][0])}


def write_fastq(path, reads):
    with open(path, "w") as f:
        f.write(qc.fastq_text(reads))
    return path


def write_lanes(d, stem, files, cuts):
    """the reads of `files` (one list, or the two mates') cut into lanes at the read indices `cuts`: the paths, [lanes of file 0,
    lanes of file 1], and the concatenated files' paths"""
    os.makedirs(d, exist_ok=True)
    bounds = [0] + list(cuts) + [len(files[0])]
    lanes, whole = [], []
    for m, f in enumerate(files):
        lanes.append([write_fastq(os.path.join(d, "%s_%d_lane%d.fq" % (stem, m + 1, i)), f[bounds[i]:bounds[i + 1]]) for i in range(len(bounds) - 1)])
        whole.append(write_fastq(os.path.join(d, "%s_%d_all.fq" % (stem, m + 1)), f))
    return lanes, whole


# ------------------------------------------------------------------------------------------------ inputs
TRIM_M = 40                    # the --min_len of the trim input: above k = 24, so that a span of TRIM_M - 1 holds an anchor and is dropped


def trim_case(seed=3):
    """Paired reads in which every class of span occurs (test_correct.test_every_span_class_occurs says which and checks it).
    G: a transcript of 110 bases, every window of it an anchor; H: one of 60 bases.  Nothing continues either beyond its ends, so a
    read that runs off an end with random low-quality bases has no candidate there and its walk stops at the end exactly.
    Returns (files, {name: pair index})."""
    rng = random.Random(seed)
    G, H = qc.rand_seq(rng, 110), qc.rand_seq(rng, 60)
    sup = qc.support(G) + [(H, "I" * 60)] * 3
    clean = (G[20:80], "I" * 60)

    def off_end(core, head, tail):
        return (qc.rand_seq(rng, head) + core + qc.rand_seq(rng, tail), "#" * head + "I" * len(core) + "#" * tail)

    special = [
        ("whole", qc.with_errors(rng, G[10:70], [40]), clean),
        ("whole_base_0", qc.with_errors(rng, G[10:70], [0]), clean),
        ("cut_3", off_end(G[60:110], 0, 10), clean),
        ("cut_5", off_end(G[0:50], 10, 0), clean),
        ("cut_both", off_end(H, 8, 8), clean),
        ("revert_right", qc.with_errors(rng, G[10:70], [30, 32, 34, 36]), clean),
        ("revert_left", qc.with_errors(rng, G[10:70], [20, 22, 24, 26]), clean),
        ("revert_right_kept", qc.with_errors(rng, G[10:70], [45, 47, 49, 51]), clean),
        ("no_anchor", (qc.rand_seq(rng, 60), "I" * 60), clean),
        ("short", (G[10:30], "I" * 20), clean),
        ("span_m_minus_1", off_end(G[110 - (TRIM_M - 1):110], 0, 12), clean),
        ("span_m", off_end(G[110 - TRIM_M:110], 0, 12), clean),
        ("mate_2_only", clean, (qc.rand_seq(rng, 50), "I" * 50)),
        ("n_mended", (G[10:40] + "N" + G[41:70], "I" * 60), clean),
        ("n_in_cut_tail", (G[60:110] + "ACNNGTACGT", "I" * 50 + "#" * 10), clean),
    ]
    f1 = [s[1] for s in special] + sup
    f2 = [s[2] for s in special] + [(qc.revcomp(b), ql) for b, ql in sup]
    return [f1, f2], {s[0]: i for i, s in enumerate(special)}


def lane_effect_case(seed=5):
    """Two single-end lanes.  Lane 1 holds the transcript's read twice, lane 2 once and a probe with one low-quality error at base
    40: the windows over base 40 are high-quality twice in lane 1 and once in lane 2 -- anchors (A = 3) only in the sum -- and the
    windows before it 2 + 2 times.  No lane alone holds an anchor, so the probe is corrected only against the added tables.
    Returns (lanes: two lists of reads, the probe's (lane, index), its clean text)."""
    rng = random.Random(seed)
    G = qc.rand_seq(rng, 60)
    other = qc.rand_seq(rng, 70)
    lane1 = [(G, "I" * 60), (G, "I" * 60), (other[:64], "I" * 64)]
    lane2 = [qc.with_errors(rng, G, [40]), (G, "I" * 60), (other[3:70], "I" * 67)]
    return [lane1, lane2], (1, 0), G


def noisy_tail_pairs(seed=4, every=10, tail=12):
    """the planted pairs of quorum_cases, and in every 10th pair a first mate whose last 12 bases are random and of low quality: the
    walk mends the first of them from the transcript, finds a fourth substitution inside the window, sets the three back and ends --
    such a mate is trimmed, its file becomes ragged"""
    files, _clean = qc.planted_case(seed)
    rng = random.Random(seed + 77)
    for i in range(0, len(files[0]), every):
        b, ql = files[0][i]
        files[0][i] = (b[:-tail] + qc.rand_seq(rng, tail), ql[:-tail] + "#" * tail)
    return files
