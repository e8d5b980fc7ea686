"""--quorum: the brute force of the rule, in plain Python over strings and a dict, and the inputs of the tests.

Written from the rule's text, not from the kernels: a read is a pair (bases, qualities) of two strings of one length; the table is a
dict {canonical k-mer string: count}; a corrected read is a string over ACGTN (a base outside ACGT is N, as the ingest codes it and
as the FASTA formatter writes it).  Strings compare as the 2k-bit numbers do, since A < C < G < T."""
import random

K, Q, A, W, E = 24, 5, 3, 10, 3
ACGT = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
STAT_NAMES = ("anchored", "changed", "substitutions", "stopped", "reverts")


_RC = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_RC)[::-1]


def can(x):
    return min(x, revcomp(x))


def norm(bases):
    """a read's bases as ingested: upper case, anything outside ACGT is N"""
    return "".join(c if c in ACGT else "N" for c in bases.upper())


def hq_bits(bases, quals, q=Q):
    """rule 1: base p is hq when it is one of ACGT and ord(quality[p]) - 33 >= q"""
    return [c in ACGT and ord(ql) - 33 >= q for c, ql in zip(norm(bases), quals)]


def brute_table(files, k=K, q=Q):
    """rule 1: {can(w): number of HQ windows w} over all reads of all files (files: lists of (bases, qualities))"""
    table = {}
    for reads in files:
        for bases, quals in reads:
            b, hq = norm(bases), hq_bits(bases, quals, q)
            for i in range(len(b) - k + 1):
                if all(hq[i:i + k]):
                    key = can(b[i:i + k])
                    table[key] = table.get(key, 0) + 1
    return table


def brute_correct(bases, table, k=K, a=A, w=W, e=E):
    """rules 2-5 on one read: (corrected bases, {"anchored", "substitutions", "stopped", "reverts"})"""
    b = norm(bases)
    L = len(b)
    st = {"anchored": 0, "substitutions": 0, "stopped": 0, "reverts": 0}
    if L < k:
        return b, st

    def present(x):
        return table.get(can(x), 0) >= 1

    i0 = None
    for i in range(L - k + 1):
        win = b[i:i + k]
        if all(c in ACGT for c in win) and table.get(can(win), 0) >= a:
            i0 = i
            break
    if i0 is None:
        return b, st
    st["anchored"] = 1
    t = list(b)

    def walk(forward):
        cur = b[i0:i0 + k]
        subs = []                                                   # positions substituted in this direction, still in place
        positions = range(i0 + k, L) if forward else range(i0 - 1, -1, -1)
        for p in positions:
            ext = (lambda x, c: x[1:] + c) if forward else (lambda x, c: c + x[:-1])
            r = t[p]
            if r in ACGT and present(ext(cur, r)):
                cur = ext(cur, r)
                continue
            S = [c for c in ACGT if c != r and present(ext(cur, c))]
            if len(S) >= 2:
                nxt = p + 1 if forward else p - 1
                if 0 <= nxt < L and t[nxt] in ACGT:
                    S = [c for c in S if present(ext(ext(cur, c), t[nxt]))]
                    if len(S) != 1:
                        st["stopped"] += 1
                        return
                else:
                    st["stopped"] += 1
                    return
            if len(S) == 0:
                st["stopped"] += 1
                return
            c = S[0]
            inside = [x for x in subs if (p - w < x < p if forward else p < x < p + w)]
            if len(inside) >= e:
                for x in inside:
                    t[x] = b[x]
                    subs.remove(x)
                st["reverts"] += 1
                st["stopped"] += 1
                st["substitutions"] -= len(inside)
                return
            t[p] = c
            subs.append(p)
            st["substitutions"] += 1
            cur = ext(cur, c)

    walk(True)
    walk(False)
    return "".join(t), st


def brute_apply(files, k=K, q=Q, a=A, w=W, e=E):
    """the whole step: (corrected files: lists of strings, stats summed over all reads + "table" and "windows", the table)"""
    table = brute_table(files, k, q)
    stats = dict.fromkeys(STAT_NAMES, 0)
    out = []
    for reads in files:
        fixed = []
        for bases, _quals in reads:
            t, st = brute_correct(bases, table, k, a, w, e)
            fixed.append(t)
            for name in ("anchored", "substitutions", "stopped", "reverts"):
                stats[name] += st[name]
            stats["changed"] += 1 if t != norm(bases) else 0
        out.append(fixed)
    stats["table"], stats["windows"] = len(table), sum(table.values())
    return out, stats, table


# ------------------------------------------------------------------------------------------------ inputs
def rand_seq(rng, n):
    return "".join(rng.choice(ACGT) for _ in range(n))


def other(rng, c):
    return rng.choice([x for x in ACGT if x != c])


def fastq_text(reads):
    return "".join("@%d\n%s\n+\n%s\n" % (i, b, ql) for i, (b, ql) in enumerate(reads))


def fasta_text(seqs):
    return "".join(">%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def support(genome, length=60, stride=10, copies=3):
    """clean reads of quality I that cover `genome` `copies` times and more: every k-window of it becomes an anchor"""
    starts = list(range(0, len(genome) - length + 1, stride))
    if starts[-1] != len(genome) - length:
        starts.append(len(genome) - length)
    return [(genome[s:s + length], "I" * length) for s in starts for _ in range(copies)]


def with_errors(rng, clean, positions, qual="#"):
    """(bases, qualities): `clean` with another base of quality `qual` at every position, quality I elsewhere"""
    b, ql = list(clean), ["I"] * len(clean)
    for p in positions:
        b[p] = other(rng, clean[p])
        ql[p] = qual
    return "".join(b), "".join(ql)


def scenario(name, seed=1):
    """One small input per situation of the rule: {"files": [reads], "probe": (file, index) of the read the case is about,
    "clean": what that read was before its errors}.  The probe read comes first in its file, the support behind it."""
    rng = random.Random("%s/%d" % (name, seed))
    G = rand_seq(rng, 110)
    sup = support(G)
    clean = G[10:70]

    def one(read, clean_text=clean, extra=()):
        return {"files": [[read] + sup + list(extra)], "probe": (0, 0), "clean": clean_text}

    if name == "mid":
        return one(with_errors(rng, clean, [40]))
    if name == "first_window":
        return one(with_errors(rng, clean, [5]))
    if name == "last_base":
        return one(with_errors(rng, clean, [59]))
    if name == "base_0":
        return one(with_errors(rng, clean, [0]))
    if name in ("lookahead_settles", "lookahead_fails"):
        # two transcripts share 40 bases and part at one base: after the shared stretch `A...` follows in one, `C...` in the other.
        # The probe follows the first with an error AT the fork: both letters are candidates, the base behind the fork decides --
        # unless the two agree there too
        P, X1 = rand_seq(rng, 40), rand_seq(rng, 30)
        nxt = X1[0] if name == "lookahead_fails" else other(rng, X1[0])
        X2 = nxt + rand_seq(rng, 29)
        T1, T2 = P + "A" + X1, P + "C" + X2
        probe_clean = T1[5:65]
        b, ql = list(probe_clean), ["I"] * 60
        b[35], ql[35] = "G", "#"                                     # (the fork is base 40 of T1: base 35 of the probe)
        return {"files": [[("".join(b), "".join(ql))] + support(T1, 60, 11) + support(T2, 60, 11)], "probe": (0, 0), "clean": probe_clean}
    if name == "no_candidate":
        # the probe runs off the end of everything the table knows: its last ten bases (low quality) continue nothing
        tail = rand_seq(rng, 10)
        read = (G[60:110] + tail, "I" * 50 + "#" * 10)
        return one(read, G[60:110] + tail)
    if name == "n_base":
        b = list(clean)
        b[40] = "N"
        return one(("".join(b), "I" * 60))
    if name == "fourth_forward":
        return one(with_errors(rng, clean, [30, 32, 34, 36]))
    if name == "fourth_backward":
        return one(with_errors(rng, clean, [20, 22, 24, 26]))
    if name == "no_anchor":
        lone = rand_seq(rng, 60)
        return one((lone, "I" * 60), lone)
    if name == "short":
        return one((G[10:30], "I" * 20), G[10:30])
    if name == "mates_two_lengths":
        # mate files of 60 and 50 bases, ONE table over both: the second file's errors are mended by windows only the first holds
        f1 = [with_errors(rng, G[10:70], [40])] + sup
        f2 = [with_errors(rng, revcomp(G[40:90]), [12])] + [(revcomp(b)[:50], "I" * 50) for b, _q in sup]
        return {"files": [f1, f2], "probe": (1, 0), "clean": revcomp(G[40:90])}
    raise KeyError(name)


SCENARIOS = ("mid", "first_window", "last_base", "base_0", "lookahead_settles", "lookahead_fails", "no_candidate", "n_base", "fourth_forward",
             "fourth_backward", "no_anchor", "short", "mates_two_lengths")


def ragged_case(n=5000, seed=7):
    """about n reads of 20 .. 130 bases from a few transcripts, every fifth with low-quality errors, some with N: blocks of the
    kernels and the 32 / 64-base word boundaries are crossed by reads, windows and substitutions alike"""
    rng = random.Random(seed)
    T = [rand_seq(rng, 400) for _ in range(6)]
    reads = []
    for i in range(n):
        t = T[rng.randrange(len(T))]
        L = rng.choice((20, 23, 24, 25, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 130))
        s = rng.randrange(0, len(t) - L + 1)
        clean = t[s:s + L] if rng.random() < 0.5 else revcomp(t[s:s + L])
        if i % 5 == 0:
            b, ql = with_errors(rng, clean, sorted(rng.sample(range(L), rng.choice((1, 1, 2, 4)))))
        else:
            b, ql = clean, "I" * L
        if i % 97 == 0:
            p = rng.randrange(L)
            b = b[:p] + "N" + b[p + 1:]
        reads.append((b, ql))
    return [reads]


def planted_case(seed=4, n_tr=8, tr_len=300, read_len=50, coverage=20):
    """random transcripts of 300 bases, about 20x coverage with 50-base pairs of quality I (mate 2 from the other strand, 150 bases
    downstream of mate 1's start at the most), and one substituted base of quality # in every fifth read of either file:
    (files, clean files)"""
    rng = random.Random(seed)
    T = [rand_seq(rng, tr_len) for _ in range(n_tr)]
    n_pairs = n_tr * tr_len * coverage // (2 * read_len)
    files, clean = [[], []], [[], []]
    for i in range(n_pairs):
        t = T[i % n_tr]
        frag = rng.randrange(120, 201)
        s = rng.randrange(0, tr_len - frag + 1)
        pair = (t[s:s + read_len], revcomp(t[s + frag - read_len:s + frag]))
        for m in (0, 1):
            c = pair[m]
            clean[m].append(c)
            files[m].append(with_errors(rng, c, [rng.randrange(read_len)]) if (2 * i + m) % 5 == 0 else (c, "I" * read_len))
    return files, clean


def kallisto_case(seed=4):
    """the planted-error pairs, and in every 40th pair a first mate with TWO # errors 25 bases apart (both mates of those pairs are
    clean in planted_case): as it stands such a mate cannot be placed on its transcript by the rule of DESIGN.md 3.8 / 3.10 (a
    50-base mate may carry 50 // 30 = 1 mismatch), corrected it can -- the original and the corrected pairs quantify differently.
    (files, clean files, indices of those pairs)"""
    files, clean = planted_case(seed)
    rng = random.Random(seed + 1000)
    double = [i for i in range(len(files[0])) if i % 40 == 1]
    for i in double:
        assert files[0][i][0] == clean[0][i] and files[1][i][0] == clean[1][i]
        files[0][i] = with_errors(rng, clean[0][i], [12, 37])
    return files, clean, double
