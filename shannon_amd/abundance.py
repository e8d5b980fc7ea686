"""--kallisto_cutoff: drop the final transcripts that the reads barely express (shannon.py:309-318, 609-614, filter_kallisto.py).

The reference moves reconstructed.fasta to rec_before_kallisto.fasta, runs `kallisto index` + `kallisto quant` on it and the
original read files, and filter_using_kallisto (filter_kallisto.py:8-21) keeps a transcript when est_counts / eff_length * L of
its abundance.tsv line reaches the cutoff.  Here kallisto is a stated rule run on the device
(csrc/abundance.hip: shn_abundance_classes, shn_abundance_em); the table's text and the decision are the reference's, made on the host:

    classes        the pairs' compatibility classes, span histogram and mapped count (the first device call)
    eff_lengths    rule 2: effective lengths from the integer histogram, in double
    em             rule 4 on host arrays of classes (the second device call)
    quantify       names + sequences + resident mates -> table (classes, eff_lengths, em, tpm)
    abundance_tsv  table -> the text of abundance.tsv, floats written with repr
    decide         filter_kallisto.py:8-21 on the TEXT of abundance.tsv and of the FASTA -> the text of the filtered FASTA
    apply          final transcripts {name: sequence} -> (filtered {name: sequence}, table, tsv text, FASTA text before)

Single reads (the command is shannon_amd/quant.py):

    classes_single     a read's compatibility set over its orientations, classes, mapped count (shn_abundance_classes_single)
    eff_lengths_model  effective lengths from the fixed fragment-length model (mean, sd), in double
    quantify_single    names + sequences + one resident read set -> table

Bootstrap replicates (quant.py's -b B --seed S; quantify / quantify_single with bootstraps=B):

    resample           B resampled count vectors of the classes (shn_abundance_resample)
    em_batch           the EM on a matrix of count vectors at once, every row bit for bit `em`'s (shn_abundance_em_batch)
    bootstrap          both, the counts staying on the device (shn_abundance_bootstrap)
    bootstrap_summary  mean, sd, min, max per transcript over the replicates' est_counts
    bootstrap_summary_tsv, replicate_table  the texts of bootstrap_summary.tsv and, through abundance_tsv, of bs_abundance_<b>.tsv

Reads in several parts -- the lane files of a sample, the slices of N ranks (quant.py's comma lists and --gpus N):

    list_key           the 63-bit key of a member list, in plain integers
    merge_classes      the class dicts of the parts -> the classes of all their reads (shn_abundance_merge)
    quantify_classes   class dicts of parts -> table: merge_classes, then the tail of quantify / quantify_single
    quantify_parts     resident read sets, one part at a time -> table

`eff_lengths`, `eff_lengths_model`, `abundance_tsv`, `decide`, `bootstrap_summary`, `bootstrap_summary_tsv`, `replicate_table` and
`list_key` need neither the library nor a GPU.
"""
import ctypes as C
import io
import math
import numpy as np

MAX_SPAN = 500        # as --filter_FP: the longest fragment a concordant pair may span
SEED = 15             # a transcript shorter than this takes part in no class
MODEL_MEAN, MODEL_SD, MODEL_BINS = 200.0, 20.0, 1000        # single reads: kallisto quant --single -l 200 -s 20 (filter_kallisto.py:25), fragments of 0..999 bases
HEADER = "target_id\tlength\teff_length\test_counts\ttpm\n"


def _transcript_text(seqs):
    """(text uint8, t_off uint64[n + 1]) of the transcripts one after the other; one shorter than SEED bases or with a base outside
    ACGT is handed over empty: it takes part in no class"""
    seqs = [s if len(s) >= SEED and not s.encode().translate(None, b"ACGTacgt") else "" for s in seqs]
    t_off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        t_off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    joined = "".join(seqs).encode()
    return (np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)), t_off


def classes(ctx, seqs, d1, d2, strand_specific, max_span=MAX_SPAN):
    """rules 1-3 (shn_abundance_classes): {"class_off", "members", "n_c", "hist", "mapped", "fragments"}.  A transcript shorter
    than SEED bases or with a base outside ACGT is handed over empty: it takes part in no class."""
    from . import _lib
    text, t_off = _transcript_text(seqs)
    h = C.c_void_p()
    lib = _lib.lib()
    _lib.check(lib.shn_abundance_classes(ctx.h, text.ctypes.data, t_off.ctypes.data, len(seqs), d1.h, d2.h, 1 if strand_specific else 0, int(max_span),
                                         C.byref(h)))
    return _export(lib, h)


def classes_single(ctx, seqs, d, strand_specific):
    """rules 1 of DESIGN.md 3.13 and 3 of 3.10 for the single reads of the resident set d (shn_abundance_classes_single): {"class_off",
    "members", "n_c", "mapped", "fragments"} (fragments: the reads) and "hist", empty -- single reads have no span.  Transcripts as in
    `classes`."""
    from . import _lib
    text, t_off = _transcript_text(seqs)
    h = C.c_void_p()
    lib = _lib.lib()
    _lib.check(lib.shn_abundance_classes_single(ctx.h, text.ctypes.data, t_off.ctypes.data, len(seqs), d.h, 1 if strand_specific else 0, C.byref(h)))
    return _export(lib, h)


def _export(lib, h):
    """what a handle of shn_abundance_classes / _single holds, as arrays; destroys the handle"""
    from . import _lib
    try:
        sizes = np.zeros(6, dtype=np.uint64)
        _lib.check(lib.shn_abundance_sizes(h, sizes.ctypes.data))
        _n_tr, n_frag, mapped, n_classes, n_entries, n_bins = (int(x) for x in sizes)
        class_off = np.zeros(n_classes + 1, dtype=np.uint64)
        members = np.zeros(max(n_entries, 1), dtype=np.uint32)
        n_c = np.zeros(max(n_classes, 1), dtype=np.uint64)
        hist = np.zeros(n_bins, dtype=np.uint64)
        _lib.check(lib.shn_abundance_export(h, class_off.ctypes.data, members.ctypes.data, n_c.ctypes.data, hist.ctypes.data if n_bins else None))
    finally:
        lib.shn_abundance_destroy(h)
    return {"class_off": class_off, "members": members[:n_entries], "n_c": n_c[:n_classes], "hist": hist, "mapped": mapped, "fragments": n_frag}


_M64 = (1 << 64) - 1


def _mix(h, v):
    """abd_mix of csrc/abundance.hip in plain integers"""
    h ^= (v + 0x9E3779B97F4A7C15) & _M64
    h ^= h >> 33
    h = h * 0xFF51AFD7ED558CCD & _M64
    h ^= h >> 33
    h = h * 0xC4CEB9FE1A85EC53 & _M64
    h ^= h >> 33
    return h


def list_key(members):
    """the 63-bit key of an ascending member list: what abd_finish_list gives a fragment with this list -- the mix of 0
    and the length, then of every member in order, shifted right by one.  Plain integers: needs neither the library nor a GPU."""
    members = [int(j) for j in members]
    h = _mix(0, len(members))
    for j in members:
        h = _mix(h, j)
    return h >> 1


def merge_classes(ctx, parts, m, hash_bits=63):
    """DESIGN.md 3.15 (shn_abundance_merge): the class dicts of P >= 1 read sets on the same m transcripts -> one dict of the same shape,
    the classes of the union of the reads: the parts' classes as weighted lists, in part order, merged on the device; "hist", "mapped"
    and "fragments" are the parts' sums.  Parts whose "hist" differ in length (another max_span, pairs beside single reads) are
    refused.  One part goes through the device too."""
    from . import _lib
    parts = list(parts)
    if not parts:
        raise ValueError("abundance.merge_classes: no parts")
    bins = set(len(p["hist"]) for p in parts)
    if len(bins) != 1:
        raise ValueError("abundance.merge_classes: the parts' histograms have %s bins: not built with one max_span" % sorted(bins))
    sizes = [len(p["n_c"]) for p in parts]
    for p, n in zip(parts, sizes):
        if len(p["class_off"]) != n + 1 or int(p["class_off"][0]) != 0 or int(p["class_off"][-1]) != len(p["members"]):
            raise ValueError("abundance.merge_classes: a part's class_off does not fit its n_c and members")
    n_lists = sum(sizes)
    class_off = np.zeros(n_lists + 1, dtype=np.uint64)                 # one CSR: every part's offsets rebased behind the parts before it
    at = base = 0
    for p, n in zip(parts, sizes):
        class_off[at + 1:at + n + 1] = np.asarray(p["class_off"][1:], dtype=np.uint64) + np.uint64(base)
        at, base = at + n, base + len(p["members"])
    members = np.ascontiguousarray(np.concatenate([np.asarray(p["members"], dtype=np.uint32) for p in parts]))
    n_c = np.ascontiguousarray(np.concatenate([np.asarray(p["n_c"], dtype=np.uint64) for p in parts]))
    h = C.c_void_p()
    lib = _lib.lib()
    _lib.check(lib.shn_abundance_merge(ctx.h, class_off.ctypes.data, members.ctypes.data if len(members) else None, n_c.ctypes.data if n_lists else None,
                                       n_lists, int(m), int(hash_bits), C.byref(h)))
    out = _export(lib, h)
    hist = np.zeros(bins.pop(), dtype=np.uint64)
    for p in parts:
        hist += np.asarray(p["hist"], dtype=np.uint64)
    out["hist"], out["mapped"], out["fragments"] = hist, sum(int(p["mapped"]) for p in parts), sum(int(p["fragments"]) for p in parts)
    return out


def _eff_from_prefix(lens, cnt, tot):
    """the tail of both rules 2 over prefix sums (cnt[k], tot[k]: the sums over s < k of the weights and of s times the weights, for
    len(cnt) - 1 bins): eff_j = len_j - tot[k] / cnt[k] + 1 with k = min(len_j, bins - 1) + 1 -- one division, then rounded to double
    -- or len_j when that is < 1 or cnt[k] is 0"""
    out = []
    for n in lens:
        n = int(n)
        k = min(n, len(cnt) - 2) + 1
        eff = float(n)
        if k > 0 and cnt[k] > 0:
            e = float(n) - tot[k] / cnt[k] + 1.0
            if e >= 1.0:
                eff = e
        out.append(eff)
    return np.array(out, dtype=np.float64)


def eff_lengths(lens, hist):
    """rule 2: eff_j = len_j - mu_{len_j} + 1, mu_l = (sum of s h[s] over s <= l) / (sum of h[s] over s <= l), the two sums as
    integers and their quotient rounded once to double; eff_j = len_j when that is < 1 or when no span is <= len_j."""
    h = [int(x) for x in hist]
    cnt, tot = [0] * (len(h) + 1), [0] * (len(h) + 1)            # prefix sums: spans < s
    for s, x in enumerate(h):
        cnt[s + 1] = cnt[s] + x
        tot[s + 1] = tot[s] + s * x
    return _eff_from_prefix(lens, cnt, tot)


def em(ctx, class_off, members, n_c, eff):
    """rule 4 (shn_abundance_em) on host arrays -> (alpha float64[m], rounds)"""
    from . import _lib
    n_c = np.ascontiguousarray(n_c, dtype=np.uint64)
    class_off, members, eff, n_classes = _em_arrays("em", class_off, members, eff, len(n_c))
    m = len(eff)
    alpha = np.zeros(max(m, 1), dtype=np.float64)
    rounds = C.c_uint32(0)
    _lib.check(_lib.lib().shn_abundance_em(ctx.h, class_off.ctypes.data, members.ctypes.data if len(members) else None,
                                           n_c.ctypes.data if n_classes else None, n_classes, eff.ctypes.data if m else None, m, alpha.ctypes.data,
                                           C.byref(rounds)))
    return alpha[:m], int(rounds.value)


def _em_arrays(who, class_off, members, eff, n_count_cols):
    """the classes and eff as the library takes them, with em's own checks"""
    class_off = np.ascontiguousarray(class_off, dtype=np.uint64)
    members = np.ascontiguousarray(members, dtype=np.uint32)
    eff = np.ascontiguousarray(eff, dtype=np.float64)
    n_classes = len(class_off) - 1
    if n_classes < 0 or n_count_cols != n_classes:
        raise ValueError("abundance.%s: class_off has %d entries for %d class counts" % (who, len(class_off), n_count_cols))
    if n_classes and int(class_off[-1]) > len(members):
        raise ValueError("abundance.%s: class_off ends at %d, %d members given" % (who, int(class_off[-1]), len(members)))
    return class_off, members, eff, n_classes


def _replicates(who, B):
    B = int(B)
    if not 1 <= B < 1 << 32:
        raise ValueError("abundance.%s: %d replicates (1 .. 2^32 - 1)" % (who, B))
    return B


def _seed(who, seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("abundance.%s: seed %d outside 0 .. 2^64 - 1" % (who, seed))
    return seed


def resample(ctx, n_c, B, seed):
    """rule 1 of DESIGN.md 3.14 (shn_abundance_resample): uint64[B][classes], row b the class counts of bootstrap replicate b"""
    from . import _lib
    n_c = np.ascontiguousarray(n_c, dtype=np.uint64)
    B, seed = _replicates("resample", B), _seed("resample", seed)
    out = np.zeros((B, len(n_c)), dtype=np.uint64)
    _lib.check(_lib.lib().shn_abundance_resample(ctx.h, n_c.ctypes.data if len(n_c) else None, len(n_c), B, seed, out.ctypes.data if len(n_c) else None))
    return out


def em_batch(ctx, class_off, members, n_c_matrix, eff, max_live=0):
    """rule 4 for every row of n_c_matrix[B][classes] at once (shn_abundance_em_batch) -> (alpha float64[B][m], rounds uint32[B]), row b
    bit for bit em's answer on n_c_matrix[b]; max_live caps the replicates resident at once (0: the library's budget)"""
    from . import _lib
    n_c_matrix = np.ascontiguousarray(n_c_matrix, dtype=np.uint64)
    if n_c_matrix.ndim != 2:
        raise ValueError("abundance.em_batch: the counts are no matrix [replicates][classes]")
    class_off, members, eff, n_classes = _em_arrays("em_batch", class_off, members, eff, n_c_matrix.shape[1])
    B, m = _replicates("em_batch", n_c_matrix.shape[0]), len(eff)
    alpha = np.zeros((B, max(m, 1)), dtype=np.float64)
    rounds = np.zeros(B, dtype=np.uint32)
    _lib.check(_lib.lib().shn_abundance_em_batch(ctx.h, class_off.ctypes.data, members.ctypes.data if len(members) else None,
                                                 n_c_matrix.ctypes.data if n_classes else None, n_classes, eff.ctypes.data if m else None, m, B,
                                                 int(max_live), alpha.ctypes.data, rounds.ctypes.data))
    return alpha[:, :m], rounds


def bootstrap(ctx, class_off, members, n_c, eff, B, seed, max_live=0, want_counts=False):
    """resample, then em_batch, the counts staying on the device (shn_abundance_bootstrap) -> (alpha float64[B][m], rounds uint32[B],
    counts uint64[B][classes] or None)"""
    from . import _lib
    n_c = np.ascontiguousarray(n_c, dtype=np.uint64)
    class_off, members, eff, n_classes = _em_arrays("bootstrap", class_off, members, eff, len(n_c))
    B, seed, m = _replicates("bootstrap", B), _seed("bootstrap", seed), len(eff)
    alpha = np.zeros((B, max(m, 1)), dtype=np.float64)
    rounds = np.zeros(B, dtype=np.uint32)
    counts = np.zeros((B, n_classes), dtype=np.uint64) if want_counts else None
    _lib.check(_lib.lib().shn_abundance_bootstrap(ctx.h, class_off.ctypes.data, members.ctypes.data if len(members) else None,
                                                  n_c.ctypes.data if n_classes else None, n_classes, eff.ctypes.data if m else None, m, B, seed,
                                                  int(max_live), alpha.ctypes.data, rounds.ctypes.data,
                                                  counts.ctypes.data if want_counts and n_classes else None))
    return alpha[:, :m], rounds, counts


def bootstrap_summary(est_counts_matrix):
    """rule 3 of DESIGN.md 3.14 on est_counts[B][m], per transcript over x_b = est_counts[b][j]: {"bs_mean": (x_0 + x_1 + ... in that
    order) / B, "bs_sd": sqrt(sum of (x_b - bs_mean)^2, in order, / (B - 1)), 0.0 for B = 1, "bs_min", "bs_max"} (lists); host only"""
    rows = [[float(x) for x in row] for row in est_counts_matrix]
    B = len(rows)
    if B < 1:
        raise ValueError("abundance.bootstrap_summary: no replicates")
    out = {"bs_mean": [], "bs_sd": [], "bs_min": [], "bs_max": []}
    for j in range(len(rows[0])):
        xs = [row[j] for row in rows]
        total = 0.0
        for x in xs:
            total += x
        mean = total / B
        ss = 0.0
        for x in xs:
            ss += (x - mean) * (x - mean)
        out["bs_mean"].append(mean)
        out["bs_sd"].append(math.sqrt(ss / (B - 1)) if B > 1 else 0.0)
        out["bs_min"].append(min(xs))
        out["bs_max"].append(max(xs))
    return out


def _no_targets(bootstraps, seed):
    """the bootstrap columns of a table without transcripts"""
    if bootstraps is None:
        return {}
    return {"bs_est_counts": [[] for _ in range(bootstraps)], "bs_tpm": [[] for _ in range(bootstraps)], "bs_rounds": [0] * bootstraps, "bs_mean": [],
            "bs_sd": [], "bs_min": [], "bs_max": [], "bootstraps": bootstraps, "seed": seed}


def _add_bootstraps(ctx, table, cl, eff, bootstraps, seed):
    """the bootstrap columns of quantify / quantify_single: "bs_est_counts" and "bs_tpm" (B lists), "bs_rounds", the summary"""
    alpha, rounds, _ = bootstrap(ctx, cl["class_off"], cl["members"], cl["n_c"], eff, bootstraps, seed)
    table["bs_est_counts"] = [a.tolist() for a in alpha]
    table["bs_tpm"] = [tpm_of(a, eff) for a in alpha]
    table["bs_rounds"] = [int(r) for r in rounds]
    table.update(bootstrap_summary(table["bs_est_counts"]))
    table["bootstraps"], table["seed"] = len(table["bs_rounds"]), int(seed)
    return table


def bootstrap_summary_tsv(table):
    """the text of bootstrap_summary.tsv: target_id est_counts bs_mean bs_sd bs_min bs_max, the floats written with repr"""
    out = ["target_id\test_counts\tbs_mean\tbs_sd\tbs_min\tbs_max\n"]
    for row in zip(table["names"], table["est_counts"], table["bs_mean"], table["bs_sd"], table["bs_min"], table["bs_max"]):
        out.append("%s\t%s\n" % (row[0], "\t".join(repr(float(x)) for x in row[1:])))
    return "".join(out)


def replicate_table(table, b):
    """replicate b of a table with bootstraps as a table of its own (for abundance_tsv: bs_abundance_<b>.tsv)"""
    return {"names": table["names"], "length": table["length"], "eff_length": table["eff_length"], "est_counts": table["bs_est_counts"][b],
            "tpm": table["bs_tpm"][b]}


def tpm_of(alpha, eff):
    """tpm_j = 1e6 (alpha_j / eff_j) / sum_k (alpha_k / eff_k), the sum in index order; all zeros when nothing is mapped"""
    rho = [float(a) / float(e) for a, e in zip(alpha, eff)]
    total = 0.0
    for r in rho:
        total += r
    return [1e6 * r / total if total > 0.0 else 0.0 for r in rho]


def _quantify(who, ctx, names, seqs, fragments, no_hist, classes_and_eff, bootstraps, seed):
    """what quantify and quantify_single share: the checks, the table without transcripts (`fragments` given, "hist": no_hist), then
    classes_and_eff(lens) -> (classes, eff) in the caller's order, em, the table, the bootstrap columns"""
    if len(names) != len(seqs):
        raise ValueError("%s: %d names for %d sequences" % (who, len(names), len(seqs)))
    if bootstraps is not None:
        bootstraps, seed = _replicates(who, bootstraps), _seed(who, seed)
    lens = [len(s) for s in seqs]
    if not seqs:
        return {"names": [], "length": [], "eff_length": [], "est_counts": [], "tpm": [], "mapped": 0, "fragments": fragments, "classes": 0,
                "rounds": 0, "hist": no_hist, **_no_targets(bootstraps, seed)}
    cl, eff = classes_and_eff(lens)
    alpha, rounds = em(ctx, cl["class_off"], cl["members"], cl["n_c"], eff)
    table = {"names": list(names), "length": lens, "eff_length": eff.tolist(), "est_counts": alpha.tolist(), "tpm": tpm_of(alpha, eff),
             "mapped": cl["mapped"], "fragments": cl["fragments"], "classes": len(cl["n_c"]), "rounds": rounds, "hist": cl["hist"]}
    return table if bootstraps is None else _add_bootstraps(ctx, table, cl, eff, bootstraps, seed)


def quantify(ctx, names, seqs, d1, d2, strand_specific, max_span=MAX_SPAN, bootstraps=None, seed=0):
    """the abundance table of the transcripts (names[j], seqs[j]) under the pairs of the resident sets d1 / d2 (device.Reads, the mates
    as the user gave them): {"names", "length", "eff_length", "est_counts", "tpm"} (lists, in the order given) + "mapped",
    "fragments", "classes", "rounds", "hist".  bootstraps=B adds B replicates under `seed`: "bs_est_counts" and "bs_tpm" (B
    lists), "bs_rounds", "bs_mean", "bs_sd", "bs_min", "bs_max"; None: nothing of that runs."""
    def classes_and_eff(lens):                                  # the classes first: eff needs their span histogram
        cl = classes(ctx, seqs, d1, d2, strand_specific, max_span)
        return cl, eff_lengths(lens, cl["hist"])
    return _quantify("quantify", ctx, names, seqs, len(d1), np.zeros(max_span + 1, np.uint64), classes_and_eff, bootstraps, seed)


def eff_lengths_model(lens, mean=MODEL_MEAN, sd=MODEL_SD):
    """rule 2 of DESIGN.md 3.13 (single reads: no span is seen, the fragment-length model is fixed): g[s] = exp(-0.5 * (z * z)), z =
    (s - mean) / sd, for s = 0..999; mu_l = (sum of s * g[s]) / (sum of g[s]) over s <= min(l, 999), both sums from 0.0 in ascending
    s in double; eff_j = len_j - mu_{len_j} + 1, or len_j when that is < 1 (or the sum of g is 0)."""
    mean, sd = float(mean), float(sd)
    if not sd > 0.0:
        raise ValueError("eff_lengths_model: sd %r is not above 0" % sd)
    cnt, tot = [0.0] * (MODEL_BINS + 1), [0.0] * (MODEL_BINS + 1)        # prefix sums: s < k
    for s in range(MODEL_BINS):
        z = (float(s) - mean) / sd
        g = math.exp(-0.5 * (z * z))
        cnt[s + 1] = cnt[s] + g
        tot[s + 1] = tot[s] + float(s) * g
    return _eff_from_prefix(lens, cnt, tot)


def quantify_single(ctx, names, seqs, d, strand_specific, mean=MODEL_MEAN, sd=MODEL_SD, bootstraps=None, seed=0):
    """`quantify` for the single reads of the resident set d: classes_single, eff_lengths_model, em, tpm -- the same
    table, "fragments" the reads, "hist" empty; bootstraps / seed as there"""
    def classes_and_eff(lens):                                  # eff first, as before: a bad sd is refused before anything runs
        eff = eff_lengths_model(lens, mean, sd)
        return classes_single(ctx, seqs, d, strand_specific), eff
    return _quantify("quantify_single", ctx, names, seqs, len(d), np.zeros(0, np.uint64), classes_and_eff, bootstraps, seed)


def quantify_classes(ctx, names, seqs, class_parts, paired, mean=MODEL_MEAN, sd=MODEL_SD, bootstraps=None, seed=0, hash_bits=63):
    """the table of `quantify` (paired) / `quantify_single` from the class dicts of P >= 1 parts of the reads (`classes` / `classes_single`
    of each part on these transcripts, from this process or from other ranks): merge_classes, then the same tail -- eff_lengths on the
    summed histogram or eff_lengths_model, em, tpm, the bootstrap columns.  While no two different lists share a key the merged classes
    are those of the reads in one set, and so is every number of the table.  Adds "parts" and "lists" (the lists that
    went into the merge)."""
    class_parts = list(class_parts)
    if not class_parts:
        raise ValueError("quantify_classes: no parts")

    def classes_and_eff(lens):
        eff = None if paired else eff_lengths_model(lens, mean, sd)
        cl = merge_classes(ctx, class_parts, len(seqs), hash_bits)
        return cl, (eff_lengths(lens, cl["hist"]) if paired else eff)
    table = _quantify("quantify_classes", ctx, names, seqs, sum(int(p["fragments"]) for p in class_parts),
                      np.zeros(len(class_parts[0]["hist"]), np.uint64), classes_and_eff, bootstraps, seed)
    table["parts"], table["lists"] = len(class_parts), sum(len(p["n_c"]) for p in class_parts)
    return table


def quantify_parts(ctx, names, seqs, parts_of_reads, strand_specific, max_span=MAX_SPAN, mean=MODEL_MEAN, sd=MODEL_SD, bootstraps=None, seed=0):
    """`quantify` / `quantify_single` for reads that come in P >= 1 parts (the lane files of one sample): parts_of_reads yields (d1, d2)
    -- mates -- or (d,) -- single reads -- resident sets, one kind throughout; every part's classes are built before the next part is
    asked for, so a generator may load a part, hand it over and close it: one part is resident at a time.  Then quantify_classes."""
    class_parts, paired = [], None
    for sets in parts_of_reads:
        sets = tuple(sets)
        if len(sets) not in (1, 2) or (paired is not None and paired != (len(sets) == 2)):
            raise ValueError("quantify_parts: a part is one read set or two mates, the same for every part")
        if paired is None:
            paired = len(sets) == 2
            if not paired:
                eff_lengths_model([], mean, sd)                     # (a bad sd is refused before anything runs)
        class_parts.append(classes(ctx, seqs, sets[0], sets[1], strand_specific, max_span) if paired else classes_single(ctx, seqs, sets[0], strand_specific))
    return quantify_classes(ctx, names, seqs, class_parts, paired, mean, sd, bootstraps, seed)


def abundance_tsv(table):
    """the text of abundance.tsv: kallisto's header, then target_id, length, eff_length, est_counts, tpm per transcript, the floats
    written with repr -- what filter_using_kallisto parses back is what was computed"""
    out = [HEADER]
    for name, n, el, ec, tpm in zip(table["names"], table["length"], table["eff_length"], table["est_counts"], table["tpm"]):
        out.append("%s\t%d\t%s\t%s\t%s\n" % (name, n, repr(float(el)), repr(float(ec)), repr(float(tpm))))
    return "".join(out)


def decide(tsv_text, fasta_text, cutoff, L):
    """filter_kallisto.py:8-21 on texts: a transcript is accepted iff float(est_counts) / float(eff_length) * L >= cutoff; a line of
    the FASTA is written iff the last header line before it (itself included) names an accepted transcript -- `write_now` starts True
    and carries over to the lines that follow."""
    accepted = set()
    lines = list(io.StringIO(tsv_text, newline=None))           # (the lines a file opened in text mode gives)
    for line in lines[1:]:                                      # (:11 f.readline() skips the header)
        name, _, el, ec, _weight = line.split()
        cov = float(ec) / float(el) * L
        if cov >= cutoff:
            accepted.add(name)
    write_now, out = True, []
    for line in io.StringIO(fasta_text, newline=None):
        fields = line.strip().split()
        if fields and fields[0][0] == ">":
            write_now = fields[0][1:] in accepted
        if write_now:
            out.append(line)
    return "".join(out)


def fragment_bases(d1, d2):
    """L of the decision: (bases of reads_1 + bases of reads_2) / pairs -- for mates of one length the reference's
    L * len(original_reads_files), shannon.py:613"""
    from . import _lib
    lib = _lib.lib()
    n = len(d1)
    return (int(lib.shn_reads_total_bases(d1.h)) + int(lib.shn_reads_total_bases(d2.h))) / n if n else 0.0


def apply(ctx, final, d1, d2, strand_specific, cutoff, max_span=MAX_SPAN):
    """the whole step on the final transcripts (a mapping name -> sequence in file order): (kept {name: sequence}, table, tsv text,
    text of rec_before_kallisto.fasta)"""
    names, seqs = [], []
    for name, seq in final.items():
        names.append(name)
        seqs.append(seq)
    before = "".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs))
    table = quantify(ctx, names, seqs, d1, d2, strand_specific, max_span)
    tsv = abundance_tsv(table)
    table["L"] = fragment_bases(d1, d2)
    kept_text = decide(tsv, before, float(cutoff), table["L"])
    kept, name = {}, None
    for line in kept_text.splitlines():
        if line.startswith(">"):
            name = line[1:]
        elif name is not None:
            kept[name] = line
    table["kept"] = len(kept)
    return kept, table, tsv, before
