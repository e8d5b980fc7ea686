"""Quantify a set of transcripts against single-end or paired reads: the quantifier of --kallisto_cutoff as a command of its own
(filter_kallisto.py:23-31 -- `kallisto index` + `kallisto quant`, with `--single -l 200 -s 20` for one read file).

    python -m shannon_amd.quant TRANSCRIPTS.fasta -o DIR (--single R | --left R1 --right R2) [-s] [--cutoff C] [-l MEAN] [--sd SD]
                                [-b B [--seed S]]

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

    targets       (names, sequences) of the FASTA text; a duplicate id, an empty id or an empty sequence raises QuantError
    load_reads    a read file -> a resident device.Reads (the device ingest, else record by record)
    quantify_files  the whole step
    main          the command: 0 done, 2 a usage error (with a message)

`targets` and the argument checks of `main` need neither the library nor a GPU."""
import json
import os
import re
import sys

USAGE = ("usage: python -m shannon_amd.quant TRANSCRIPTS.fasta -o DIR (--single R | --left R1 --right R2) [-s] [--cutoff C] [-l MEAN] [--sd SD] [-b B [--seed S]]\n"
         "  TRANSCRIPTS.fasta  the transcripts to quantify (2-line or multi-line FASTA; the id is the header's first token)\n"
         "  -o DIR             where abundance.tsv, quant_log.txt and filtered.fasta go\n"
         "  --single R         single-end reads (FASTA or FASTQ)\n"
         "  --left R1 --right R2  paired reads, mates in the same order\n"
         "  -s                 strand-specific: single reads are placed forward only, pairs as (R1, RC(R2)) only\n"
         "  --cutoff C         also write filtered.fasta: the transcripts with est_counts / eff_length * L >= C\n"
         "  -l MEAN, --sd SD   single-end only: mean and standard deviation of the fragment-length model (200, 20)\n"
         "  -b B               also B >= 1 bootstrap replicates: bs_abundance_<b>.tsv and bootstrap_summary.tsv\n"
         "  --seed S           with -b: the seed of the resampling, an integer in 0 .. 2^64 - 1 (0)\n")


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
    log.append("abundance kernels: " + json.dumps({k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)}
                                                    for k, v in sorted(tm.items()) if k.startswith("abundance.")}))
    with open(os.path.join(out_dir, "quant_log.txt"), "w") as f:
        f.write("".join(l + "\n" for l in log))
    return table


def parse_args(argv):
    """argv (the program's name first) -> a dict of quantify_files' arguments, or a message (a usage error)"""
    takes = {"-o": "out_dir", "--single": "single", "--left": "left", "--right": "right", "--cutoff": "cutoff", "-l": "mean", "--sd": "sd",
             "-b": "bootstraps", "--seed": "seed"}
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
    for k in ("fasta", "single", "left", "right"):
        if k in o and not os.path.isfile(o[k]):
            return "%s: no such file" % o[k]
    return o


def main(argv):
    """python -m shannon_amd.quant ...; 0 done, 2 a usage error or a refused input (a message on stderr)"""
    o = parse_args(argv)
    if isinstance(o, str):
        sys.stderr.write("%s\n%s" % (o, USAGE))
        return 2
    try:
        t = quantify_files(**o)                                 # (the transcripts are checked before the device is touched)
    except QuantError as ex:
        sys.stderr.write("%s\n" % ex)
        return 2
    print("%d of %d %s mapped, %d classes, %d EM rounds%s" % (t["mapped"], t["fragments"], "pairs" if t["paired"] else "reads", t["classes"], t["rounds"],
                                                          "; %d of %d transcripts kept" % (t["kept"], len(t["names"])) if "kept" in t else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
