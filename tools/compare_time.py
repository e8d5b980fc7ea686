#!/usr/bin/env python3
"""Time of the comparison against a reference transcriptome beside the assembly that made its input:
shannon_amd.synth pairs written as FASTA, `shannon.py --left --right` in this process, then shannon_amd.compare.compare_texts of
OUT/shannon.fasta against the planted isoforms -- one warm-up call, then --repeats timed ones.  Reported: the assembly's wall time
and the sum of its stage seconds (from its log), the call's wall time (median, min .. max), the compare.* kernel groups (HIP
events, with the launch sites' byte models) of the median call, index records / seed hits / candidate diagonals / rows, and the two
summary lines of reconstr_log.txt with false_positive's `rec,tot`.

    python tools/compare_time.py --pairs 1000000 --genes 1000 [--repeats 5] [--chain]

--chain: the chained form of the rule (compare_texts(chain=True)): the compare.chain group stands where compare.rows stood, and the
output also holds the blocks, the (query, target, orientation) groups chained and the rows with more than one block.

--dump DIR: the planted transcripts of a bench config against the final transcripts `bench.py --dump-outputs DIR` left there
(--genes / --exon-len / --seed as that run's preset; bench.py's default is --config 2: 20000 genes, exons 80 .. 600).  The dump holds
all transcripts only up to its 64 MB; beyond that it holds a seeded sample, and the summary lines are those of the sample (said in
the output: a sample of the reconstruction bounds the recovery from below, it does not measure it).  One JSON object per line."""
import argparse, json, os, statistics, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def timed_compare(ctx, ref_text, rec_text, strand_specific, repeats, chain=False):
    from shannon_amd import compare
    texts, st = compare.compare_texts(ctx, ref_text, rec_text, strand_specific, chain)   # warm-up: code objects, workspaces
    runs = []
    for _ in range(repeats):
        ctx.timer_reset()
        t0 = time.time()
        texts, st = compare.compare_texts(ctx, ref_text, rec_text, strand_specific, chain)
        wall = time.time() - t0
        tm, tb = ctx.timers(), ctx.timer_bytes()
        runs.append((wall, {k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)} for k, v in sorted(tm.items()) if k.startswith("compare.")}))
    runs.sort(key=lambda r: r[0])
    summary = [l for l in texts["reconstr_log.txt"].splitlines() if l.startswith("#")]
    extra = {k: st[k] for k in ("blocks", "groups", "multi_block_rows") if k in st}
    return {"chain": bool(chain), **extra, "compare_s": spread([r[0] for r in runs]), "kernels_of_median_call": runs[len(runs) // 2][1],
            "kernel_ms_sum_of_median_call": round(sum(k["ms"] for k in runs[len(runs) // 2][1].values()), 4),
            "records": st["records"], "hits": st["hits"], "candidates": st["candidates"], "rows": st["rows"], "summary": summary,
            "rec,tot": "%d,%d" % (st["rec"], st["tot"]), "ref_transcripts": ref_text.count(">"), "ref_bases": len(ref_text) - ref_text.count("\n"),
            "rec_transcripts": rec_text.count(">"), "rec_bases": len(rec_text) - rec_text.count("\n")}


def fasta_of(named):
    return "".join(">%s\n%s\n" % (n, s) for n, s in named)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--genes", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--exon-len", type=int, nargs=2, default=(80, 600))
    ap.add_argument("--dump", default=None)
    ap.add_argument("--chain", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from shannon_amd import synth, device
    seed = synth.DEFAULT_SEED if a.seed is None else a.seed
    if a.dump:
        iso, _ = synth.make_transcriptome(a.genes, seed, exon_len=tuple(a.exon_len))
        ref_text = fasta_of(("T%d" % k, s) for k, s in enumerate(synth.codes_to_strings(iso)))
        lens = np.load(os.path.join(a.dump, "transcript_lengths.npy")).astype(np.int64)
        pick = np.load(os.path.join(a.dump, "sample_index.npy")).astype(np.int64)
        bases = np.frombuffer(b"ACGTN", np.uint8)[np.load(os.path.join(a.dump, "sample_bases.npy")).astype(np.int64)].tobytes().decode()
        off = np.concatenate([[0], np.cumsum(lens[pick])])
        rec_text = fasta_of(("X%d" % j, bases[off[k]:off[k + 1]]) for k, j in enumerate(pick.tolist()))
        ctx = device.Context(0)
        out = timed_compare(ctx, ref_text, rec_text, False, a.repeats, a.chain)
        ctx.close()
        out.update(dump=a.dump, genes=a.genes, final_transcripts=int(len(lens)), dumped=int(len(pick)),
                   note="all final transcripts" if len(pick) == len(lens) else "a seeded SAMPLE of the final transcripts: the summary bounds the recovery from below")
        print(json.dumps(out))
        return
    import shannon
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=seed, sigma=0.5)
    ref_text = fasta_of(("T%d" % k, s) for k, s in enumerate(synth.codes_to_strings(iso)))
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(tmp, "r%d.fasta" % (k + 1)) for k in range(2)]
        for p, m in zip(files, (r1, r2)):
            synth.write_fasta(p, m)
        asm = []
        for rep in range(2):                                   # (the first run pays the code objects; the second is the one beside the call)
            out = os.path.join(tmp, "OUT%d" % rep)
            t0 = time.time()
            assert shannon.main(["shannon.py", "-o", out, "--left", files[0], "--right", files[1]]) == 0
            wall = time.time() - t0
            log = open(os.path.join(out, "log.txt")).read().splitlines()
            stages = json.loads([l for l in log if "stage seconds: " in l][0].split("stage seconds: ")[1])
            asm.append({"wall_s": round(wall, 4), "stages_s": round(sum(v for k, v in stages.items() if isinstance(v, float) and ": " not in k), 4)})
        rec_text = open(os.path.join(out, "shannon.fasta")).read()
    ctx = device.Context(0)
    res = timed_compare(ctx, ref_text, rec_text, False, a.repeats, a.chain)
    ctx.close()
    res.update(pairs=a.pairs, genes=a.genes, assembly_first_run=asm[0], assembly=asm[1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
