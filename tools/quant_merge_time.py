#!/usr/bin/env python3
"""Time of the merge of class sets on tools/abundance_time.py's workload: shannon_amd.synth pairs (strand-specific, as
there) on their true isoforms, cut into lanes of equal size.  Per repeat, in this process: abundance.quantify_parts over the lanes -- a
lane's classes, then the next lane's, then abundance.merge_classes and the tail -- and abundance.quantify on all pairs at once; the two
tables are compared (est_counts, eff_length, tpm equal as lists) and the abundance.* kernel groups of the lanes run are printed (HIP events,
with the launch sites' byte models), abundance.merge beside abundance.map.

    python tools/quant_merge_time.py --pairs 200000 --genes 50 [--lanes 8] [--repeats 3]
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from shannon_amd import abundance, device, synth
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    seqs = synth.codes_to_strings(iso)
    names = ["t%d" % j for j in range(len(seqs))]
    cuts = [a.pairs * k // a.lanes for k in range(a.lanes + 1)]
    ctx = device.Context(0)

    def lanes():
        for lo, hi in zip(cuts, cuts[1:]):
            d1, d2 = device.Reads.from_codes(ctx, r1[lo:hi]), device.Reads.from_codes(ctx, r2[lo:hi])
            try:
                yield d1, d2
            finally:
                d1.close()
                d2.close()

    def whole():
        d1, d2 = device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2)
        try:
            return abundance.quantify(ctx, names, seqs, d1, d2, True)
        finally:
            d1.close()
            d2.close()
    abundance.quantify_parts(ctx, names, seqs, lanes(), True)        # warm-up of both: code objects, allocator
    whole()
    for rep in range(a.repeats):
        ctx.sync()
        ctx.timer_reset()
        t0 = time.perf_counter()
        t = abundance.quantify_parts(ctx, names, seqs, lanes(), True)
        t_lanes = time.perf_counter() - t0
        tm, tb = ctx.timers(), ctx.timer_bytes()
        t0 = time.perf_counter()
        w = whole()
        t_whole = time.perf_counter() - t0
        same = all(t[k] == w[k] for k in ("est_counts", "eff_length", "tpm", "mapped", "fragments", "classes", "rounds"))
        print(json.dumps({"pairs": a.pairs, "genes": a.genes, "isoforms": len(seqs), "lanes": a.lanes, "repeat": rep, "lists_in": t["lists"],
                          "classes_out": t["classes"], "mapped": t["mapped"], "equal_to_one_set": same, "lanes_s": round(t_lanes, 4),
                          "one_set_s": round(t_whole, 4),
                          "kernels": {k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)} for k, v in sorted(tm.items()) if k.startswith("abundance.")}}))
        assert same, "the lanes' table differs from the one-set table"
    ctx.close()


if __name__ == "__main__":
    main()
