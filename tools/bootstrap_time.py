#!/usr/bin/env python3
"""Time of the bootstrap replicates of `python -m shannon_amd.quant -b B` on tools/abundance_time.py's workload:
shannon_amd.synth pairs (strand-specific, as there) on their true isoforms.  The classes are made once; then, per repeat and one after
the other in this process,

    batched    abundance.bootstrap: resample + one EM over all replicates (the counts stay on the device)
    loop       the same counts (abundance.resample, checked here to give the batched call's counts) fed to B calls of abundance.em

each timed with a host clock around calls that end in a device synchronise, and the answers compared bit for bit.  Printed per repeat:
both times, their ratio, the abundance.resample / abundance.em_batch kernel groups of the batched call (HIP events, with the launch
sites' byte models), the time of abundance.resample alone and its draws per second.

    python tools/bootstrap_time.py --pairs 200000 --genes 50 [-b 100] [--seed 7] [--repeats 3]
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("-b", type=int, default=100)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    from shannon_amd import abundance, device, synth
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    seqs = synth.codes_to_strings(iso)
    ctx = device.Context(0)
    d1, d2 = device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2)
    try:
        cl = abundance.classes(ctx, seqs, d1, d2, True)
    finally:
        d1.close()
        d2.close()
    eff = abundance.eff_lengths([len(s) for s in seqs], cl["hist"])
    off, mem, n_c = cl["class_off"], cl["members"], cl["n_c"]
    N = int(n_c.sum())
    head = {"pairs": a.pairs, "genes": a.genes, "isoforms": len(seqs), "mapped": N, "classes": len(n_c), "members": len(mem), "B": a.b, "seed": a.seed}

    def batched():
        return abundance.bootstrap(ctx, off, mem, n_c, eff, a.b, a.seed, want_counts=True)

    def loop(counts):
        out = [abundance.em(ctx, off, mem, row, eff) for row in counts]
        return np.array([x for x, _ in out]), np.array([r for _, r in out], dtype=np.uint32)

    alpha, rounds, counts = batched()                            # warm-up of every shape the timed calls use: code objects, allocator
    loop(counts)
    abundance.resample(ctx, n_c, a.b, a.seed)
    for rep in range(a.repeats):
        ctx.sync()
        ctx.timer_reset()
        t0 = time.perf_counter()
        alpha, rounds, counts = batched()
        t_batched = time.perf_counter() - t0
        tm, tb = ctx.timers(), ctx.timer_bytes()
        t0 = time.perf_counter()
        alone = abundance.resample(ctx, n_c, a.b, a.seed)
        t_resample = time.perf_counter() - t0
        assert np.array_equal(alone, counts) and (counts.sum(axis=1) == N).all()
        t0 = time.perf_counter()
        alpha_loop, rounds_loop = loop(counts)
        t_loop = time.perf_counter() - t0
        assert np.array_equal(alpha_loop, alpha) and rounds_loop.tolist() == rounds.tolist(), "the batched EM differs from the loop"
        print(json.dumps(dict(head, repeat=rep, batched_s=round(t_batched, 6), loop_of_em_s=round(t_loop, 6), loop_over_batched=round(t_loop / t_batched, 2),
                              resample_alone_s=round(t_resample, 6), draws_per_s_by_the_call=round(a.b * N / t_resample),
                              rounds=sorted(set(int(r) for r in rounds)),
                              kernels={k: {"ms": round(v[0], 4), "regions": v[1], "bytes": tb.get(k, 0)} for k, v in sorted(tm.items())
                                       if k in ("abundance.resample", "abundance.em_batch")})), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
