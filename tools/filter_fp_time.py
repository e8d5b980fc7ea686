#!/usr/bin/env python3
"""What --filter_FP costs: a step of the pipeline with filter_fp=True against the same step with filter_fp=False on the same
resident batch (BASELINE configs[1]-shaped input: one gene family, 2 x 100 bases, 0.5 % errors), at 1 M and 10 M pairs.

    python tools/filter_fp_time.py [--pairs 1000000 10000000] [--repeats 3] [--out results.json]

Per size: one warm-up step of each kind, then `repeats` steps of each kind, alternating.  Reported: the median and the spread
(min .. max) of the step's wall time with and without the flag, of the stage's wall time (timings["filter_FP"]: parsing the
texts on the host, the device call, writing the filtered texts), of the kernels' HIP-event time per timer slot
(filter_fp.index / .map / .count) with the algorithmic bytes their launch sites declare; routes looked at / fragments placed;
transcripts kept / total; and -- for scale -- the rate of the tests' brute force (tests/filter_fp_cases.py) on 300 routed
pairs of the same input.  Then the owner's half of the filter on N ranks alone (shn_filter_fp_count, timer filter_fp.merge): the OR
of --merge-covers synthetic bitmaps (8: one per rank of a node) and the count per transcript over --merge-bases bases of
transcripts of 200 .. 3,000 bases, with the bytes the launch site declares.  One JSON object on the last line of the output."""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def time_merge(ctx, n_covers, n_bases, repeats, seed):
    """shn_filter_fp_count on synthetic input: the kernel's HIP-event time (filter_fp.merge) and the call's wall time (the upload of
    the bitmaps included), one warm-up call first; the result is held against the numpy mirror on the first 2,000 transcripts"""
    import numpy as np
    from shannon_amd import filter_fp
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(200, 3001, max(1, n_bases // 1600))
    t_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n_words = (int(t_off[-1]) + 63) // 64
    covers = rng.integers(0, 1 << 63, (n_covers, n_words), dtype=np.uint64) & rng.integers(0, 1 << 63, (n_covers, n_words), dtype=np.uint64)
    hits = filter_fp.hits_from_bitmaps(ctx, covers, t_off)
    k = min(2000, len(lens))
    w = (int(t_off[k]) + 63) // 64
    assert hits[:k].tolist() == filter_fp.hits_from_bitmaps(None, covers[:, :w], t_off[:k + 1]).tolist()
    ms, wall = [], []
    for _ in range(repeats):
        ctx.timer_reset()
        t0 = time.time()
        filter_fp.hits_from_bitmaps(ctx, covers, t_off)
        ctx.sync()
        wall.append(time.time() - t0)
        ms.append(ctx.timers()["filter_fp.merge"][0])
    byts = ctx.timer_bytes()["filter_fp.merge"]
    return {"covers": n_covers, "transcripts": int(len(lens)), "bases": int(t_off[-1]), "bitmap_bytes": int(covers.nbytes), "kernel_ms": spread(ms),
            "call_seconds": spread(wall), "kernel_bytes": byts, "kernel_GBps_at_median": round(byts / (statistics.median(ms) * 1e-3) / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240501)
    ap.add_argument("--merge-covers", type=int, default=8)
    ap.add_argument("--merge-bases", type=int, default=50_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import bench
    import shannon_amd
    from shannon_amd import device, pipeline, kmers_for_component as kfc
    import filter_fp_cases as fc
    ctx = device.Context(0)
    report = {"input": "one gene family (bench.py --config 1 generator), 2 x 100 bases, 0.5 % substitutions, K = 25", "sizes": []}
    for n_pairs in args.pairs:
        r1, r2 = bench.gen_reads(n_pairs, args.seed, 1, "cuda")
        d1, d2 = device.Reads.from_codes(ctx, r1), device.Reads.from_codes(ctx, r2)
        store = kfc.ReadStore(r1, r2)

        def step(flag, keep=False):
            T = {}
            ctx.timer_reset()
            t0 = time.time()
            R = pipeline.assemble_resident(ctx, d1, d2, store, K=25, sample="t", seed=0, timings=T, filter_fp=flag, keep_partitioning=keep)
            ctx.sync()
            wall = time.time() - t0
            kern = {k: v for k, v in ctx.timers().items() if k.startswith("filter_fp.")}
            byts = {k: v for k, v in ctx.timer_bytes().items() if k.startswith("filter_fp.")}
            return R, wall, T, kern, byts
        step(False)
        step(True)
        walls = {False: [], True: []}
        stage, kern_ms, last = [], {}, None
        for _ in range(args.repeats):
            for flag in (False, True):
                R, wall, T, kern, byts = step(flag, keep=flag)
                walls[flag].append(wall)
                if flag:
                    stage.append(T["filter_FP"])
                    for k, (ms, _n) in kern.items():
                        kern_ms.setdefault(k, []).append(ms)
                    last = (R, byts)
        R, byts = last
        entry = {"pairs": n_pairs, "step_seconds_without": spread(walls[False]), "step_seconds_with": spread(walls[True]),
                 "stage_seconds": spread(stage), "kernel_ms": {k: spread(v) for k, v in kern_ms.items()}, "kernel_bytes": byts,
                 "kernel_GBps_at_median": {k: round(byts.get(k, 0) / (statistics.median(v) * 1e-3) / 1e9, 2) for k, v in kern_ms.items() if statistics.median(v) > 0},
                 "routes": R.filter_fp_stats["routes"], "placed": R.filter_fp_stats["placed"],
                 "transcripts": R.filter_fp_stats["transcripts"], "kept": R.filter_fp_stats["kept"],
                 "final_transcripts_with": len(R.final)}
        # the brute force on 300 routed pairs of the partition with the most routes
        name = max(R.partitions, key=lambda nm: R.partitions[nm]["n_reads_routed"])
        idx = np.asarray(R.partitioning["routes"][name][:300], dtype=np.int64)
        frag = np.unique(idx % n_pairs)
        seqs = [l for l in R.partitions[name]["reconstructed_org_fasta"].splitlines() if not l.startswith(">")]
        A = np.frombuffer(b"ACGT", np.uint8)
        case = fc.make_case(seqs, [0] * len(seqs), 1, [A[r1[i]].tobytes().decode() for i in frag], [A[r2[i]].tobytes().decode() for i in frag],
                            (np.zeros(len(frag), np.uint32), np.arange(len(frag))), False)
        t0 = time.time()
        fc.brute_hits(case)
        dt = time.time() - t0
        entry["brute_force"] = {"pairs": int(len(frag)), "transcripts": len(seqs), "seconds": round(dt, 3), "pairs_per_second": round(len(frag) / dt, 1)}
        report["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
        del R, last
        d1.close()
        d2.close()
    if args.merge_covers > 0 and args.merge_bases > 0:
        report["merge"] = time_merge(ctx, args.merge_covers, args.merge_bases, args.repeats, args.seed)
        print(json.dumps(report["merge"]), flush=True)
    ctx.close()
    line = json.dumps(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
