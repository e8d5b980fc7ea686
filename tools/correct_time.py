#!/usr/bin/env python3
"""Time of `python -m shannon_amd.correct` in this process, on the input of tools/quorum_time.py: shannon_amd.synth
pairs written as FASTQ -- quality I, and in every fifth read one substituted base of quality #.  The command with 1 lane and with 4
lanes, with and without --trim: wall seconds, the seconds of its parts (both ingests, table, the addition of tables, correction,
trimming, writing, joining the parts) and the quorum.* kernel groups (HIP events, with the launch sites' byte models).  Run
tools/quorum_time.py in the same session for the `quorum` and `quorum files` stage seconds of `shannon.py --quorum` to hold them against.

    python tools/correct_time.py --pairs 200000 --genes 50 [--repeats 3]
"""
import argparse, json, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    from shannon_amd import synth, correct, device
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    rng = np.random.Generator(np.random.PCG64(9))
    with tempfile.TemporaryDirectory() as tmp:
        whole, lanes = [], []
        for k, m in enumerate((r1, r2)):
            m = np.array(m, dtype=np.uint8)
            n, L = m.shape
            rows = np.arange(k, n, 5)                                 # every fifth read: one base becomes another one, quality #
            cols = rng.integers(0, L, len(rows))
            m[rows, cols] = (m[rows, cols] + rng.integers(1, 4, len(rows)).astype(np.uint8)) & 3
            low = dict(zip(rows.tolist(), cols.tolist()))
            records = []
            for i, s in enumerate(synth.codes_to_strings(m)):
                q = "I" * L
                if i in low:
                    q = q[:low[i]] + "#" + q[low[i] + 1:]
                records.append("@r%d\n%s\n+\n%s\n" % (i, s, q))
            paths = []
            for name, lo, hi in [("all", 0, n)] + [("lane%d" % j, j * n // 4, (j + 1) * n // 4) for j in range(4)]:
                p = os.path.join(tmp, "r%d_%s.fastq" % (k + 1, name))
                with open(p, "w") as f:
                    f.write("".join(records[lo:hi]))
                paths.append(p)
            whole.append(paths[0])
            lanes.append(",".join(paths[1:]))
        ctx = device.Context(0)
        run = 0
        for rep in range(a.repeats):
            for n_lanes, files in ((1, whole), (4, lanes)):
                for trim in (False, True):
                    out = os.path.join(tmp, "OUT%d" % run)
                    run += 1
                    o = correct.parse_args(["correct", "-o", out, "--left", files[0], "--right", files[1]] + (["--trim"] if trim else []))
                    assert isinstance(o, dict), o
                    o.pop("gpus")
                    T = {}
                    ctx.timer_reset()
                    t0 = time.time()
                    s = correct.run(o, ctx, timings=T)
                    wall = time.time() - t0
                    log = open(os.path.join(out, "correct_log.txt")).read().splitlines()
                    kernels = json.loads([l for l in log if l.startswith("quorum kernels: ")][0].split("quorum kernels: ")[1])
                    print(json.dumps({"pairs": a.pairs, "genes": a.genes, "isoforms": len(iso), "repeat": rep, "lanes": n_lanes, "trim": trim,
                                      "wall_s": round(wall, 4), "parts_s": {k: round(v, 4) for k, v in T.items()}, "kernels": kernels,
                                      "counters": {k: v for k, v in s.items() if isinstance(v, int)}}))
        ctx.close()


if __name__ == "__main__":
    main()
