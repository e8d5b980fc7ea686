#!/usr/bin/env python3
"""Time of the --quorum step in one CLI run: shannon_amd.synth pairs written as FASTQ -- quality I, and in every
fifth read one substituted base of quality # -- `shannon.py --left --right -s --quorum` in this process, then timings["quorum"]
beside the ingest and counting times of the same run, and the quorum.* kernel groups (HIP events, with the launch sites' byte models)
from the run's log.

    python tools/quorum_time.py --pairs 200000 --genes 50 [--repeats 3]
"""
import argparse, json, os, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import shannon
    from shannon_amd import synth
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    rng = np.random.Generator(np.random.PCG64(9))
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, m in enumerate((r1, r2)):
            m = np.array(m, dtype=np.uint8)
            n, L = m.shape
            rows = np.arange(k, n, 5)                                 # every fifth read: one base becomes another one, quality #
            cols = rng.integers(0, L, len(rows))
            m[rows, cols] = (m[rows, cols] + rng.integers(1, 4, len(rows)).astype(np.uint8)) & 3
            low = dict(zip(rows.tolist(), cols.tolist()))
            p = os.path.join(tmp, "r%d.fastq" % (k + 1))
            with open(p, "w") as f:
                for i, s in enumerate(synth.codes_to_strings(m)):
                    q = "I" * L
                    if i in low:
                        q = q[:low[i]] + "#" + q[low[i] + 1:]
                    f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
            files.append(p)
        for rep in range(a.repeats):
            out = os.path.join(tmp, "OUT%d" % rep)
            rc = shannon.main(["shannon.py", "-o", out, "--left", files[0], "--right", files[1], "-s", "-K", "25", "--quorum"])
            assert rc == 0
            log = open(os.path.join(out, "log.txt")).read().splitlines()
            stages = json.loads([l for l in log if "stage seconds: " in l][0].split("stage seconds: ")[1])
            line = [l for l in log if "--quorum: " in l][0].split(": ", 1)[1]
            kernels = json.loads([l for l in log if "quorum kernels: " in l][0].split("quorum kernels: ")[1])
            print(json.dumps({"pairs": a.pairs, "genes": a.genes, "isoforms": len(iso), "repeat": rep, "quorum_s": stages.get("quorum"),
                              "quorum_parts_s": {k[8:]: v for k, v in stages.items() if k.startswith("quorum: ")}, "quorum_files_s": stages.get("quorum files"), "ingest_s": stages.get("ingest"), "count_s": stages.get("count"),
                              "all_stages_s": round(sum(v for k, v in stages.items() if isinstance(v, float) and not k.startswith("quorum: ")), 4), "kernels": kernels,
                              "log": line}))


if __name__ == "__main__":
    main()
