#!/usr/bin/env python3
"""Time of the --kallisto_cutoff step in one CLI run: shannon_amd.synth pairs written as FASTQ, `shannon.py --left
--right -s --kallisto_cutoff C` in this process, then timings["abundance"] and the abundance.* kernel groups (HIP events,
with the launch sites' byte models) from the run's log.

    python tools/abundance_time.py --pairs 200000 --genes 50 [--cutoff 2.5] [--repeats 3]
"""
import argparse, json, os, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--cutoff", type=float, default=2.5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import shannon
    from shannon_amd import synth
    (r1, r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, m in enumerate((r1, r2)):
            p = os.path.join(tmp, "r%d.fastq" % (k + 1))
            with open(p, "w") as f:
                for i, s in enumerate(synth.codes_to_strings(m)):
                    f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
            files.append(p)
        for rep in range(a.repeats):
            out = os.path.join(tmp, "OUT%d" % rep)
            rc = shannon.main(["shannon.py", "-o", out, "--left", files[0], "--right", files[1], "-s", "-K", "25", "--kallisto_cutoff", str(a.cutoff)])
            assert rc == 0
            log = open(os.path.join(out, "log.txt")).read().splitlines()
            stages = json.loads([l for l in log if "stage seconds: " in l][0].split("stage seconds: ")[1])
            line = [l for l in log if "--kallisto_cutoff" in l][0].split(": ", 1)[1]
            kernels = json.loads([l for l in log if "abundance kernels: " in l][0].split("abundance kernels: ")[1])
            print(json.dumps({"pairs": a.pairs, "genes": a.genes, "isoforms": len(iso), "repeat": rep, "abundance_s": stages.get("abundance"),
                              "all_stages_s": round(sum(v for v in stages.values() if isinstance(v, float)), 4), "kernels": kernels,
                              "log": line}))


if __name__ == "__main__":
    main()
