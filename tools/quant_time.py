#!/usr/bin/env python3
"""Time of `python -m shannon_amd.quant --single` on tools/abundance_time.py's workload: shannon_amd.synth pairs, the
mates of file 1 written as FASTQ and taken as single reads, the true isoforms as TRANSCRIPTS.fasta; the command runs in this
process, then the wall time of the call and the abundance.* kernel groups (HIP events, with the launch sites' byte models) from
quant_log.txt.

    python tools/quant_time.py --pairs 200000 --genes 50 [--cutoff 2.5] [--repeats 3] [-s]
"""
import argparse, json, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--cutoff", type=float, default=2.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("-s", action="store_true")
    a = ap.parse_args()
    from shannon_amd import quant, synth
    (r1, _r2), iso = synth.make_dataset(a.pairs, a.genes, seed=5, sigma=0.5)
    with tempfile.TemporaryDirectory() as tmp:
        reads = os.path.join(tmp, "r1.fastq")
        with open(reads, "w") as f:
            for i, s in enumerate(synth.codes_to_strings(r1)):
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        fasta = os.path.join(tmp, "t.fasta")
        with open(fasta, "w") as f:
            for j, s in enumerate(synth.codes_to_strings(iso)):
                f.write(">iso%d\n%s\n" % (j, s))
        for rep in range(a.repeats):
            out = os.path.join(tmp, "Q%d" % rep)
            t0 = time.time()
            rc = quant.main(["quant", fasta, "-o", out, "--single", reads, "--cutoff", str(a.cutoff)] + (["-s"] if a.s else []))
            wall = time.time() - t0
            assert rc == 0
            log = open(os.path.join(out, "quant_log.txt")).read().splitlines()
            kernels = json.loads([l for l in log if l.startswith("abundance kernels: ")][0].split("abundance kernels: ")[1])
            print(json.dumps({"reads": a.pairs, "genes": a.genes, "isoforms": len(iso), "strand_specific": a.s, "repeat": rep, "command_s": round(wall, 4),
                              "kernels": kernels, "log": [l for l in log if not l.startswith("abundance kernels: ")]}))


if __name__ == "__main__":
    main()
