"""Generator of tests/golden/filter_fp_decide.json.gz: the reference's own write_filtered_tr (filter_FP.py:7-25) run on made-up
depth files and FASTAs.  TEST INFRASTRUCTURE ONLY, like ref_harness.py: it needs the reference's sources (SHANNON_REFERENCE) and
is never run on the GPU machine.

filter_FP.py is translated into a scratch directory the way ref_harness.prepare_translated does it (tr -d '\\r' | expand -t 8,
python3 -m lib2to3 -w -n) and imported from there; nothing of it is written into the repository.  The fixture holds inputs and
outputs only:

    cases: [{"fasta": text of in_tr_file, "hits": depth-file lines per record (in file order),
             "kept": text of out_tr_file, "log": text of log_file}]

The depth file of a case has hits[j] lines `name<TAB>pos<TAB>depth` for record j (samtools depth prints one line per covered
position).  Lengths 1..40 and a spread up to 5,000; hits at ceil(0.9 len) - 1, ceil(0.9 len), len and 0; names with further
tokens behind the first (spaces and tabs), which write_filtered_tr drops.

    python tests/golden/make_filter_fp_golden.py
"""
import gzip, importlib.util, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_harness import REF


def translated_filter_fp(dst):
    txt = open(os.path.join(REF, "filter_FP.py"), "rb").read().replace(b"\r", b"")
    p = subprocess.run(["expand", "-t", "8"], input=txt, stdout=subprocess.PIPE, check=True)
    path = os.path.join(dst, "filter_FP.py")
    open(path, "wb").write(p.stdout)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", dst], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   check=True)
    spec = importlib.util.spec_from_file_location("ref_filter_FP", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ceil_09(n):
    """the smallest integer h with h >= 0.9 n, in integers: ceil(9 n / 10)"""
    return (9 * n + 9) // 10


def make_cases():
    import random
    rnd = random.Random(20240607)
    lengths = list(range(1, 41)) + [41, 49, 50, 51, 99, 100, 101, 110, 111, 250, 333, 999, 1000, 1001, 1111, 2500, 3333, 4990, 4999, 5000]
    headers = ["%s", "%s extra", "%s\tw=3.5\tn1,n2", "%s 0_1\t12.0\tx y z", "%s  two  spaces "]
    cases = []
    for which in range(4):                                   # one case per kind of hit count, every length in each
        recs, k = [], 0
        for n in lengths:
            c = ceil_09(n)
            h = (max(c - 1, 0), c, n, 0)[which]
            name = "tr%d_%d" % (which, k)
            recs.append((headers[k % len(headers)] % name, name, "".join(rnd.choice("ACGT") for _ in range(n)), h))
            k += 1
        cases.append(recs)
    mixed, k = [], 0                                         # ... and one with everything mixed, in random order
    for n in lengths:
        c = ceil_09(n)
        for h in sorted({max(c - 1, 0), c, n, 0, max(c - 2, 0), min(c + 1, n)}):
            name = "Shannon_mix_%d" % k
            mixed.append((headers[k % len(headers)] % name, name, "".join(rnd.choice("ACGT") for _ in range(n)), h))
            k += 1
    rnd.shuffle(mixed)
    cases.append(mixed[:120])
    return cases


def main():
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        ref = translated_filter_fp(tmp)
        for c, recs in enumerate(make_cases()):
            fa, depth, kept, log = (os.path.join(tmp, "%s%d" % (nm, c)) for nm in ("in.fasta", "rec.depth", "out.fasta", "rec.log"))
            text = "".join(">%s\n%s\n" % (hdr, seq) for hdr, _name, seq, _h in recs)
            open(fa, "w").write(text)
            with open(depth, "w") as f:
                for _hdr, name, _seq, h in recs:
                    for pos in range(h):
                        f.write("%s\t%d\t%d\n" % (name, pos + 1, 1 + pos % 7))
            ref.write_filtered_tr(depth, fa, kept, log)
            out.append({"fasta": text, "hits": [h for _hdr, _name, _seq, h in recs], "kept": open(kept).read(), "log": open(log).read()})
    path = os.path.join(HERE, "filter_fp_decide.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"source": "filter_FP.py:7-25 (write_filtered_tr), translated at run time", "cases": out}, sort_keys=True).encode())
    print("%s: %d cases, %d records, %d bytes" % (path, len(out), sum(len(c["hits"]) for c in out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
