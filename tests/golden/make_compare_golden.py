"""Generator of tests/golden/compare_decide.json.gz: the reference's own analyzer_blat_noExp (tester.py:135-167) and false_positive
(tester.py:269-317) run on made-up PSL files and FASTAs.  TEST INFRASTRUCTURE ONLY, like make_kallisto_golden.py: it needs the
reference's sources (SHANNON_REFERENCE) and is never run on the GPU machine.

tester.py is translated into a scratch directory the way make_kallisto_golden.py does it (tr -d '\\r' | expand -t 8 -- the file mixes
tabs and spaces --, python3 -m lib2to3 -w -n) and imported from there; nothing of it is written into the repository.  Under Python 3
a dict keeps the order of first insertion, which is the order DESIGN.md 3.12 states for the two logs, and str(float) is repr.  The
fixture holds inputs and outputs only:

    cases: [{"what": ..., "psl": text of reconstr_per.txt, "fasta": text of the reconstructed FASTA,
             "log": text of reconstr_log.txt, "rev_log": text of reconstr_rev_log.txt, "printed": what false_positive printed}]

Cases: ties in matches between two targets of one query and between two queries of one target (in both orders); matches exactly at
0.9 * size (sizes that are multiples of 10: the product in double is the integer itself), one below and one above, and around
0.9 * 2049 = 1844.1; targets no line names; multi-line records, headers with further tokens, a header without a sequence,
two records of one name; the empty PSL file; random files.

    python tests/golden/make_compare_golden.py
"""
import contextlib, gzip, importlib.util, io, json, os, random, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_harness import REF


def translated_tester(dst):
    txt = open(os.path.join(REF, "tester.py"), "rb").read().replace(b"\r", b"")
    p = subprocess.run(["expand", "-t", "8"], input=txt, stdout=subprocess.PIPE, check=True)
    path = os.path.join(dst, "tester.py")
    open(path, "wb").write(p.stdout)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", dst], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   check=True)
    spec = importlib.util.spec_from_file_location("ref_tester", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def psl(m, q, q_size, t, t_size, strand="+", mm=0, q0=0, t0=0):
    n = m + mm
    return "\t".join(str(x) for x in (m, mm, 0, 0, 0, 0, 0, 0, strand, q, q_size, q0, q0 + n, t, t_size, t0, t0 + n, 1, "%d," % n, "%d," % q0,
                                      "%d," % t0)) + "\n"


def fasta(recs, width=0):
    out = []
    for header, n in recs:
        out.append(">%s\n" % header)
        s = ("ACGT" * (n // 4 + 1))[:n]
        out += [s[k:k + width] + "\n" for k in range(0, n, width)] if width else ([s + "\n"] if n else [])
    return "".join(out)


def make_cases():
    rnd = random.Random(20240719)
    cases = []
    # ---- ties
    fa = fasta([("x0", 300), ("x1", 300), ("x2", 250)])
    for what, lines in (
            ("two targets of one query tie in matches: the first line stays", [psl(120, "r0", 200, "x0", 300), psl(120, "r0", 200, "x1", 300)]),
            ("... in the other order", [psl(120, "r0", 200, "x1", 300), psl(120, "r0", 200, "x0", 300)]),
            ("two queries of one target tie in matches: the last line stays", [psl(120, "r0", 200, "x0", 300), psl(120, "r1", 400, "x0", 300)]),
            ("... in the other order", [psl(120, "r1", 400, "x0", 300), psl(120, "r0", 200, "x0", 300)]),
            ("two queries of one target tie in matches / qSize", [psl(60, "r0", 200, "x0", 300), psl(120, "r1", 400, "x0", 300), psl(30, "r2", 100, "x0", 300)]),
            ("a later line with more matches takes over, one with fewer does not",
             [psl(100, "r0", 200, "x0", 300), psl(150, "r0", 200, "x1", 300), psl(140, "r0", 200, "x2", 250), psl(90, "r1", 100, "x2", 250, "-", 3)])):
        cases.append({"what": what, "psl": "".join(lines), "fasta": fa})
    # ---- the 90 % comparisons
    for size in (100, 70, 110, 130, 10, 1000, 2049):
        for dm in (-1, 0, 1):
            m = int(0.9 * size + 0.5) + dm
            cases.append({"what": "matches %d of qSize %d" % (m, size), "psl": psl(m, "r0", size, "x0", 5000) + psl(40, "r1", 400, "x1", 600),
                          "fasta": fasta([("x0", 5000), ("x1", 600)])})
            cases.append({"what": "matches %d of tSize %d" % (m, size), "psl": psl(m, "r0", 5000, "x0", size) + psl(m, "r1", size + 1, "x1", size + 2),
                          "fasta": fasta([("x0", size), ("x1", size + 2), ("x2", 77)])})
    # both 90 % tests of one target, in both orders (the code 1 -> 2 path and the 2 that stays)
    cases.append({"what": "min(qSize, tSize) first, tSize later", "psl": psl(90, "r0", 100, "x0", 400) + psl(380, "r1", 900, "x0", 400),
                  "fasta": fasta([("x0", 400)])})
    cases.append({"what": "tSize first, min(qSize, tSize) later", "psl": psl(380, "r1", 900, "x0", 400) + psl(90, "r0", 100, "x0", 400),
                  "fasta": fasta([("x0", 400)])})
    # ---- the texts
    recs = [("Shannon_0_0 w=3.5", 400), ("Shannon_0_1\tx y", 120), ("Shannon_1_0", 0), ("Shannon_1_1", 333), ("Shannon_0_1", 30), ("Shannon_2_0  two", 64)]
    lines = [psl(100, "ENST1", 500, "Shannon_0_0", 400, "-", 2), psl(140, "ENST2", 150, "Shannon_0_1", 150), psl(64, "ENST1", 500, "Shannon_2_0", 64)]
    cases.append({"what": "headers with further tokens, a header without a sequence, two records of one name, a target no line names",
                  "psl": "".join(lines), "fasta": fasta(recs, width=50)})
    cases.append({"what": "the empty PSL file", "psl": "", "fasta": fasta([("x0", 100), ("x1", 50)])})
    cases.append({"what": "the empty PSL file and the empty FASTA", "psl": "", "fasta": ""})
    # ---- random files
    for k in range(12):
        n_q, n_t = rnd.randint(1, 12), rnd.randint(1, 15)
        q_size = [rnd.choice([50, 100, 110, 250, 999, rnd.randint(40, 3000)]) for _ in range(n_q)]
        t_size = [rnd.choice([60, 100, 130, 500, rnd.randint(40, 3000)]) for _ in range(n_t)]
        lines = []
        for i in range(n_q):
            for j in range(n_t):
                if rnd.random() < 0.35:
                    top = min(q_size[i], t_size[j])
                    m = rnd.choice([top, int(0.9 * top), int(0.9 * top) + 1, rnd.randint(30, max(30, top)), 30])
                    lines.append(psl(min(m, top), "ref%d" % i, q_size[i], "Shannon_%d" % j, t_size[j], rnd.choice("+-"), rnd.randint(0, 3)))
        cases.append({"what": "random %d" % k, "psl": "".join(lines), "fasta": fasta([("Shannon_%d" % j, t_size[j]) for j in range(n_t)], width=rnd.choice([0, 60]))})
    return cases


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = translated_tester(tmp)
        cases = make_cases()
        for c, case in enumerate(cases):
            per, fa, log, rev = (os.path.join(tmp, "%s%d" % (nm, c)) for nm in ("per.txt", "rec.fasta", "log.txt", "rev_log.txt"))
            open(per, "w").write(case["psl"])
            open(fa, "w").write(case["fasta"])
            ref.analyzer_blat_noExp(per, log, None, 0)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ref.false_positive(fa, per, rev)
            case["log"], case["rev_log"], case["printed"] = open(log).read(), open(rev).read(), buf.getvalue()
    path = os.path.join(HERE, "compare_decide.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"source": "tester.py:135-167 (analyzer_blat_noExp), 269-317 (false_positive), translated at run time", "cases": cases},
                           sort_keys=True).encode())
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
