"""Generator of tests/golden/kallisto_decide.json.gz: the reference's own filter_using_kallisto (filter_kallisto.py:8-21) run on
made-up abundance.tsv files and FASTAs.  TEST INFRASTRUCTURE ONLY, like make_filter_fp_golden.py: it needs the reference's sources
(SHANNON_REFERENCE) and is never run on the GPU machine.

filter_kallisto.py is translated into a scratch directory the way make_filter_fp_golden.py does it (tr -d '\\r' | expand -t 8,
python3 -m lib2to3 -w -n) and imported from there (its `import rc_gnu`, which the function does not use, is met with an empty
module); nothing of it is written into the repository.  The fixture holds inputs and outputs only:

    cases: [{"what": ..., "tsv": text of ab_file, "fasta": text of rec_file, "cutoff": COV_CUTOFF, "L": L, "kept": text of out_file}]

Cases: cov = float(est_counts) / float(eff_length) * L equal to the cutoff, one ulp below it and one ulp above it, for many
(est_counts, eff_length, L); headers with further tokens behind the name (spaces and tabs); sequences over several lines, blank
lines and a sequence before the first header (write_now starts True and carries over); names absent from the table; est_counts 0;
floats written with repr, as abundance.abundance_tsv writes them.

    python tests/golden/make_kallisto_golden.py
"""
import gzip, importlib.util, json, math, os, subprocess, sys, tempfile, types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_harness import REF

HEADER = "target_id\tlength\teff_length\test_counts\ttpm\n"


def translated_filter_kallisto(dst):
    txt = open(os.path.join(REF, "filter_kallisto.py"), "rb").read().replace(b"\r", b"")
    p = subprocess.run(["expand", "-t", "8"], input=txt, stdout=subprocess.PIPE, check=True)
    path = os.path.join(dst, "filter_kallisto.py")
    open(path, "wb").write(p.stdout)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", dst], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   check=True)
    sys.modules.setdefault("rc_gnu", types.ModuleType("rc_gnu"))
    spec = importlib.util.spec_from_file_location("ref_filter_kallisto", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tsv_of(rows):
    return HEADER + "".join("%s\t%d\t%s\t%s\t%s\n" % (n, ln, repr(float(el)), repr(float(ec)), repr(float(tpm))) for n, ln, el, ec, tpm in rows)


def make_cases():
    import random
    rnd = random.Random(20240611)

    def seq(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))
    cases = []
    # ---- the comparison itself: one transcript, the cutoff at cov, one ulp above cov (cov is one ulp below) and one ulp below cov
    for k in range(40):
        ec = rnd.choice([0.5, 1.0, 3.0, 7.25]) * rnd.random() * 10 ** rnd.randint(0, 4) if k % 5 else float(rnd.randint(1, 5000))
        el = rnd.choice([1.0, 98.5, 301.0]) + rnd.random() * 10 ** rnd.randint(0, 3)
        L = rnd.choice([200, 200.0, 150, 101.5, 164.37])
        cov = float(repr(ec)) / float(repr(el)) * L
        s = seq(60 + k)
        for what, cut in (("equal", cov), ("one ulp below", math.nextafter(cov, math.inf)), ("one ulp above", math.nextafter(cov, -math.inf))):
            cases.append({"what": "cov %s the cutoff" % what, "tsv": tsv_of([("t%d" % k, len(s), el, ec, 1e6)]), "fasta": ">t%d\n%s\n" % (k, s),
                          "cutoff": cut, "L": L})
    # ---- the texts
    headers = ["%s", "%s extra", "%s\tw=3.5\tn1,n2", "%s 0_1\t12.0\tx y z", "%s  two  spaces "]
    rows, fa = [], []
    for k in range(60):
        name = "Shannon_%d_%d" % (k // 7, k)
        s = seq(rnd.randint(80, 400))
        ec = 0.0 if k % 6 == 0 else rnd.random() * 50
        el = float(len(s)) if k % 4 == 0 else len(s) - 40.25
        if k % 11 != 3:                                      # (k % 11 == 3: a name the table does not hold)
            rows.append((name, len(s), el, ec, rnd.random() * 1e5))
        hdr = ">" + headers[k % len(headers)] % name
        if k % 3 == 0:                                       # the sequence over several lines, a blank line inside some
            cut = sorted(rnd.sample(range(1, len(s)), 3))
            parts = [s[:cut[0]], s[cut[0]:cut[1]], s[cut[1]:cut[2]], s[cut[2]:]]
            body = "\n".join(parts[:2]) + ("\n\n" if k % 6 == 0 else "\n") + "\n".join(parts[2:]) + "\n"
        else:
            body = s + "\n"
        fa.append(hdr + "\n" + body)
    rnd.shuffle(rows)                                        # (the table need not be in the FASTA's order)
    text = "".join(fa)
    for cut in (0.0, 1.0, 5.0, 20.0, 1e9):
        cases.append({"what": "texts", "tsv": tsv_of(rows), "fasta": text, "cutoff": cut, "L": 200})
    # a sequence line and a blank line before the first header: write_now starts True; then a dropped record's lines stay dropped
    cases.append({"what": "lines before the first header", "tsv": tsv_of([("a", 100, 60.0, 10.0, 5.0), ("b", 100, 60.0, 0.1, 5.0)]),
                  "fasta": "ACGTACGT\n\n>b\nAAAA\nCCCC\n>a x\nGGGG\nTTTT\n>c\nACAC\n", "cutoff": 2.5, "L": 200})
    cases.append({"what": "an empty table", "tsv": HEADER, "fasta": "ACGT\n>a\nAAAA\n", "cutoff": 0.0, "L": 200})
    return cases


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = translated_filter_kallisto(tmp)
        cases = make_cases()
        for c, case in enumerate(cases):
            fa, ab, out = (os.path.join(tmp, "%s%d" % (nm, c)) for nm in ("rec.fasta", "abundance.tsv", "out.fasta"))
            open(fa, "w").write(case["fasta"])
            open(ab, "w").write(case["tsv"])
            ref.filter_using_kallisto(fa, ab, out, case["cutoff"], case["L"])
            case["kept"] = open(out).read()
    path = os.path.join(HERE, "kallisto_decide.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"source": "filter_kallisto.py:8-21 (filter_using_kallisto), translated at run time", "cases": cases},
                           sort_keys=True).encode())
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
