"""Generator of tests/golden/abundance_em_bits.json: the bits of shannon_amd.abundance.em (shn_abundance_em, DESIGN.md 3.10 rule 4) as
this project's own library computed them before the single-replicate EM became the one-slot case of the batched one.  Needs the built
library and a GPU; nothing of the reference.

Per case of tests/abundance_cases.em_golden_names() -- every entry of em_cases() and union_case() -- and per row of em_golden_case(name)
(the case's own n_c, then the 65 rows of bootstrap_cases.brute_counts_np(n_c, 65, 7); the union case: its 5 rows) the file holds

    [label, rounds, SHA-256 of alpha.tobytes()]            alpha: float64[m], little-endian, as abundance.em returns it

tests/test_abundance_gpu.py holds abundance.em and abundance.em_batch to these.

    python tests/golden/make_abundance_em_golden.py            writes the file
    python tests/golden/make_abundance_em_golden.py --check    recomputes and compares instead
"""
import hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import abundance_cases as ac

PATH = os.path.join(HERE, "abundance_em_bits.json")


def digest(alpha):
    assert alpha.dtype == "<f8" and alpha.flags["C_CONTIGUOUS"]
    return hashlib.sha256(alpha.tobytes()).hexdigest()


def compute(ctx):
    from shannon_amd import abundance
    cases = {}
    for name in ac.em_golden_names():
        lists, matrix, eff, labels = ac.em_golden_case(name)
        off, mem = ac.csr(lists)
        rows = []
        for label, n_c in zip(labels, matrix):
            alpha, rounds = abundance.em(ctx, off, mem, n_c, eff)
            rows.append([label, int(rounds), digest(alpha)])
        cases[name] = rows
        print("%s: %d rows, rounds %s" % (name, len(rows), sorted(set(r[1] for r in rows))), flush=True)
    return {"source": "shannon_amd.abundance.em at the commit before shn_abundance_em ran through the batched EM", "cases": cases}


def write(obj):
    """a row a line"""
    cases = ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(json.dumps(row) for row in rows)) for name, rows in sorted(obj["cases"].items()))
    with open(PATH, "w") as f:
        f.write('{"source": %s,\n"cases": {\n%s\n}}\n' % (json.dumps(obj["source"]), cases))


def main():
    from shannon_amd import device
    ctx = device.Context(0)
    try:
        got = compute(ctx)
    finally:
        ctx.close()
    if "--check" in sys.argv:
        want = json.load(open(PATH))["cases"]
        bad = []
        for name in sorted(set(want) | set(got["cases"])):
            g, w = got["cases"].get(name, []), want.get(name, [])
            bad += [(name, "%d rows for %d" % (len(g), len(w)))] if len(g) != len(w) else [(name, a[0]) for a, b in zip(g, w) if a != b]
        print("check: %d rows differ %s" % (len(bad), bad[:10]))
        return 1 if bad else 0
    write(got)
    print("%s: %d cases, %d bytes" % (PATH, len(got["cases"]), os.path.getsize(PATH)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
