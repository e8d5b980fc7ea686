"""Child process of tests/test_primitives_gpu.py, started with SHN_DEV_POISON=165 and SHN_DEV_POISON_WS=1 (read once per process):
every block of the caching allocator and every workspace slot, on EVERY request, is filled with the poison byte first, so a primitive
that reads a slot it did not write reads 0xA5.  Repeats the largest sort cases, the largest run cases, a scan of more than 1024 block sums and the table
build with duplicates, twice over (the second round meets slots the first one left full), and prints one line of counts of wrong
elements."""
import os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import primitives_cases as pc
import primitives_hooks as ph


def main():
    from shannon_amd import device
    assert os.environ.get("SHN_DEV_POISON") == "165" and os.environ.get("SHN_DEV_POISON_WS") == "1"
    ctx = device.Context(0)
    wrong = {"SORT_PAIRS": 0, "SORT_KEYS": 0, "RUNS": 0, "SCAN": 0, "TABLE": 0, "FIND": 0}
    for _round in range(2):
        for name in pc.SORT_CASES:
            c = pc.sort_case(name)
            if len(c.keys) != 70001:
                continue
            order = pc.stable_order(c.keys, c.lo, c.hi)
            ko, vo = ph.sort_pairs(ctx, c.keys, c.vals, c.lo, c.hi)
            wrong["SORT_PAIRS"] += int((ko != c.keys[order]).sum()) + int((vo != c.vals[order]).sum())
            wrong["SORT_KEYS"] += int((ph.sort_keys(ctx, c.keys, c.lo, c.hi) != c.keys[order]).sum())
        for name in pc.RUN_CASES:
            c = pc.run_case(name)
            if len(c.keys) != 70001:
                continue
            st = pc.run_starts(c.keys, c.shift)
            n_runs, rk, start, ln, pos = ph.sorted_runs(ctx, c.keys, c.shift)
            head = np.zeros(len(c.keys), dtype=np.uint64)
            head[st] = 1
            if n_runs != len(st):
                wrong["RUNS"] += max(n_runs, len(st))
            else:
                wrong["RUNS"] += (int((rk != c.keys[st]).sum()) + int((start != np.r_[st, len(c.keys)]).sum()) +
                                  int((ln != np.diff(np.r_[st, len(c.keys)])).sum()))
            wrong["RUNS"] += int((pos != np.r_[0, np.cumsum(head)].astype(np.uint64)).sum())
        v = pc.scan_case("random_%d" % ((1 << 21) + 5))
        want = np.zeros(len(v) + 1, dtype=np.uint64)
        np.cumsum(v.astype(np.uint64), out=want[1:])
        for with_total in (True, False):
            out, total = ph.scan(ctx, v, with_total)
            wrong["SCAN"] += int((out != want).sum()) + int(total != int(want[-1]))
        c = pc.table_case("dups")
        uk, sums = pc.table_reference("dups")
        q = pc.table_queries("dups")
        for how in sorted(ph.BUILDS):
            t = ph.BUILDS[how](ctx, c.keys, c.counts, c.k, c.canonical)
            tk, tc = t.download()
            o = np.argsort(tk, kind="stable")
            if len(tk) != len(uk):
                wrong["TABLE"] += max(len(tk), len(uk))
            else:
                wrong["TABLE"] += int((tk[o] != uk).sum()) + int((tc[o].astype(np.uint64) != sums).sum())
                want_idx = pc.expected_find(tk, q)
                for variant in (0, 1, 2):
                    wrong["FIND"] += int((ph.find(ctx, t, q, variant) != want_idx).sum())
            wrong["TABLE"] += int(t.total != int(sums.sum()))
            t.close()
    ctx.close()
    print(" ".join("%s %d" % kv for kv in sorted(wrong.items())), flush=True)


if __name__ == "__main__":
    main()
