"""Child process of tests/test_ext_walks_gpu.py, started with SHN_DEV_POISON=165 and SHN_DEV_POISON_WS=1 (read once per process): every
block of the caching allocator and every workspace slot, on EVERY request, is filled with the poison byte first, so a kernel of the
extension that reads what it did not write reads 0xA5.  Runs the dependency chain, a dense table and the planted lengths twice over
(the second round meets what the first one left behind) and prints, per case, the number of ranks whose n_right, n_left, tot_weight
or contig is not the reference's."""
import os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ext_setup_cases as ec
import ext_walk_cases as wc
import primitives_hooks as ph

CASES = ("chain_canon", "dense_6_canon", "lengths_26_canon")


def wrong_ranks(ctx, name):
    from shannon_amd import extension_correction as xc
    case = wc.table(name)
    t = ph.table_create(ctx, case.keys, case.counts, case.k, case.canonical)
    try:
        keys, counts = t.download()
        ref = ec.reference(keys, counts, t.k, t.canonical, 3)
        w = wc.walk_reference(ref, t.k)
        ext = xc.Extension(ctx, t, 3, max_iterations=2000)
        try:
            if ext.n_walks != len(ref.order):
                return max(ext.n_walks, len(ref.order))
            nr, nl, tw = ext.stats()
            bad = (nr != w.n_right) | (nl != w.n_left) | (tw != w.tot_weight)
            live = np.flatnonzero((nr != ec.NONE32) & ~bad)
            contigs = ext.emit(live.astype(np.uint32), nr[live].astype(np.int64) + nl[live] + t.k)
            for r, c in zip(live.tolist(), contigs):
                bad[r] |= c != w.contigs[r]
            return int(bad.sum())
        finally:
            ext.close()
    finally:
        t.close()


def main():
    from shannon_amd import device
    assert os.environ.get("SHN_DEV_POISON") == "165" and os.environ.get("SHN_DEV_POISON_WS") == "1"
    os.environ["SHN_EXT_AUDIT"] = "2"
    ctx = device.Context(0)
    wrong = dict.fromkeys(CASES, 0)
    for _round in range(2):
        for name in CASES:
            wrong[name] += wrong_ranks(ctx, name)
    ctx.close()
    print(" ".join("%s %d" % kv for kv in sorted(wrong.items())), flush=True)


if __name__ == "__main__":
    main()
