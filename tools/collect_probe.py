#!/usr/bin/env python3
"""What collecting a partition's reads costs on the N-rank path: the host gather (kmers_for_component.ReadStore.gather_codes over the
host copies of the reads) against the device collect (device.Reads.collect = shn_reads_collect over the resident packed sets), on
one GPU.

    python tools/collect_probe.py [--reads 10000000] [--repeats 5] [--out results.json]

Two synthetic sets of --reads reads: ragged (30 .. 150 bases, about 1 % of the reads with an N) and of one length (L = 100, the
same share of N), each with a sorted selection of half of its reads.  Per set and path: one warm-up call, then the median and the
spread (min .. max) of --repeats calls -- wall time, bytes of codes per second.  For the device path also the expansion kernel's
HIP-event time (timer reads.collect) beside the bytes its launch site declares (0.25 B read per base, + 0.125 with a mask, + 4 B
of selection per read, + 1 B written per base), and the download of the same number of bytes timed alone: what share of the
device figure is the copy to the host.  The two paths' outputs are compared.  One JSON object on the last line."""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def probe(ctx, name, host, dev, store, repeats, seed):
    import numpy as np
    import torch
    from shannon_amd import device
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(dev)
    sel = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
    zeros = np.zeros(len(sel), np.uint8)

    def on_host():
        buf, off, _rc, _enc = store.gather_codes(sel, 1)
        return buf, off

    def on_device():
        return device.Reads.collect(dev, None, sel, zeros)
    (hb, ho), (db, do) = on_host(), on_device()                              # warm-up, and the comparison
    total = int(do[-1])
    assert np.array_equal(np.asarray(ho, dtype=np.uint64), do) and np.array_equal(hb[:total], db), "the two paths differ"
    if not store.ragged:
        store.release(hb)
    wall = {"host": [], "device": []}
    kern = []
    for _ in range(repeats):
        for path, fn in (("host", on_host), ("device", on_device)):
            ctx.timer_reset()
            t0 = time.perf_counter()
            out = fn()
            wall[path].append(time.perf_counter() - t0)
            if path == "device":
                kern.append(ctx.timers()["reads.collect"][0] / 1e3)
                model = ctx.timer_bytes()["reads.collect"]
            elif not store.ragged:
                store.release(out[0])
    # the download alone: as many bytes from device memory into a pageable host buffer
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8)
    down = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        if i:
            down.append(time.perf_counter() - t0)
    res = {"reads": n, "selected": len(sel), "bases": total, "host_s": spread(wall["host"]), "device_s": spread(wall["device"]),
           "kernel_s": spread(kern), "download_alone_s": spread(down), "kernel_model_bytes": int(model)}
    med = lambda k: res[k]["median"]
    res["host_GBps"] = round(total / med("host_s") / 1e9, 3)
    res["device_GBps"] = round(total / med("device_s") / 1e9, 3)
    res["kernel_model_GBps"] = round(model / med("kernel_s") / 1e9, 1)
    res["download_share_of_device"] = round(med("download_alone_s") / med("device_s"), 3)
    res["device_over_host"] = round(med("host_s") / med("device_s"), 2)
    print("%-8s %d reads, %d selected, %d bases: host %.4f s (%.2f GB/s)  device %.4f s (%.2f GB/s; kernel %.5f s = %.0f GB/s of its model's %d bytes; "
          "a download of the bytes alone %.4f s = %.0f %% of the device figure)  host / device = %.2f"
          % (name, n, len(sel), total, med("host_s"), res["host_GBps"], med("device_s"), res["device_GBps"], med("kernel_s"), res["kernel_model_GBps"], model,
             med("download_alone_s"), 100 * res["download_share_of_device"], res["device_over_host"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from shannon_amd import device, kmers_for_component as kfc
    ctx = device.Context(0)
    rng = np.random.Generator(np.random.PCG64(1))
    n = a.reads
    out = {}
    # ---- ragged: 30 .. 150 bases, an N in about 1 % of the reads
    lens = rng.integers(30, 151, n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    codes = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    bad = np.nonzero(rng.random(n) < 0.01)[0]
    codes[(off[bad] + (rng.integers(0, 1 << 30, len(bad)) % lens[bad]).astype(np.uint64)).astype(np.int64)] = 4
    host = device.RaggedCodes(codes, off)
    dev = device.Reads.from_ragged(ctx, codes, off)
    out["ragged"] = probe(ctx, "ragged", host, dev, kfc.ReadStore(host), a.repeats, 2)
    dev.close()
    del host, codes, off
    # ---- one length
    L = 100
    rows = rng.integers(0, 4, (n, L), dtype=np.uint8)
    bad = np.nonzero(rng.random(n) < 0.01)[0]
    rows[bad, rng.integers(0, L, len(bad))] = 4
    dev = device.Reads.from_codes(ctx, rows)
    out["L100"] = probe(ctx, "L100", rows, dev, kfc.ReadStore(rows), a.repeats, 3)
    dev.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
