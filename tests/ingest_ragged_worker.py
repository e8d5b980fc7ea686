"""Worker of tests/test_ingest_ranks_ragged.py (gloo, no GPU): every rank ingests its share of the read files by bytes with
ragged=True (shannon_amd.distributed.ingest_rank_slice) and writes what it holds -- codes + offsets for device.RaggedCodes, the
matrix otherwise -- and what it looked at."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist
from shannon_amd import device, distributed


def main():
    out, paths = sys.argv[1], sys.argv[2:]
    dist.init_process_group("gloo")
    rank, W = dist.get_rank(), dist.get_world_size()
    stats = {}
    sl = distributed.ingest_rank_slice(paths, rank, W, None, torch.device("cpu"), stats=stats, ragged=True)
    if sl is None:
        json.dump({"declined": True}, open("%s.rank%d.json" % (out, rank), "w"))
    else:
        stores, n = sl
        arrays = {}
        kinds = []
        for i, m in enumerate(stores):
            if isinstance(m, device.RaggedCodes):
                kinds.append("ragged")
                arrays["codes%d" % i], arrays["off%d" % i] = m.codes, m.off
            else:
                kinds.append("matrix")
                arrays["m%d" % i] = m
        np.savez("%s.rank%d.npz" % (out, rank), **arrays)
        stats.update({"n": n, "kinds": kinds})
        json.dump(stats, open("%s.rank%d.json" % (out, rank), "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
