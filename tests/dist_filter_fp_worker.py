"""Worker for tests/test_distributed_filter_fp_gpu.py: assemble_distributed(filter_fp=True) with world_size > 1 and every rank on
cuda:0 (the product's GpuOps; collectives over gloo through host memory, as tests/dist_gpu_worker.py)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist


def main():
    n_genes, seed, n_pairs, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    ss = len(sys.argv) > 5 and sys.argv[5] == "ss"             # -s / --strand_specific
    from shannon_amd import device, synth, distributed, kmers_for_component as kfc
    dist.init_process_group("gloo")
    rank, W = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    (q1, q2), _ = synth.make_dataset(n_pairs, n_genes, seed=seed)
    n = len(q1)
    lo, hi = rank * n // W, (rank + 1) * n // W
    q1, q2 = q1[lo:hi], q2[lo:hi]
    ctx = device.Context(0)
    d1, d2 = device.Reads.from_codes(ctx, q1), device.Reads.from_codes(ctx, q2)
    ops = distributed.GpuOps(ctx, d1, d2, kfc.ReadStore(q1, q2), 25)
    T = {}
    res = distributed.assemble_distributed(ops, 25, 500, "t", 1, double_stranded=not ss, timings=T, filter_fp=True)
    local = [None] * W
    dist.all_gather_object(local, getattr(ops, "filter_fp_local", None))
    if rank == 0:
        json.dump({"partitions": dict(res["partitions"]), "partitions_org": dict(res["partitions_org"]), "filter_logs": dict(res["filter_logs"]),
                   "filter_fp_stats": res["filter_fp_stats"], "final": res["final"], "timings": T, "local": local}, open(out, "w"))
    dist.barrier()
    d1.close()
    d2.close()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
