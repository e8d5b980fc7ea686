"""Worker for tests/test_filter_fp_ranks.py: distributed.filter_owned_texts and the gather behind it over gloo, without a GPU.  The
two compute callables are numpy: every rank "covers" a seeded pseudo-random subset of the bits, the count is the numpy mirror
(filter_fp.hits_from_bitmaps(None, ...)).  The test process imports make_case / rank_bitmap to compute what one process gives."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

OWNERS = {"split2": [0, 1, 0, 0, 1, 1, 0],        # two ranks, runs that are not contiguous
          "idle3": [0, 2, 0, 0, 2, 2, 0],         # three ranks, rank 1 owns nothing
          "idle0": [1, 1, 1, 1, 1, 1, 1]}         # rank 0 (which merges) owns nothing
N_TRANSCRIPTS = [3, 0, 2, 5, 1, 0, 4]             # partitions 1 and 5 hold no transcript
LENGTHS = [1, 14, 15, 63, 64, 65, 130, 200, 257, 300, 90, 128, 31, 77, 640]


def make_case():
    """(names, texts): 7 partitions of random transcripts whose lengths put boundaries inside words; some shorter than a seed"""
    rng = np.random.Generator(np.random.PCG64(5))
    names, texts, k = [], [], 0
    for i, n in enumerate(N_TRANSCRIPTS):
        names.append("c%d" % i)
        t = ""
        for j in range(n):
            t += ">s_c%d_%d len extra\n%s\n" % (i, j, "".join("ACGT"[c] for c in rng.integers(0, 4, LENGTHS[k % len(LENGTHS)])))
            k += 1
        texts.append(t)
    return names, texts


def rank_bitmap(rank, n_words):
    """what rank `rank` covers: bits drawn with a density that is low or high for four words at a time (the same density on every
    rank, so that the union covers some transcripts to 90 % and others not)"""
    dens = np.repeat(np.random.Generator(np.random.PCG64(77)).choice([0.3, 0.97], (n_words + 3) // 4), 4)[:n_words]
    bits = np.random.Generator(np.random.PCG64(100 + rank)).random((n_words, 64)) < dens[:, None]
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n_words)


class _Res(object):
    single_contigs, contigs = [], []


def main():
    import torch.distributed as dist
    from shannon_amd import distributed, filter_fp as ffp
    case, out, boom = sys.argv[1], sys.argv[2], int(sys.argv[3])
    dist.init_process_group("gloo")
    rank, W = dist.get_rank(), dist.get_world_size()
    names, texts = make_case()
    owner = np.asarray(OWNERS[case])
    mine = {i: texts[i] for i in range(len(names)) if owner[i] == rank}

    def cover(seqs, part_of, n_parts):
        if rank == boom:
            raise RuntimeError("boom on purpose")
        assert n_parts == len(names) and len(part_of) == len(seqs)
        return rank_bitmap(rank, (int(ffp.text_offsets(seqs)[-1]) + 63) // 64), {"routes": 10 * (rank + 1), "placed": rank + 1}

    T = {}
    clock = distributed.Clock(T)
    kept, org, logs, stats, err = distributed.filter_owned_texts(mine, names, owner, cover, lambda c, t, w: ffp.hits_from_bitmaps(None, c, t, w),
                                                                 clock=clock)
    msg, res = "", None
    try:
        res = distributed._gather_and_merge(kept, names, _Res(), None, None, clock, error=err, extra={"org": org, "logs": logs, "stats": stats})
    except RuntimeError as ex:
        msg = str(ex)
    json.dump({"kept": {str(i): t for i, t in kept.items()}, "logs": {str(i): t for i, t in logs.items()}, "stats": stats, "error": msg,
               "timings": sorted(T),
               "result": None if res is None else {"partitions": dict(res["partitions"]), "partitions_org": dict(res["partitions_org"]),
                                                   "filter_logs": dict(res["filter_logs"]), "filter_fp_stats": res["filter_fp_stats"],
                                                   "final": sorted(dict(res["final"]).values())}},
              open("%s.rank%d" % (out, rank), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
