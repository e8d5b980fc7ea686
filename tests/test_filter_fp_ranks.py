"""CPU: --filter_FP on N ranks.  The two halves of shn_filter_fp_hits are declared and bound; the numpy mirror of the owner's count
(filter_fp.hits_from_bitmaps(None, ...)) on hand-written bitmaps; distributed.filter_owned_texts over gloo with numpy compute
against what one process computes from the OR of all ranks' bitmaps; a failing rank is told to every rank; the command line."""
import inspect, json, os, re, subprocess, sys
import numpy as np
import pytest
from conftest import ROOT
import dist_filter_fp_cpu_worker as worker


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "shannon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "include/shannon_hip.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("shn_filter_fp_cover", 16), ("shn_filter_fp_count", 8)])
def test_both_halves_are_declared_and_bound_with_matching_arity(name, n_args):
    from shannon_amd import _lib
    args = _declaration(name)
    assert len(args) == n_args
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args)
    assert len(_declaration("shn_filter_fp_hits")) == len(_lib.SIGNATURES["shn_filter_fp_hits"][1]) == 16       # (kept as it was)


def _bitmap(n_words, ranges):
    bits = np.zeros(n_words * 64, dtype=bool)
    for a, b in ranges:
        bits[a:b] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)


def test_mirror_counts_transcripts_whose_boundaries_fall_inside_words():
    from shannon_amd import filter_fp
    lens = [1, 15, 63, 64, 65, 130]
    t_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)                  # 0 1 16 79 143 208 338
    nw = (int(t_off[-1]) + 63) // 64
    full = _bitmap(nw, [(0, 338)])
    assert filter_fp.hits_from_bitmaps(None, full[None, :], t_off).tolist() == lens
    # base 0 alone; the last 5 of the 15; bases 70..150 across three transcripts and two words; the last base of the text
    part = _bitmap(nw, [(0, 1), (11, 16), (70, 150), (337, 338)])
    assert filter_fp.hits_from_bitmaps(None, part[None, :], t_off).tolist() == [1, 5, 9, 64, 7, 1]
    assert filter_fp.hits_from_bitmaps(None, np.zeros((1, nw), np.uint64), t_off).tolist() == [0] * 6


def test_mirror_ignores_neighbours_bits_in_a_window():
    from shannon_amd import filter_fp
    # the text's words 2..5 = bases 128..383; transcripts [150, 200) [200, 200) [200, 370): bases 128..149 and 370..383 are neighbours'
    t_off = np.array([150, 200, 200, 370], dtype=np.uint64)
    whole = _bitmap(8, [(100, 160), (199, 201), (360, 400)])
    win = whole[2:6]
    assert int(win[0] & np.uint64((1 << 22) - 1)) != 0 and int(win[3] >> np.uint64(370 - 320)) != 0      # set bits of neighbours in both boundary words
    assert filter_fp.hits_from_bitmaps(None, win[None, :], t_off, word0=2).tolist() == [11, 0, 11]
    assert filter_fp.hits_from_bitmaps(None, whole[None, :], t_off).tolist() == [11, 0, 11]


def test_mirror_is_an_or_not_a_sum_and_refuses_what_the_device_refuses():
    from shannon_amd import filter_fp
    t_off = np.array([0, 70, 70, 100], dtype=np.uint64)
    a, b = _bitmap(2, [(0, 40), (80, 90)]), _bitmap(2, [(30, 75)])
    one = filter_fp.hits_from_bitmaps(None, a[None, :], t_off).tolist()
    assert one == [40, 0, 10]                                                                           # (an empty transcript gives 0)
    assert filter_fp.hits_from_bitmaps(None, np.stack([a, a]), t_off).tolist() == one
    assert filter_fp.hits_from_bitmaps(None, np.stack([a, b, a]), t_off).tolist() == [70, 0, 15]
    with pytest.raises(ValueError):
        filter_fp.hits_from_bitmaps(None, np.zeros((0, 2), np.uint64), t_off)
    with pytest.raises(ValueError):
        filter_fp.hits_from_bitmaps(None, a[None, :1], t_off)                                           # a transcript behind the window
    with pytest.raises(ValueError):
        filter_fp.hits_from_bitmaps(None, a[None, :], t_off, word0=1)                                   # ... and before it
    with pytest.raises(ValueError):
        filter_fp.hits_from_bitmaps(None, a, t_off)                                                     # not 2-D


def _run(case, world, port, boom, tmp_path):
    out = str(tmp_path / "res")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_filter_fp_cpu_worker.py"), case, out, str(boom)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    return [json.load(open("%s.rank%d" % (out, r))) for r in range(world)]


@pytest.mark.parametrize("case,world,port", [("split2", 2, 29661), ("idle3", 3, 29662), ("idle0", 2, 29663)])
def test_owners_hits_equal_one_process_on_the_or_of_all_bitmaps(case, world, port, tmp_path):
    from shannon_amd import filter_fp
    got = _run(case, world, port, -1, tmp_path)
    names, texts = worker.make_case()
    owner = worker.OWNERS[case]
    assert any(r not in owner for r in range(world)) or case == "split2"                  # a rank that owns no partition
    assert "" in texts                                                                    # a partition without transcripts
    # one process: the layout, the OR of all ranks' bitmaps, the count over the whole text, the decision per partition
    parsed = [filter_fp.records(t) for t in texts]
    seqs = [s for _nm, sq in parsed for s in sq]
    t_off = filter_fp.text_offsets(seqs)
    nw = (int(t_off[-1]) + 63) // 64
    assert any(int(v) % 64 for v in t_off[1:-1]) and any(len(s) < filter_fp.SEED for s in seqs)
    covers = np.stack([worker.rank_bitmap(r, nw) for r in range(world)])
    hits = filter_fp.hits_from_bitmaps(None, covers, t_off)
    assert hits.tolist() != filter_fp.hits_from_bitmaps(None, covers[:1], t_off).tolist()           # (one rank's bitmap is not enough)
    want, at = [], 0
    for nm, sq in parsed:
        want.append(filter_fp._filter_records(nm, sq, hits[at:at + len(sq)].tolist()))
        at += len(sq)
    n_kept = sum(k.count(">") for k, _l in want)
    assert 0 < n_kept < len(seqs)                                                         # some dropped, some kept
    for r, g in enumerate(got):
        assert g["error"] == ""
        assert sorted(int(i) for i in g["kept"]) == [i for i, o in enumerate(owner) if o == r]
        for i in g["kept"]:
            assert (g["kept"][i], g["logs"][i]) == want[int(i)], (r, i)
        assert g["stats"] == {"routes": sum(10 * (q + 1) for q in range(world)), "placed": sum(q + 1 for q in range(world)),
                              "transcripts": len(seqs), "kept": n_kept}
        assert {"filter_FP", "x:filter_FP texts", "x:filter_FP coverage"} <= set(g["timings"])
    res = got[0]["result"]
    assert all(g["result"] is None for g in got[1:])
    assert list(res["partitions"]) == names
    assert [res["partitions"][n] for n in names] == [k for k, _l in want]
    assert [res["filter_logs"][n] for n in names] == [l for _k, l in want]
    assert [res["partitions_org"][n] for n in names] == texts
    assert res["filter_fp_stats"] == got[0]["stats"]
    assert 0 < len(res["final"]) <= n_kept                                                # the merge saw the kept texts only
    kept_seqs = {s for k, _l in want for s in filter_fp.records(k)[1]}
    assert set(res["final"]) <= kept_seqs


def test_a_failing_cover_is_told_to_every_rank(tmp_path):
    """rank 1's cover raises: it still takes part in every collective of the step (with zeros), its message travels with the FASTA
    gather, all ranks raise together and none hangs"""
    got = _run("idle3", 3, 29664, 1, tmp_path)
    for g in got:
        assert "graph stage failed on rank 1" in g["error"] and "boom on purpose" in g["error"] and "rank 0" not in g["error"], g["error"]
        assert g["result"] is None


def test_ops_without_the_filter_are_refused_before_any_collective():
    from shannon_amd import distributed

    class Ops(object):
        paired = True
    with pytest.raises(ValueError, match="filter_cover"):
        distributed.assemble_distributed(Ops(), filter_fp=True)                          # (no process group exists: a collective would fail otherwise)


def test_single_end_ranks_are_not_filtered_and_say_so():
    """run_MB_SF_fn.py:110: the flag is set for paired-end runs only -- no collective, the texts as they were, a note for rank 0"""
    from shannon_amd import distributed

    class Ops(object):
        paired = False
    texts = {0: ">a\nACGT\n"}
    got, extra, err = distributed._filter_step(Ops(), {}, texts, ["c0"], [0], None, None, None)
    assert got is texts and err is None and list(extra) == ["note"] and "single-end" in extra["note"]


def test_cli_keeps_the_flag_on_the_n_rank_path(capsys):
    import shannon
    o = shannon.parse_args(["shannon.py", "-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "-p", "2", "--filter_FP"])
    capsys.readouterr()
    assert o.filter_fp is True and not any("filter_FP" in n for n in o.noted)
    src = inspect.getsource(shannon.rank_main)
    assert "not applied on the N-rank path" not in src and "filter_fp=filter_fp" in src
    o = shannon.parse_args(["shannon.py", "-o", "OUT", "--single", "a.fasta", "-p", "2", "--filter_FP"])
    capsys.readouterr()
    assert o.filter_fp is False and any("--filter_FP: single-end input" in n for n in o.noted)
