"""GPU: `shannon.py ... --inDisk` writes TEMP/<sample>_<comp>algo_input/reads*.fasta and k1mer.dict for every partition -- the
values the reference's own run left in the fixtures (reads_digest, read_names, k1mers_digest), byte for byte the files
reference_api.kmers_for_component writes for the same inputs, usable by multibridging.main, and without a change to shannon.fasta."""
import os
import pytest
from golden_util import *

pytestmark = pytest.mark.gpu

CASES = ["syn_pe_s0", "syn_se_s7_K20", "syn_pe_ss_s69", "syn_se_ss_s53"]


def _run_cli(argv, capsys):
    """shannon.main in this process (one device context per run, closed at its end); returns what it printed"""
    import shannon
    capsys.readouterr()
    rc = shannon.main(["shannon.py"] + argv)
    out = capsys.readouterr().out
    assert rc == 0, out
    return out


def _reference_files(name, work):
    """the files of reference_api.kmers_for_component for the case, chained through files as shannon.py chains them
    (tests/test_reference_api_gpu.py): {comp: ([read files], k1-mer file)}"""
    from shannon_amd import reference_api as api
    from oracle import count
    g, K, paired = load_case(name), meta(name)["K"], meta(name)["paired"]
    ai = os.path.join(work, "s_algo_input")
    os.makedirs(ai)
    dbl = read_files(name, load_inputs(name))
    rf = []
    for i, reads in enumerate(dbl):
        p = os.path.join(work, "reads_%d.fasta" % (i + 1))
        open(p, "w").write("".join(">%d\n%s\n" % (e, s) for e, s in enumerate(reads)))
        rf.append(p)
    tab = count.count_k1mers_dict([r for f in dbl for r in f], K + 1)
    open(os.path.join(ai, "k1mer.dict_org"), "w").write("".join("%s\t%d\n" % (k, tab[k]) for k in sorted(tab, reverse=True)))
    args = [os.path.join(ai, "k1mer.dict_org"), os.path.join(ai, "k1mer.dict"), "3", "75", work, "500", "1"] + rf
    allowed, reads = api.extension_correction(args, True)
    api.kmers_for_component(allowed, ai, reads, rf, work, "contigs.txt", True, False, paired, True, 500, 2, K, "true", 5, False, False, 1)
    out = {}
    for comp in g["partitions"]:
        files = [os.path.join(work, "reads%s_%s.fasta" % (comp, x)) for x in ("1", "2")] if paired else [os.path.join(work, "reads%s.fasta" % comp)]
        out[comp] = (files, os.path.join(work, "component%sk1mers_allowed.dict" % comp))
    return out


@pytest.mark.parametrize("name", CASES)
def test_cli_in_disk_writes_the_partition_files(name, tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("SHN_MALLOC_TUNE", "0")                 # (the CLI's allocator settings are for a process of its own)
    g, m = load_case(name), meta(name)
    K, paired = m["K"], m["paired"]
    inp = load_inputs(name)
    files = []
    for i, reads in enumerate(inp):
        p = str(tmp_path / ("in_%d.fasta" % (i + 1)))
        open(p, "w").write("".join(">%d\n%s\n" % (e, s) for e, s in enumerate(reads)))
        files.append(p)
    argv = (["--left", files[0], "--right", files[1]] if paired else ["--single", files[0]]) + ["-K", str(K)] + (["-s"] if strand_specific(name) else [])
    # (the sample name, which the transcripts' headers carry, is the output directory's base name: the same for both runs)
    out_a, out_b = str(tmp_path / "with" / "run"), str(tmp_path / "without" / "run")
    os.makedirs(str(tmp_path / "with")), os.makedirs(str(tmp_path / "without"))
    log = _run_cli(["-o", out_a] + argv + ["--inDisk"], capsys)
    assert "OPTIONS --inDisk: In Memory mode disabled" in log
    assert not [l for l in log.splitlines() + open(os.path.join(out_a, "log.txt")).read().splitlines() if "NOTE" in l and "--inDisk" in l]
    ref = _reference_files(name, str(tmp_path / "ref"))
    assert list(ref) == list(g["partitions"])
    for comp, gp in g["partitions"].items():
        d = os.path.join(out_a, "TEMP", "run_%salgo_input" % comp)
        mine = [os.path.join(d, x) for x in (("reads_1.fasta", "reads_2.fasta") if paired else ("reads.fasta",))]
        got_reads = [[l.strip() for l in open(f) if l[0] != ">"] for f in mine]
        assert digest(got_reads) == gp["reads_digest"]
        assert [l.strip() for l in open(mine[0]) if l[0] == ">"][:3] == gp["read_names"]
        kf = os.path.join(d, "k1mer.dict")
        assert digest([l.split() for l in open(kf)]) == gp["k1mers_digest"]
        # byte for byte the files of the reference's file interface
        for f_mine, f_ref in zip(mine + [kf], ref[comp][0] + [ref[comp][1]]):
            assert open(f_mine, "rb").read() == open(f_ref, "rb").read(), (f_mine, f_ref)
        if name == "syn_pe_s0":
            # ... and usable as the reference uses them: multibridging.main on the written files gives the fixture's graph
            from shannon_amd import reference_api as api
            from test_reference_api_gpu import _canonical_from_files
            pdir = str(tmp_path / ("p_" + comp)) + "/"
            api.multibridging_main("-f --kmer=%d -e --only_k1 %s %s %s %sintermediate" % (K, kf, kf, " ".join(mine), pdir))
            can, _n = _canonical_from_files(pdir + "intermediate")
            for k in can:
                assert approx_eq(can[k], gp["graph"][k])
    # the same command without --inDisk: the same transcripts, no such files
    _run_cli(["-o", out_b] + argv, capsys)
    assert open(os.path.join(out_a, "shannon.fasta"), "rb").read() == open(os.path.join(out_b, "shannon.fasta"), "rb").read()
    assert not [d for d in os.listdir(os.path.join(out_b, "TEMP")) if d.endswith("algo_input") and d != "run_algo_input"]
