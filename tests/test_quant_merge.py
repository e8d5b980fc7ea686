"""CPU: the merge of class sets behind `python -m shannon_amd.quant` on lane files and on N ranks: the key of a list in
plain integers, the brute force of tests/merge_cases.py on a hand-checked input, the command's new arguments, the entry point's
declaration and binding, and the launch of the ranks (the ranks meet over gloo and report; nothing touches a GPU)."""
import os, re, subprocess, sys
import pytest
from conftest import ROOT
import merge_cases as mc

M64 = (1 << 64) - 1


def _mix_by_hand(h, v):
    h ^= (v + 0x9E3779B97F4A7C15) & M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    return h ^ (h >> 33)


def test_list_key_against_hand_computed_values():
    """the values below come from 64-bit unsigned machine arithmetic (numpy uint64), not from list_key"""
    from shannon_amd import abundance
    assert _mix_by_hand(0, 1) == 16572613472718614229
    assert abundance.list_key([0]) == 5111352657881770025 == _mix_by_hand(_mix_by_hand(0, 1), 0) >> 1
    assert abundance.list_key([5]) == 6770760817256958843 == _mix_by_hand(_mix_by_hand(0, 1), 5) >> 1
    assert abundance.list_key([0, 1]) == 9157739204802303814 == _mix_by_hand(_mix_by_hand(_mix_by_hand(0, 2), 0), 1) >> 1
    assert abundance.list_key([3, 70000]) == 3001038848293309186
    assert abundance.list_key((3, 70000)) == abundance.list_key([3, 70000]) < 1 << 63
    assert abundance.list_key([0, 1]) != abundance.list_key([1, 0])              # the order of the members is part of the key


def test_brute_force_on_a_hand_checked_input():
    lists = [[5], [0, 1], [5], [3, 70000], [0, 1]]
    # keys: [3, 70000] 3.00e18 < [5] 6.77e18 < [0, 1] 9.16e18 (the values of the test above)
    assert mc.brute_merge(lists, [2, 3, 4, 5, 6]) == [((3, 70000), 5), ((5,), 6), ((0, 1), 9)]
    off, mem, n_c = mc.brute_arrays(lists, [2, 3, 4, 5, 6])
    assert off.tolist() == [0, 2, 3, 5] and mem.tolist() == [3, 70000, 5, 0, 1] and n_c.tolist() == [5, 6, 9]
    assert mc.brute_merge([], []) == []
    assert mc.brute_merge([[7]], [0]) == [((7,), 0)]                             # a weight of 0 stays
    assert mc.brute_merge([[7], [7]], [3000000000, 3000000000]) == [((7,), 6000000000)]


def _files(tmp_path, *names):
    out = []
    for n in names:
        p = tmp_path / n
        p.write_text(">a\nACGT\n")
        out.append(str(p))
    return out


def test_parse_args_lanes(tmp_path):
    from shannon_amd import quant
    fa, a, b, c, d = _files(tmp_path, "t.fasta", "a.fq", "b.fq", "c.fq", "d.fq")
    base = ["quant", fa, "-o", "OUT"]
    o = quant.parse_args(base + ["--single", a + "," + b + "," + c])
    assert o["single"] == [a, b, c] and "gpus" not in o
    o = quant.parse_args(base + ["--left", a + "," + b, "--right", c + "," + d])
    assert o["left"] == [a, b] and o["right"] == [c, d]
    assert quant._lanes(None, o["left"], o["right"]) == [(a, c), (b, d)] and quant._lanes([a, b], None, None) == [(a,), (b,)]
    # a file whose own name holds a comma stays one file
    (comma,) = _files(tmp_path, "x,y.fq")
    o = quant.parse_args(base + ["--single", comma])
    assert o["single"] == comma
    # every piece must be a file
    msg = quant.parse_args(base + ["--single", a + "," + str(tmp_path / "missing.fq")])
    assert isinstance(msg, str) and "missing.fq: no such file" in msg
    # --left and --right list the same number of files
    msg = quant.parse_args(base + ["--left", a + "," + b, "--right", c])
    assert isinstance(msg, str) and "--left lists 2 files, --right 1" in msg
    msg = quant.parse_args(base + ["--left", a, "--right", c + "," + d])
    assert isinstance(msg, str) and "--left lists 1 files, --right 2" in msg


def test_parse_args_gpus(tmp_path):
    from shannon_amd import quant
    fa, a = _files(tmp_path, "t.fasta", "a.fq")
    base = ["quant", fa, "-o", "OUT", "--single", a]
    today = quant.parse_args(base)
    assert today == {"strand_specific": False, "fasta": fa, "out_dir": "OUT", "single": a}
    assert quant.parse_args(base + ["--gpus", "1"]) == today                      # one process: the dict it always was
    assert quant.parse_args(base + ["--gpus", "3"]) == dict(today, gpus=3)
    for bad, word in (("0", "at least 1"), ("-2", "at least 1"), ("two", "not an integer"), ("1.5", "not an integer")):
        msg = quant.parse_args(base + ["--gpus", bad])
        assert isinstance(msg, str) and "--gpus" in msg and word in msg, msg
    assert quant.parse_args(base + ["--gpus"]) == "--gpus needs a value"
    assert "--gpus N" in quant.USAGE and "R,R" in quant.USAGE


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "shannon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "include/shannon_hip.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


def test_the_entry_point_is_declared_and_bound_with_matching_arity():
    from shannon_amd import _lib
    args = _declaration("shn_abundance_merge")
    assert len(args) == 8 and args[-1].startswith("shn_abundance**") and args[-2].startswith("uint32_t")
    assert len(_lib.SIGNATURES["shn_abundance_merge"][1]) == 8


def test_merge_classes_refuses_parts_of_different_histograms():
    """(before the library is touched: no GPU needed)"""
    import numpy as np
    from shannon_amd import abundance
    part = lambda bins: {"class_off": np.zeros(1, np.uint64), "members": np.zeros(0, np.uint32), "n_c": np.zeros(0, np.uint64),
                         "hist": np.zeros(bins, np.uint64), "mapped": 0, "fragments": 0}
    with pytest.raises(ValueError, match="histograms"):
        abundance.merge_classes(None, [part(501), part(0)], 3)
    with pytest.raises(ValueError, match="no parts"):
        abundance.merge_classes(None, [], 3)


def test_gpus_starts_that_many_ranks_from_a_parent_that_touches_no_gpu(tmp_path):
    fa, a, b = _files(tmp_path, "t.fasta", "a.fq", "b.fq")
    env = dict(os.environ, SHN_CLI_BACKEND="gloo", SHN_CLI_LAUNCH_PROBE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "shannon_amd.quant", fa, "-o", str(tmp_path / "out"), "--left", a + "," + b, "--right", b + "," + a, "--gpus", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "launch probe: 3 ranks met, 2 paired lanes" in p.stdout
    # a usage error is refused before any rank starts
    p = subprocess.run([sys.executable, "-m", "shannon_amd.quant", fa, "-o", str(tmp_path / "out"), "--single", a, "--gpus", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 2 and "--gpus 0: at least 1" in p.stdout and "launch probe" not in p.stdout
