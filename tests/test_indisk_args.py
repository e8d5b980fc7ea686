"""CPU: --inDisk on the command line (shannon.parse_args: no GPU, no file system), and the host side of the file drivers
(shannon_amd/csrc/chunk_writer.h) built with a CPU formatter into a program of its own (tools/indisk_host_check.cpp)."""
import os
import shutil
import subprocess
import pytest
from conftest import ROOT


def _parse(argv, capsys):
    import shannon
    capsys.readouterr()
    o = shannon.parse_args(["shannon.py"] + argv)
    return o, capsys.readouterr().out


def test_in_disk_flag(capsys):
    o, out = _parse(["-o", "OUT", "--single", "r.fasta", "--inDisk"], capsys)
    assert o.in_disk is True
    assert "OPTIONS --inDisk: In Memory mode disabled" in out.splitlines()
    assert o.noted == [] and o.ignored == []


def test_without_the_flag(capsys):
    o, out = _parse(["-o", "OUT", "--single", "r.fasta"], capsys)
    assert o.in_disk is False and "--inDisk" not in out and o.noted == []


@pytest.mark.parametrize("ranks", [["-p", "2"], ["--gpus", "4"]])
def test_in_disk_on_several_ranks_is_noted(ranks, capsys):
    o, _out = _parse(["-o", "OUT", "--left", "a.fasta", "--right", "b.fasta", "--inDisk"] + ranks, capsys)
    assert o.in_disk is False
    notes = [n for n in o.noted if n.startswith("--inDisk")]
    assert len(notes) == 1 and "one-process runs only" in notes[0]


def test_only_reads_still_notes(capsys):
    o, _out = _parse(["-o", "OUT", "--single", "r.fasta", "--only_reads"], capsys)
    assert o.in_disk is False
    assert len(o.noted) == 1 and o.noted[0].startswith("--only_reads") and "--inDisk" not in o.noted[0]


def test_host_side_of_the_file_drivers(tmp_path):
    """writer thread, two staging buffers, chunk boundaries, open / write failures: the stand-alone program says OK"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "indisk_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tools", "indisk_host_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "indisk_host_check: OK" in p.stdout, p.stdout


def test_device_side_of_the_formatters_on_the_host(tmp_path):
    """csrc/record_expand.h as plain C++ -- the length functions, the record search, every 16-byte chunk of collect, reads*.fasta
    and k1mer.dict with arrays of exactly the allocated sizes -- against a per-record writer: the stand-alone program says OK"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "expand_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "expand_host_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "expand_host_check: OK" in p.stdout, p.stdout
