"""kmernator::ContigExtender of include/kmernator_amd.hpp from a C++ host (tests/cpp/extend_demo.cpp): it compiles without a warning
and names contigs as the restatement does; on the device it extends the contigs of tests/extendcases.py as the restatement does."""
import os
import struct
import subprocess

import pytest

import extendcases as ec
import refextend as rx
from helpers import default_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp_path):
    exe = str(tmp_path / "extend_demo")
    lib_dir = os.path.join(ROOT, "kmernator_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "extend_demo.cpp"), "-L" + lib_dir, "-lkmernator_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_extend_demo_names(tmp_path):
    exe = build_demo(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run([exe, "names"], capture_output=True)
    assert p.returncode == 0, p.stderr
    names = [b"c1", b"c1-l3r4", b"cell-1", b"ctgl", b"x-l2", b"a-l1r2-l3r4"]
    want = [b"%s %s %s" % (n, rx.new_name(n, 0, 0), rx.new_name(n, 2, 5)) for n in names] + [b"%d %d %d" % rx.min_max_kmer_size(31, 150, 15000, 100)]
    assert p.stdout.splitlines() == want


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 97])
def test_cpp_extend_demo_extends(tmp_path, k):
    c = ec.several(k)[0]
    (tmp_path / "c.fa").write_bytes(b"".join(b">%s\n%s\n" % (n, s) for n, s in zip(c["names"], c["contigs"])))
    (tmp_path / "r.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])))
    (tmp_path / "p.txt").write_text("".join(" ".join(str(j) for j in p) + "\n" for p in c["pools"]))
    p = subprocess.run([build_demo(tmp_path), "extend", str(k), str(tmp_path / "c.fa"), str(tmp_path / "r.fastq"), str(tmp_path / "p.txt"), str(c["options"]["max_extend"])],
                       capture_output=True)
    assert p.returncode == 0, p.stderr
    w = rx.Extender(default_config(k), **c["options"]).extend(c["contigs"], [ec.pool_of(c, i) for i in range(len(c["contigs"]))])
    lines = p.stdout.splitlines()
    for i, (seq, l, r, stops) in enumerate(w):
        vals = b" ".join(b"%016x" % struct.unpack("<Q", rx.bits(v))[0] for st in stops for v in st[1])
        assert lines[i] == b"%s %d %d %d %d %s %s" % (rx.new_name(c["names"][i], l, r), l, r, stops[0][0], stops[1][0], vals, seq)
    assert lines[len(w)] == b"extended %d bases %d batch %d" % (sum(1 for x in w if x[1] + x[2]), sum(x[1] + x[2] for x in w), len(w))
