"""dump_line and dump_size_kernel (kmernator_amd/csrc/kmr_dump.hpp: the line generator of the mercount / mergraph writer and its
size pass) as host functions: tests/cpp/dump_line_test.cpp compiled alone against a stub of the few HIP names the header uses
(tests/cpp/hipstub), under the host's address and undefined-behaviour sanitizers, and run; it checks its own expectations: every
line of both texts against snprintf at every byte offset across a tile's start and end, for k = 1 .. 20 and around every word
border up to 128.  The walk over tiles needs a workgroup: tests/test_gpu_dump_edges.py."""
import os
import subprocess

from helpers import ROOT


def test_dump_line_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "dump_line_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing depends on the loader's order
                           "-I" + os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I" + os.path.join(ROOT, "kmernator_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dump_line_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and p.stdout.count(" ok\n") == 31, p.stdout + p.stderr
    assert p.stdout.splitlines()[-1].endswith(" placements, 0 wrong") and int(p.stdout.splitlines()[-1].split()[0]) > 250000
