"""dedup_key_kernel (kmernator_amd/csrc/kmr_dedup.hpp: the duplicate-fragment key built by shifts over four words, its reverse
complement, the canonical choice of mode 2, the skip tests and their counters) as a host function: tests/cpp/dedup_key_test.cpp
compiled alone against a stub of the few HIP names the header uses (tests/cpp/hipstub), under the host's address and
undefined-behaviour sanitizers, and run; it checks its own expectations: every record's key, candidate flag and flip flag against a
key built base by base from strings and compared with memcmp, for all sixteen dedup_length values x four start offsets x both
modes x both passes, with ties up to a word border and palindromic keys.  The consensus kernel needs a wavefront:
tests/test_gpu_dedup_edges.py."""
import os
import subprocess

from helpers import ROOT


def test_dedup_key_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "dedup_key_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing depends on the loader's order
                           "-I" + os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I" + os.path.join(ROOT, "kmernator_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dedup_key_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and p.stdout.count(" ok\n") == 16, p.stdout + p.stderr
    assert p.stdout.splitlines()[-1].endswith(" records, 0 wrong") and int(p.stdout.splitlines()[-1].split()[0]) > 20000
