"""sel_label, sel_measure and sel_emit / sel_put_record (kmernator_amd/csrc/kmr_select.hpp: what a record of the selection's output is)
as host functions: tests/cpp/select_record_test.cpp compiled alone against a stub of the few HIP names the header uses
(tests/cpp/hipstub), under the host's address and undefined-behaviour sanitizers, and run; it checks its own expectations: every
label and record against snprintf, the measured length against the written one, each record into a heap block of exactly its bytes
and between guard bytes, no label longer than SEL_LABEL_MOST.  The partition and the walk over picks need a device:
tests/test_gpu_select_edges.py."""
import os
import subprocess

from helpers import ROOT


def test_select_record_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "select_record_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing depends on the loader's order
                           "-I" + os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I" + os.path.join(ROOT, "kmernator_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "select_record_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and p.stdout.count(" ok\n") == 14, p.stdout + p.stderr
    assert p.stdout.splitlines()[-1].endswith(" checks, 0 wrong") and int(p.stdout.splitlines()[-1].split()[0]) > 10000
