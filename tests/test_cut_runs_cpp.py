"""cut_runs (kmernator_amd/csrc/kmr_runs.hpp), the rule by which kmr_compare_reads* and kmr_extend_contigs* cut a batch into runs of
whole groups that fit a staging budget: tests/cpp/cut_runs_test.cpp compiled alone, with warnings as errors and under the host's
address and undefined-behaviour sanitizers, and run; it checks its own expectations."""
import os
import subprocess

from helpers import ROOT


def test_cut_runs_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "cut_runs_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe,      # the runtimes inside the program: nothing depends on the loader's order
                           os.path.join(ROOT, "tests", "cpp", "cut_runs_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and p.stdout.count(" ok") == 18, p.stdout + p.stderr
