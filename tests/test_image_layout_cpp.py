"""check_image_layout (kmernator_amd/csrc/kmr_image_layout.hpp), the host-side check kmr_load_image and kmr_merge_image make of a
stored map before any kernel follows one of its offsets: tests/cpp/image_layout_test.cpp compiled alone, with warnings as errors and
under the host's address and undefined-behaviour sanitizers, and run; it checks its own expectations.  Among them the two headers
whose size sum wraps (nb = 2^62, 2^63), refused from a 16-byte allocation, and every image read from an odd address."""
import os
import subprocess

from helpers import ROOT


def test_image_layout_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "image_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe,      # the runtimes inside the program: nothing depends on the loader's order
                           os.path.join(ROOT, "tests", "cpp", "image_layout_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and p.stdout.count(" ok\n") == 105, p.stdout + p.stderr
    for nb in ("2^62", "2^63"):
        assert p.stdout.count("nb %s, 16 bytes" % nb) == 4
