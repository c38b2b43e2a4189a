"""selectReads' partitioned branch without a device: the restatement of tests/refpartition.py on the cases the reference's loop
(apps/FilterReads.h:211-272) decides, the library's own table of rounds against it (kmr_partition_rounds), the ABI of the
kmr_partition_* entry points, and the C++ host side."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmernator_amd as ka
from kmernator_amd import _lib
from helpers import ROOT
from refpartition import file_name, output_name, partition, round_table

NEW_SYMBOLS = ["kmr_partition_config_init", "kmr_partition_rounds", "kmr_partition_reads", "kmr_partition_reads_dev", "kmr_partition_read_batch",
               "kmr_partition_read_batch_dev", "kmr_picks_segments_info", "kmr_picks_segments_copy"]
ENTRIES = ["kmr_partition_reads", "kmr_partition_reads_dev", "kmr_partition_read_batch", "kmr_partition_read_batch_dev"]


def depths(rounds):
    return [r["depth"] for r in rounds]


# ---------------------------------------------------------------- the restatement

def test_round_sequences():
    assert depths(round_table(2, 16)) == [16, 8, 4, 2]
    r = round_table(3, 20, remainder_trim=25.0)           # 20 10 5, then 2 < 3: depth == minDepth never holds, so no remainder
    assert depths(r) == [20, 10, 5] and not any(x["is_remainder"] for x in r)
    assert depths(round_table(2, 2)) == [2]
    assert round_table(2, 1, remainder_trim=25.0) == []
    for pbd in (0, -1):                                   # off (the reference's default is -1): one round at min depth, never a remainder
        r = round_table(2, pbd, remainder_trim=25.0, min_passing_in_pair=2)
        assert depths(r) == [2] and not r[0]["is_remainder"] and r[0]["both_pass"]
    r = round_table(1, 2 ** 31)
    assert len(r) == 32 and depths(r) == [float(2 ** b) for b in range(31, -1, -1)]


def test_remainder_condition():
    r = round_table(2, 16, remainder_trim=25.0)           # the default 0.40: (int) 0.40 = 0 != 25
    assert depths(r) == [16, 8, 4, 2, 2] and [x["is_remainder"] for x in r] == [False] * 4 + [True]
    assert r[4]["min_read_length"] == 25.0 and not r[4]["both_pass"] and r[3]["min_read_length"] == float(np.float32(0.40))
    # min-passing-in-pair 1 and (int) min-read-length == remainder-trim: nothing would change, the round is not run
    assert depths(round_table(2, 16, remainder_trim=25.0, min_read_length=25.0)) == [16, 8, 4, 2]
    assert depths(round_table(2, 16, remainder_trim=25.0, min_read_length=25.7)) == [16, 8, 4, 2]
    # with min-passing-in-pair 2 it runs even then, and lets single reads of a pair through
    r = round_table(2, 16, remainder_trim=25.0, min_read_length=25.0, min_passing_in_pair=2)
    assert len(r) == 5 and [x["both_pass"] for x in r] == [True] * 4 + [False]
    assert depths(round_table(2, 16, remainder_trim=0.0)) == [16, 8, 4, 2] and depths(round_table(2, 16, remainder_trim=-1.0)) == [16, 8, 4, 2]


def test_file_names():
    r = round_table(2, 16, remainder_trim=25.0)
    assert file_name("out", 2, r[0], True, "lib1") == "out-MinDepth2-PartitionDepth16-lib1.fastq"
    assert file_name("out", 2, r[3], True, "lib1", fasta=True) == "out-MinDepth2-PartitionDepth2-lib1.fasta"
    assert file_name("out", 2, r[4], True, "lib1") == "out-MinDepth2-Remainder-lib1.fastq"
    assert file_name("out", 2, round_table(2, 0)[0], False, "lib1") == "out-MinDepth2-lib1.fastq"
    assert file_name("out", 2, r[0], True, "lib1", separate_outputs=False) == "out" and output_name("out", 2, r[4], True, False) == "out"


def test_availability_order_and_pairs():
    """eight reads by hand: a read lands in the first round that picks it, its mate with it; the remainder round lets the single
    passing read of a pair and a shorter trim through; the output is round-major, ascending index inside a round, split by input"""
    names = [b"r%d" % i for i in range(8)]
    seqs = [b"A" * 50] * 8
    quals = [b"I" * 50] * 8
    sc = [16, 1, 4, 4, 2, 16, 8, 2]
    tl = [50, 50, 50, 50, 22, 50, 50, 50]
    mate = [1, 0, 3, 2, -1, -1, 7, 6]
    labels = [b"L%d" % i for i in range(8)]
    zero = [0] * 8
    rounds = round_table(2, 16, remainder_trim=20.0, min_read_length=25.0, min_passing_in_pair=2)
    text, table, rseg = partition(names, seqs, quals, labels, [False] * 8, zero, tl, sc, mate, rounds, [0, 4, 8])
    # round 16: r5 (single); 8: nothing new (r6 passes, its mate r7 does not); 4: the pair (2, 3); 2: (6, 7);
    # remainder: (0, 1) through r0 alone, r4 through the shorter length
    assert list(rseg) == [8, 8, 4, 4, 9, 1, 7, 7]
    assert [[c[1] for c in row] for row in table] == [[0, 1], [0, 0], [2, 0], [0, 2], [2, 1]]
    assert [ln[1:3] for ln in text.split(b"\n") if ln.startswith(b"@")] == [b"r5", b"r2", b"r3", b"r6", b"r7", b"r0", b"r1", b"r4"]
    assert table[4][1][:2] == (7, 1) and table[4][1][2] + table[4][1][3] == len(text) and text[table[4][1][2]:].startswith(b"@r4 L4\n" + b"A" * 22 + b"\n")


# ---------------------------------------------------------------- the ABI without a device

def _config(**kw):
    c = ka.KmrPartitionConfig()
    assert ka.load().kmr_partition_config_init(C.byref(c)) == 0
    for name, v in kw.items():
        if hasattr(c.select, name) and name != "struct_size":
            setattr(c.select, name, v)
        else:
            setattr(c, name, v)
    return c


def test_new_symbols_are_exported():
    lib = ka.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_partition_config_defaults_and_size():
    """both off: --partition-by-depth -1 and --remainder-trim -1 (src/ReadSelector.h:72); the selection's own defaults inside"""
    c = _config()
    assert c.struct_size == C.sizeof(ka.KmrPartitionConfig) == 48
    assert (c.partition_by_depth, c.remainder_trim) == (0, -1.0)
    s = c.select
    assert s.struct_size == C.sizeof(ka.KmrSelectConfig) == 32 and (s.minimum_score, s.both_pass, s.output_quality_base, s.format, s.scoring_type) == (2.0, 0, 33, 0, 1)
    assert ka.load().kmr_partition_config_init(None) == -1


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_config_null_handle_and_input_starts_are_refused(entry):
    """everything that can be judged without a device is judged before the handle is looked at"""
    lib = ka.load()
    fn = getattr(lib, entry)
    fused = "batch" in entry

    def call(cfg, starts=None):
        out = C.c_void_p(1)
        s = None if starts is None else np.array(starts, dtype=np.uint64)
        args = [None, None, None, 0, None, None, None, None] + ([] if fused else [None, None, None, None])
        args += [None if s is None else s.ctypes.data_as(C.POINTER(C.c_uint64)), 0 if s is None else s.size - 1, C.byref(cfg) if cfg is not None else None, C.byref(out)]
        rc = fn(*args)
        assert out.value is None          # *out is cleared on every failure
        return rc, lib.kmr_last_error(None).decode()
    for bad, why in ((dict(struct_size=44), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(format=2), "format"), (dict(output_quality_base=48), "output_quality_base"),
                     (dict(partition_by_depth=16, minimum_score=2.5), "whole number"), (dict(partition_by_depth=16, minimum_score=-1.0), "whole number")):
        rc, text = call(_config(**bad))
        assert rc == -1 and why in text, (bad, rc, text)
    c = _config()
    c.select.struct_size = 28
    rc, text = call(c)
    assert rc == -1 and "kmr_select_config: struct_size" in text
    rc, text = call(None)
    assert rc == -1 and "NULL" in text
    for starts in ([0, 7, 3, 10], [1, 5, 10], [0, 5, 4]):
        rc, text = call(_config(), starts)
        assert rc == -1 and "input_starts" in text, (starts, text)
    rc, text = call(_config(partition_by_depth=16), list(range(66)))            # 4 rounds x 65 inputs
    assert rc == -7 and "segments" in text
    rc, text = call(_config(partition_by_depth=2 ** 31, minimum_score=0.0, remainder_trim=25.0))            # 33 halvings and a remainder
    assert rc == -7 and "rounds" in text
    rc, text = call(_config(), [0, 4, 4, 10])
    assert rc == -1 and "NULL handle" in text and entry in text
    rc, text = call(_config())
    assert rc == -1 and "NULL handle" in text and entry in text
    assert lib.kmr_picks_segments_info(None, None, None) == -1 and lib.kmr_picks_segments_copy(None, None, None, None, None, None, None, None) == -1


def library_rounds(min_depth, partition_by_depth, remainder_trim=-1.0, min_read_length=0.40, both_pass=0):
    lib = ka.load()
    c = _config(minimum_score=float(min_depth), partition_by_depth=partition_by_depth, remainder_trim=remainder_trim, min_read_length=min_read_length, both_pass=both_pass)
    n = C.c_uint32(77)
    d, l, b, r = np.zeros(33, np.float32), np.zeros(33, np.float32), np.zeros(33, np.uint32), np.zeros(33, np.uint8)
    rc = lib.kmr_partition_rounds(C.byref(c), C.byref(n), d.ctypes.data_as(C.POINTER(C.c_float)), l.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  r.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0, lib.kmr_last_error(None)
    return [dict(depth=float(d[i]), min_read_length=float(l[i]), both_pass=bool(b[i]), is_remainder=bool(r[i])) for i in range(n.value)]


@pytest.mark.parametrize("min_depth,pbd,rem,mrl,both", [
    (2, 16, -1.0, 0.40, 0), (2, 16, 25.0, 0.40, 0), (3, 20, 25.0, 0.40, 0), (2, 2, -1.0, 0.40, 0), (2, 2, 25.0, 0.40, 1), (2, 1, 25.0, 0.40, 0), (2, 0, 25.0, 0.40, 1),
    (1, 2 ** 31, -1.0, 0.40, 0), (1, 2 ** 31, 25.0, 0.40, 0), (2, 16, 25.0, 25.0, 0), (2, 16, 25.0, 25.7, 0), (2, 16, 25.0, 25.0, 1), (0, 2, 3.0, 0.40, 0), (5, 1000, 0.3, 0.40, 0),
    (2 ** 31, 2 ** 31, 25.0, 0.40, 0), (7, 2 ** 32 - 1, 25.0, 0.40, 1)])
def test_library_round_table_is_the_restatement(min_depth, pbd, rem, mrl, both):
    want = round_table(min_depth, pbd, rem, mrl, 2 if both else 1)
    got = library_rounds(min_depth, pbd, rem, mrl, both)
    assert got == want, (got, want)


# ---------------------------------------------------------------- the C++ host side and the host code under the sanitizers

def test_cpp_partition_demo_compiles_and_links(tmp_path):
    """ReadSelector::selectReads of include/kmernator_amd.hpp against the library, warnings as errors"""
    exe = str(tmp_path / "partition_demo")
    lib_dir = os.path.join(ROOT, "kmernator_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "partition_demo.cpp"), "-L" + lib_dir, "-lkmernator_amd", "-Wl,-rpath," + lib_dir])
    assert os.path.exists(exe)


def test_round_table_and_input_starts_in_a_program_of_their_own(tmp_path):
    """tests/cpp/partition_rounds_check.cpp: kmr_select_rounds.hpp, the host arithmetic of the partition, compiled alone with warnings
    as errors and run; it checks its own expectations"""
    exe = str(tmp_path / "partition_rounds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "partition_rounds_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout, p.stdout + p.stderr
