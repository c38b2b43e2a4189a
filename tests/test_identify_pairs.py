"""Pair identification (ReadSet::identifyPairs, src/ReadSet.cpp:446-570) without a device: the sequential restatement of
tests/refpairs.py against cases worked by hand from the reference's code, the seeded generator the GPU tests share, and the
C-ABI of kmr_identify_pairs*."""
import ctypes as C

import pytest

import kmernator_amd as ka
from kmernator_amd import _lib
import refpairs

SYMBOLS = ["kmr_identify_pairs", "kmr_identify_pairs_dev", "kmr_pairs_info", "kmr_pairs_copy", "kmr_pairs_device_ptrs", "kmr_pairs_free"]
INVALID_ARG = -1
SEEDS = (1, 2, 3)


@pytest.mark.parametrize("case", refpairs.HAND_CASES, ids=[c[0] for c in refpairs.HAND_CASES])
def test_restatement_gives_the_hand_worked_pairs(case):
    label, lines, store_comment, mate, pairs = case
    r = refpairs.identify_pairs(lines, store_comment)
    assert r.mate == mate
    assert r.pairs == pairs
    assert r.n_full == sum(1 for a, b in pairs if a >= 0 and b >= 0)
    assert r.has_pairs() == (0 < len(pairs) < len(lines))


def test_name_helpers_on_the_reference_s_corner_cases():
    assert refpairs.trim_name("n 1:N:0:A", 0)[:2] == ("n/1", "") and refpairs.trim_name("n 1:N:0:A", 1)[:2] == ("n", "1:N:0:A")
    assert refpairs.trim_name("n/1 2:N:0:A", 0)[:2] == ("n/1", "")             # already ends in /x: not rewritten
    assert refpairs.trim_name("/1 2:N:0:A", 0)[:2] == ("/1/2", "")             # pos <= 2: rewritten whatever the name ends in
    assert refpairs.trim_name("n 2:Y:0:A", 1)[2] is False and refpairs.trim_name("n 2:N:0:A", 1)[2] is True
    assert refpairs.trim_name("n x", 1)[:2] == ("n", "x") and refpairs.trim_name("n ", 1)[:2] == ("n", "")
    assert refpairs.trim_name("n\r", 1)[:2] == ("n", "")
    assert [refpairs.read_num(n, "") for n in ("a/1", "a/A", "a/F", "a/2", "a/B", "a/R", "a/3", "a", "/1", "1")] == [1, 1, 1, 2, 2, 2, 0, 0, 1, 0]
    assert refpairs.read_num("a/1", "2:N:0:A") == 2                             # the comment wins
    assert [refpairs.common_name(n) for n in ("a/1", "/1", "ab", "ab/", "a/1/2")] == ["a/", "/1", "ab", "ab/", "a/1/"]


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_takes_every_branch(seed):
    """so that the GPU comparison on these batches cannot pass on easy inputs alone"""
    lines = refpairs.generate(seed)
    kept, rewritten = refpairs.identify_pairs(lines, 1), refpairs.identify_pairs(lines, 0)
    for r in (kept, rewritten):
        print("seed %d: %d reads, %d pairs (%d sequential, %d by name), conflicts read1 %d read2 %d, chain reads %d, readNum 0 matches %d"
              % (seed, r.n_reads, r.n_pairs, r.n_sequential, r.name_matched, r.conflict_read1, r.conflict_read2, r.chain_reads, r.zero_matches))
        assert r.n_sequential > 0 and r.name_matched > 0
        assert r.conflict_read1 > 0 and r.conflict_read2 > 0
        assert r.chain_reads > 0
        assert r.zero_matches > 0
        assert r.has_pairs()
    assert refpairs.casava_rewrites(lines, 0) > 0 and refpairs.casava_rewrites(lines, 1) == 0
    assert kept.pairs != rewritten.pairs          # the rewrite matters on this batch


def test_the_symbols_are_exported_and_bound():
    lib = ka.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.kmr_abi_version() == 1


def test_null_arguments_are_invalid_arg():
    lib = ka.load()
    out = C.c_void_p()
    # refused before anything is looked at: any non-NULL address will do for the other arguments
    standin = C.create_string_buffer(256)
    x = C.cast(standin, C.c_void_p)
    for fn in (lib.kmr_identify_pairs, lib.kmr_identify_pairs_dev):
        assert fn(None, x, None, 0, 1, C.byref(out)) == INVALID_ARG and not out.value
        assert fn(x, None, None, 0, 1, C.byref(out)) == INVALID_ARG and not out.value
        assert fn(x, x, None, 0, 1, None) == INVALID_ARG
        assert fn(x, x, None, 5, 1, C.byref(out)) == INVALID_ARG and not out.value          # a length without a text
    n = C.c_uint64()
    assert lib.kmr_pairs_info(None, C.byref(n), None, None, None, None, None) == INVALID_ARG
    assert lib.kmr_pairs_copy(None, None, None, None) == INVALID_ARG
    assert lib.kmr_pairs_device_ptrs(None, C.byref(out), None, None) == INVALID_ARG
    lib.kmr_pairs_free(None)          # a no-op, as free(NULL)


def test_python_mirror_has_the_methods():
    assert callable(ka.ReadSet.identifyPairs)
    for name in ("getPairSize", "hasPairs", "device_ptrs", "close"):
        assert callable(getattr(ka.ReadPairs, name)), name
    for name in ("mate", "pairs"):
        assert isinstance(getattr(ka.ReadPairs, name), property), name
