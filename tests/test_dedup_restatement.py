"""CPU-side checks of the duplicate-fragment stage: the restatement in tests/refdedup.py against the reference's own consensus
fixtures (testConsensus, test/ReadSetTest.cpp:219-242) and against cases worked by hand; kmr_consensus_qual, the host helper
that shares the device's quality steps, against getQualChar; and the shape of the C-ABI (kmr_dedup_*)."""
import ctypes as C
import os

import numpy as np
import pytest

import kmernator_amd as ka
from kmernator_amd import _lib
from helpers import GOLDEN
import refdedup

FIXTURES = ["consensus1", "consensus2", "consensus3", "consensus2-diff"]


@pytest.mark.parametrize("name", [f + s for f in FIXTURES for s in (".fastq", ".std.fastq")])
def test_consensus_fixtures(name):
    """testConsensus: minimum quality 0, the reads at even indices in one set and those at odd indices in the other; the consensus
    of each set has the bases of the file's first two reads"""
    reads = refdedup.parse_fastq(open(os.path.join(GOLDEN, name), "rb").read())
    assert len(reads) >= 2 and len(reads) % 2 == 0
    if not name.endswith(".std.fastq"):          # Phred-64: the reference rescales to 33 as it reads (src/ReadSet.cpp:324-337)
        reads = [(n, b, "".join(chr(ord(c) - 31) for c in q)) for n, b, q in reads]
    assert len(refdedup.pair_list(reads)) == len(reads) // 2
    table = refdedup.quality_to_probability(3, 33)          # made before the test lowers the minimum
    for side in (0, 1):
        name_, bases, quals = refdedup.consensus_read(reads[side::2], 0, 33, table)
        assert bases == reads[side][1]
        assert name_ == "C%d-%s" % (len(reads) // 2, reads[side][0])
        assert len(quals) == len(bases) and all(33 <= ord(c) <= 73 for c in quals)


def _qual(lib, p):
    return ord(lib.kmr_consensus_qual(float(p)))


def test_consensus_qual_matches_get_qual_char():
    lib = ka.load()          # no device needed
    for p in (0.0, 0.25, 0.2501, 0.9999, 1.0):
        assert _qual(lib, p) == refdedup.get_qual_char(p, 0), p
    assert _qual(lib, 0.0) == 0 and _qual(lib, 0.9999) == 40 and _qual(lib, 1.0) == 40
    # the double at which the expression steps to q, and two neighbours on either side
    for q in range(1, 40):
        lo, hi = 0.0, 0.9999
        for _ in range(200):
            mid = (lo + hi) / 2
            if refdedup.prob_to_qual(mid) >= q:
                hi = mid
            else:
                lo = mid
        assert np.nextafter(lo, 1.0) == hi or lo == hi
        assert refdedup.prob_to_qual(hi) == q and (refdedup.prob_to_qual(lo) == q - 1 or lo == hi)
        p = np.nextafter(np.nextafter(hi, 0.0), 0.0)
        for _ in range(5):
            if p < 0.9999:
                assert _qual(lib, p) == refdedup.get_qual_char(float(p), 0), (q, p)
            p = np.nextafter(p, 1.0)
    rng = np.random.default_rng(7)
    for p in rng.random(10000):
        assert _qual(lib, p) == refdedup.get_qual_char(float(p), 0), p


def test_abi_shape():
    lib = ka.load()
    for name in ("kmr_dedup_config_init", "kmr_dedup_fragments", "kmr_dedup_fragments_dev", "kmr_dedup_info", "kmr_dedup_copy", "kmr_dedup_device_ptrs",
                 "kmr_dedup_reads", "kmr_dedup_names_copy", "kmr_dedup_free", "kmr_consensus_qual"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    c = _lib.KmrDedupConfig()
    assert lib.kmr_dedup_config_init(C.byref(c)) == 0
    assert c.struct_size == C.sizeof(_lib.KmrDedupConfig) == 28
    # _DuplicateFragmentFilterOptions' constructor (src/DuplicateFragmentFilter.h:60-61); deDupSingle false = the paired pass
    assert (c.dedup_mode, c.paired, c.consensus, c.edit_distance, c.start_offset, c.dedup_length) == (0, 1, 1, 0, 0, 24)
    assert lib.kmr_dedup_config_init(None) == -1


def _fragments_rc(lib, **fields):
    """the configuration is checked before anything else, so its verdict is there without a handle"""
    c = _lib.KmrDedupConfig()
    lib.kmr_dedup_config_init(C.byref(c))
    c.dedup_mode = 1
    for k, v in fields.items():
        setattr(c, k, v)
    out = C.c_void_p()
    rc = lib.kmr_dedup_fragments(None, None, None, 0, None, None, C.byref(c), C.byref(out))
    assert not out.value
    return rc


def test_config_checks():
    lib = ka.load()
    assert _fragments_rc(lib) == -1                                  # a good configuration: the NULL handle is what is wrong
    assert b"NULL argument" in lib.kmr_last_error(None)
    assert _fragments_rc(lib, struct_size=24) == -1 and b"struct_size" in lib.kmr_last_error(None)
    for bad in (dict(dedup_length=22), dict(start_offset=2), dict(dedup_length=0), dict(dedup_mode=3), dict(paired=2)):
        assert _fragments_rc(lib, **bad) == -1, bad                  # KMR_ERR_INVALID_ARG (the option check, :137)
        assert b"kmr_dedup_config" in lib.kmr_last_error(None)
    for unsupported in (dict(edit_distance=1), dict(consensus=0), dict(dedup_length=68)):
        assert _fragments_rc(lib, **unsupported) == -7, unsupported  # KMR_ERR_UNSUPPORTED
    assert _fragments_rc(lib, dedup_length=64) == -1 and b"NULL argument" in lib.kmr_last_error(None)


def test_no_device_means_no_handle():
    import torch
    if torch.cuda.is_available():
        return          # the calls themselves are exercised in test_gpu_dedup.py
    h = C.c_void_p()
    cfg = ka.default_config(31)
    assert ka.load().kmr_create(C.byref(cfg), C.byref(h)) == -2          # KMR_ERR_NO_DEVICE: there is no CPU path


@pytest.mark.parametrize("case", refdedup.HAND_CASES, ids=[c[0] for c in refdedup.HAND_CASES])
def test_hand_worked_cases(case):
    label, reads, cfg, discarded, expect = case
    got = refdedup.run_case(case)
    assert got.groups == expect["groups"], label
    assert got.skipped == expect["skipped"], label
    assert got.discarded == expect["discarded"], label
    assert got.affected == expect["affected"], label
    assert got.consensus == expect["consensus"], label


def test_hand_cases_reach_what_they_name():
    by = {c[0]: refdedup.run_case(c) for c in refdedup.HAND_CASES}
    assert by["flipped_duplicate_mode2"].flipped == 1 and by["key_equal_to_its_reverse_complement"].flipped == 0


def test_generator_reaches_every_path():
    reads, discarded = refdedup.generate(1)
    pairs = refdedup.pair_list(reads)
    assert 1500 <= len(pairs) <= 3000
    for mode in (1, 2):
        r = refdedup.filter_duplicate_fragments(reads, pairs, discarded, dedup_mode=mode, dedup_length=24)
        assert all(v > 0 for v in r.skipped[:3]) and r.skipped[3] == 0
        sizes = [m for _, m in r.groups]
        assert len(sizes) > 50 and max(sizes) >= 3
        assert any(len(b) > 64 for _, b, _ in r.consensus) and any("!" in q for _, _, q in r.consensus)
    assert r.flipped > 0
    assert refdedup.filter_duplicate_fragments(reads, pairs, discarded, dedup_mode=1, dedup_length=24).groups != r.groups
    s = refdedup.filter_duplicate_fragments(reads, pairs, r.discarded, dedup_mode=2, paired=False, dedup_length=24)
    assert len(s.groups) > 5 and s.skipped[2] > 0
