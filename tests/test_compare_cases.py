"""CompareSpectrums on the CPU: the restatement (tests/refcompare.py) by two routes that share no code, every family of
tests/comparecases.py against the restatement with its one rule changed, kmr_compare_line and the header byte for byte, and the
new symbols of the library."""
import ctypes as C

import numpy as np
import pytest

import comparecases as cc
import kmernator_amd as ka
from helpers import default_config
from kmernator_amd import _lib
from refcompare import HEADER, Comparer, evaluate, line, oracle_set_map

K = 21


def cfg_of(k, min_weight=0.10):
    return default_config(k, min_weight=min_weight)


@pytest.fixture(scope="module")
def set2_map():
    return Comparer(cfg_of(K)).set_map(cc.set2())


def reads_of(fam):
    return [(s, q) for _, _, s, q in fam]


@pytest.mark.parametrize("k,min_weight", [(21, 0.10), (22, 0.10), (33, 0.0), (65, 0.10)])
def test_read_map_equals_oracle_spectrum_of_that_read(k, min_weight):
    """(a) a read's map from buildWeightedKmers and the weight test == the oracle's solid spectrum built from that read alone;
    and the sum of the reads' maps == the oracle's spectrum of the set"""
    cfg = cfg_of(k, min_weight)
    cmp_ = Comparer(cfg)
    reads = reads_of(cc.families(k) + cc.circular(k))
    m2 = cmp_.set_map(cc.set2())
    for seq, qual in reads:
        m1 = cmp_.read_map(seq, qual)
        o1 = oracle_set_map(cfg, [(seq, qual)])
        assert m1 == o1
        assert evaluate(m1, m2) == evaluate(o1, m2)
    assert m2 == oracle_set_map(cfg, cc.set2())
    assert {k_: c for k_, c in m2.items() if c >= 2} == oracle_set_map(cfg, cc.set2(), min_depth=2)


class DistinctOnly(Comparer):
    """counts occurrences as distinct keys"""
    def add(self, m, key):
        m[key] = 1


class NoWeightTest(Comparer):
    def passes(self, w):
        return True


class NoCanonical(Comparer):
    def key(self, canonical, forward_text):
        return forward_text


class KMinusOne(Comparer):
    """drops the doubled first k-mer of a circular read"""
    def circular_extra(self):
        return self.k - 1


def _family(k, name):
    return [r for r in cc.families(k) if r[0] == name]


DEVIATIONS = [
    ("homopolymer", DistinctOnly, 21), ("tandem", DistinctOnly, 21), ("palindrome", DistinctOnly, 22),
    ("with_n", NoWeightTest, 21), ("low_quality", NoWeightTest, 21),
    ("strand", NoCanonical, 21), ("genome", NoCanonical, 21),
]


@pytest.mark.parametrize("family,deviant,k", DEVIATIONS)
def test_every_family_notices_its_deviation(family, deviant, k):
    """(b)"""
    cfg = cfg_of(k)
    reads = reads_of(_family(k, family))
    assert reads
    m2 = Comparer(cfg).set_map(cc.set2())
    want = Comparer(cfg).per_read(reads, m2)
    got = deviant(cfg).per_read(reads, m2)
    assert want != got


def test_circular_family_notices_k_minus_one():
    cfg = cfg_of(K)
    reads = reads_of(cc.circular(K))
    m2 = Comparer(cfg).set_map(cc.set2())
    a, b = Comparer(cfg), KMinusOne(cfg)
    want, got = a.per_read(a.circularize(reads), m2), b.per_read(b.circularize(reads), m2)
    assert want != got
    # the first k-mer of a circular sequence is counted twice
    L = len(reads[0][0])
    assert want[0]["total_count1"] == L + 1 and got[0]["total_count1"] == L
    assert a.circularize([(b"ACGT", b"IIII")], 9) == [(b"ACGTACGT", b"IIIIIIII")] and a.circularize([(b"", b"")]) == [(b"", b"")]


def test_strand_and_weight_families_mean_what_they_say(set2_map):
    cfg = cfg_of(K)
    cmp_ = Comparer(cfg)
    s = reads_of(_family(K, "strand"))
    assert cmp_.read_map(*s[0]) == cmp_.read_map(*s[1])
    lq = reads_of(_family(K, "low_quality"))[0]
    strict, lax = cmp_.read_map(*lq), Comparer(cfg_of(K, 0.0)).read_map(*lq)
    assert 0 < len(strict) < len(lax) == len(lq[0]) - K + 1
    short = reads_of(_family(K, "short"))[0]
    assert evaluate(cmp_.read_map(*short), set2_map) == dict(size1=0, size2=len(set2_map), common=0, common_count1=0, common_count2=0, total_count1=0,
                                                              total_count2=sum(set2_map.values()), saturated=0)
    so = reads_of(_family(K, "singleton_only"))[0]
    r = evaluate(cmp_.read_map(*so), set2_map)
    assert r["common"] == r["size1"] == r["common_count2"] == len(so[0]) - K + 1
    hp = evaluate(cmp_.read_map(*reads_of(_family(K, "homopolymer"))[0]), set2_map)
    assert hp["size1"] == 1 and hp["total_count1"] == 41


LINE_RECORDS = [
    dict(size1=3, size2=7, common=2, common_count1=5, common_count2=9, total_count1=6, total_count2=1234567, saturated=0),
    dict(size1=0, size2=0, common=0, common_count1=0, common_count2=0, total_count1=0, total_count2=0, saturated=0),
    dict(size1=0, size2=7, common=0, common_count1=0, common_count2=0, total_count1=0, total_count2=12, saturated=0),
    dict(size1=5, size2=0, common=0, common_count1=0, common_count2=0, total_count1=9, total_count2=0, saturated=0),
    dict(size1=1, size2=1, common=1, common_count1=1, common_count2=1, total_count1=1, total_count2=1, saturated=0),
    dict(size1=3, size2=3, common=1, common_count1=1, common_count2=2, total_count1=3, total_count2=3, saturated=0),
    dict(size1=99999, size2=100000, common=99994, common_count1=1, common_count2=99995, total_count1=3 * 10 ** 9, total_count2=100000, saturated=0),
    dict(size1=2 ** 40, size2=2 ** 41 + 1, common=2 ** 39 + 12345, common_count1=2 ** 50, common_count2=7, total_count1=2 ** 52 + 1, total_count2=2 ** 63, saturated=3),
    dict(size1=1000000, size2=8, common=1, common_count1=1, common_count2=1, total_count1=123456789, total_count2=9, saturated=0),
]


@pytest.mark.parametrize("rec", LINE_RECORDS)
@pytest.mark.parametrize("label", [b"", b"read/1 comment", b"x" * 300])
def test_line_matches_the_restatement_byte_for_byte(rec, label):
    """(c) kmr_compare_line against the reference's stream formatting, the -nan of a zero denominator included; needs no device"""
    assert ka.compare_line(rec, label) == line(rec, label)


def test_header_and_nan_line():
    assert ka.COMPARE_HEADER == HEADER == b"\nSet 1\tSet 2\tCommon\t%Uniq1\t%Tot1\t%Uniq2\t%Tot2\n"
    assert ka.compare_line(LINE_RECORDS[1]) == b"0\t0\t0\t-nan\t-nan\t-nan\t-nan\t\n"
    assert ka.compare_line(LINE_RECORDS[0], b"r") == b"3\t7\t2\t66.67\t83.33\t28.57\t0.000729\tr\n"


def test_line_capacity_and_arguments():
    lib = ka.load()
    c = _lib.KmrCompareCounts(3, 7, 2, 5, 9, 6, 1234567, 0)
    want = line(LINE_RECORDS[0], b"abc")
    nb = C.c_uint64()
    buf = C.create_string_buffer(len(want))
    assert lib.kmr_compare_line(C.byref(c), b"abc", 3, buf, len(want) - 1, C.byref(nb)) == -6 and nb.value == len(want)      # KMR_ERR_CAPACITY
    assert lib.kmr_compare_line(C.byref(c), b"abc", 3, buf, len(want), C.byref(nb)) == 0 and buf.raw == want
    assert lib.kmr_compare_line(None, b"", 0, buf, len(want), C.byref(nb)) == -1
    assert lib.kmr_compare_line(C.byref(c), None, 3, buf, len(want), C.byref(nb)) == -1


def test_symbols_are_exported_and_fail_loudly_without_a_device():
    """(d)"""
    lib = ka.load()
    for name in ("kmr_compare_spectrums", "kmr_compare_reads", "kmr_compare_reads_dev", "kmr_compare_line", "kmr_reads_circularize"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert C.sizeof(_lib.KmrCompareCounts) == 64 == ka.COMPARE_DTYPE.itemsize
    out = _lib.KmrCompareCounts()
    r = C.c_void_p()
    # no handle can exist without a device (kmr_create fails with KMR_ERR_NO_DEVICE), and no entry point invents one
    assert lib.kmr_compare_spectrums(None, None, C.byref(out)) == -1
    assert lib.kmr_compare_reads(None, None, None) == -1
    assert lib.kmr_compare_reads_dev(None, None, None) == -1
    assert lib.kmr_reads_circularize(None, None, 21, C.byref(r)) == -1 and not r.value
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(ka.KmerSpectrumError, match="NO_DEVICE"):
            ka.KmerSpectrum(ka.default_config(31))
