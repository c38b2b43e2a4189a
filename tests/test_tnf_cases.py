"""TnfDistance without a device: the column calls of the library (kmr_tnf_dims, kmr_tnf_columns, kmr_tnf_header) against the
restatement of tests/reftnf.py, and the directed inputs of tests/tnfcases.py against mutated restatements -- every family must notice
the deviation it was written for, so that the equalities of tests/test_gpu_tnf.py prove what they claim."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import reftnf
import tnfcases as tc
from helpers import default_config
from reftnf import EUCLIDEAN, SPEARMAN, F32, F64, Tnf

KS = (1, 2, 3, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def tnf(k, hash_kind=0):
    return Tnf(default_config(k, hash_kind=hash_kind))


@functools.lru_cache(maxsize=None)
def distance_counts(k, n=24):
    """the vectors of the first n sequences of the set the device's distance tests use"""
    t = tnf(k)
    return np.array([t.vector(s, q) for s, q in tc.distance_set(n, k)], dtype=np.uint64)


def bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("k", KS)
def test_dims_and_columns(k):
    t = tnf(k)
    assert t.D == reftnf.dims(k) == ((4 ** k + 4 ** (k // 2)) // 2 if k % 2 == 0 else 4 ** k // 2)
    assert [reftnf.dims(j) for j in KS] == [2, 10, 32, 136, 512, 2080]
    assert len(set(t.codes)) == t.D
    assert all(c <= reftnf.revcomp_code(c, k) for c in t.codes)
    assert set(t.codes) == {min(c, reftnf.revcomp_code(c, k)) for c in range(4 ** k)}


@pytest.mark.parametrize("hash_kind", (0, 1))
@pytest.mark.parametrize("k", KS)
def test_library_columns_equal_restatement(k, hash_kind):
    t = tnf(k, hash_kind)
    assert ka.tnf_dims(k) == t.D
    assert list(ka.tnf_columns(k, hash_kind)) == t.codes
    assert ka.tnf_header(k, hash_kind) == t.header()
    if k > 1:
        assert t.codes != sorted(t.codes)                    # the map's order is not the code order


def test_library_column_refusals():
    lib = ka.load()
    d, nb = C.c_uint32(), C.c_uint64()
    codes = np.zeros(4096, dtype=np.uint16)
    for k in (0, 7, 32):
        assert lib.kmr_tnf_dims(k, C.byref(d)) == -7
        assert lib.kmr_tnf_columns(k, 0, codes.ctypes.data_as(C.POINTER(C.c_uint16))) == -7
        assert lib.kmr_tnf_header(k, 0, None, 0, C.byref(nb)) == -7
    assert lib.kmr_tnf_dims(4, None) == -1 and lib.kmr_tnf_columns(4, 0, None) == -1 and lib.kmr_tnf_columns(4, 2, codes.ctypes.data_as(C.POINTER(C.c_uint16))) == -1
    assert lib.kmr_tnf_header(4, 0, None, 0, C.byref(nb)) == -6 and nb.value == len(tnf(4).header())      # KMR_ERR_CAPACITY, with the size


# ------------------------------------------------------------------------------------------------------------------------- mutations
class PlainColumns(Tnf):
    def column_key(self, code):
        return code


class ClosedWindowBound(Tnf):
    def window_bound(self, i, limit):
        return i <= limit


class WindowsWithOwnQuality(Tnf):
    def window_qual(self, seq, qual, i, window):
        return qual[i:i + window]


class FusedAccumulate(Tnf):
    def accumulate(self, dist, d):
        return (dist.astype(F64) + d.astype(F64) * d.astype(F64)).astype(F32)      # one rounding, as a multiply-add has


class TiesByPosition(Tnf):
    def tie_rank(self, tie_sum, tie_size, rank):
        return F32(rank)


class IndexWithoutOne(Tnf):
    def hist_index(self, v, formula, bins):
        return max(0, Tnf.hist_index(self, v, formula, bins) - 1)


def mutant(cls, k):
    return cls(default_config(k))


@pytest.mark.parametrize("k", (4, 6))
def test_column_order_shows_in_a_distance_bit(k):
    """the same vectors summed in plain code order give another float somewhere: the device's equality proves its column order"""
    a, m = tnf(k), mutant(PlainColumns, k)
    assert m.codes == sorted(a.codes) != a.codes
    reads = tc.distance_set(24, k)
    va, vm = distance_counts(k), np.array([m.vector(s, q) for s, q in reads], dtype=np.uint64)
    assert np.array_equal(np.sort(va, axis=1), np.sort(vm, axis=1))
    assert (bits(a.euclidean(va, va)) != bits(m.euclidean(vm, vm))).any()
    # (the Spearman sums are sums of quarters below 2^24 at these D: exact in float, so no order shows in them)


@pytest.mark.parametrize("k", (1, 4, 6))
def test_fused_multiply_add_shows_in_a_distance_bit(k):
    v = distance_counts(k)
    plain, fused = tnf(k).euclidean(v, v), mutant(FusedAccumulate, k).euclidean(v, v)
    assert (bits(plain) != bits(fused)).any()
    assert np.allclose(plain, fused, rtol=1e-5, atol=1e-7)


def test_window_bound_is_strict():
    window, step = 40, 7
    reads = tc.window_lengths(window, step)
    a, m = tnf(4), mutant(ClosedWindowBound, 4)
    got = [len(a.shred(s, q, window, step)) for s, q in reads]
    assert got == [0, 0, 1, 2, 4]
    assert [len(m.shred(s, q, window, step)) for s, q in reads][1] == 1          # L == window: one window under <=


def test_windows_carry_reference_quality():
    s, q = tc.low_middle()
    a, m = tnf(4), mutant(WindowsWithOwnQuality, 4)
    wa, wm = a.shred(s, q, 120, 30), m.shred(s, q, 120, 30)
    assert len(wa) == len(wm) == 6
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(wa, wm))
    assert all(int(v.sum()) == 117 for _, v in wa)
    assert int(a.vector(s, q).sum()) < 297 == int(a.vector(s, tc.REF * len(s)).sum())      # the sequence's own vector loses the middle


def test_ties_share_a_rank():
    v = distance_counts(6)
    a, m = tnf(6), mutant(TiesByPosition, 6)
    assert (bits(a.spearman(v, v)) != bits(m.spearman(v, v))).any()
    r = a.ranks(np.array([5, 0, 0, 7, 0, 5], dtype=F32))
    assert list(r) == [4.5, 2.0, 2.0, 6.0, 2.0, 4.5]


@pytest.mark.parametrize("formula", (EUCLIDEAN, SPEARMAN))
def test_histogram_index(formula):
    a, m = tnf(4), mutant(IndexWithoutOne, 4)
    end = a.hist_end(formula)
    assert a.hist_index(F32(0.0), formula, 7) == 1 and a.hist_index(end, formula, 7) in (7, 8) and a.hist_index(np.nextafter(end, F32(2)), formula, 7) == 8
    assert a.hist_index(F32(-0.5), formula, 7) == 0
    reads, _, starts = tc.three_inputs(150, 25)
    ha, hm = a.likelihoods(reads, starts, 150, 25, bins=7, formula=formula), m.likelihoods(reads, starts, 150, 25, bins=7, formula=formula)
    assert not np.array_equal(ha, hm)
    assert (ha[:2, 0] == 0).all() and (ha[:2, -1] == 0).all()


def test_likelihood_totals_and_subsampling():
    a = tnf(4)
    reads, _, starts = tc.three_inputs(150, 25)
    w, _, b = a.windows(reads, starts, 150, 25, 112)
    sizes = [int(b[g + 1] - b[g]) for g in range(3)]
    assert sizes[1] == 1 and min(sizes[0], sizes[2]) > 1
    h = a.likelihoods(reads, starts, 150, 25, bins=100)
    assert int(h[0].sum()) == sum(s * (s - 1) // 2 for s in sizes if s > 1)
    assert int(h[1].sum()) == sizes[0] * sizes[1] + sizes[0] * sizes[2] + sizes[1] * sizes[2]
    assert int(h[2].sum()) == sum(s for s in sizes if s > 1) and int(h[3].sum()) == 2 * sum(sizes)
    assert a.likelihoods(reads, starts, 150, 25, bins=100, max_samples=30) is None
