"""TnfDistance on the device (kmr_tnf_*; kmernator_amd/csrc/kmr_tnf.hpp) held to the restatement of tests/reftnf.py over the directed
inputs of tests/tnfcases.py.  Every comparison is for equality: counts as integers, lengths and distances by their bits.
tests/test_tnf_cases.py shows that these inputs make a contracted multiply-add and a wrong column order visible in a distance bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import tnfcases as tc
from helpers import default_config
from reftnf import EUCLIDEAN, SPEARMAN, F32, Tnf

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 6)
FORMULAS = (EUCLIDEAN, SPEARMAN)


# ------------------------------------------------------------------------------------------------------------------- reference side
@functools.lru_cache(maxsize=None)
def ref(k):
    return Tnf(default_config(k))


@functools.lru_cache(maxsize=None)
def ref_vectors(k, what, n=0):
    reads = {"a": lambda: tc.distance_set(n, k, 80), "b": lambda: tc.distance_set(n, k, 81), "long": lambda: [tc.long_sequence()]}[what]()
    return ref(k).read_vectors(reads)


@functools.lru_cache(maxsize=None)
def ref_matrix(k, formula, na, nb):
    return ref(k).distances(ref_vectors(k, "a", na), ref_vectors(k, "b", nb), formula)


@functools.lru_cache(maxsize=None)
def ref_triangle(k, formula, n):
    return ref(k).triangle(ref_vectors(k, "a", n), formula)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape, np.argwhere(got != want)[:6])


# ---------------------------------------------------------------------------------------------------------------------- device side
def arrays_of(reads):
    lens = np.array([len(s) for s, _ in reads], dtype=np.uint64)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    b = np.frombuffer(b"".join(s for s, _ in reads) + b"\0", dtype=np.uint8)
    q = np.frombuffer(b"".join(q for _, q in reads) + b"\0", dtype=np.uint8)
    return b, q, off


class Handles:
    """one never-fed handle per k for the module's lifetime"""

    def __init__(self):
        self.sp = {}

    def __call__(self, k):
        if k not in self.sp:
            self.sp[k] = ka.KmerSpectrum(ka.default_config(k, device=0, estimated_raw_kmers=4096))
        return self.sp[k]

    def close(self):
        for sp in self.sp.values():
            sp.close()
        self.sp.clear()


@pytest.fixture(scope="module")
def dev():
    d = Handles()
    yield d
    d.close()


def read_set(sp, reads):
    return ka.ReadSet.from_arrays(sp, *arrays_of(reads))


def check_vectors(t, r, reads, starts=None):
    want = r.read_vectors(reads)
    assert t.n == len(reads) and t.dims == r.D and t.inexact == 0
    assert np.array_equal(t.counts(), want)
    same_bits(t.lengths(), r.lengths(want.astype(F32)))
    assert np.array_equal(t.origin(), np.array([(i, 0, len(s)) for i, (s, _) in enumerate(reads)], dtype=np.uint64).reshape(len(reads), 3))
    assert list(t.groups()) == ([0, len(reads)] if starts is None else list(starts))
    return want


# --------------------------------------------------------------------------------------------------------------------------- vectors
@pytest.mark.parametrize("k", KS)
def test_vector_families(dev, k):
    fam = tc.vector_families(k)
    reads = [(s, q) for _, s, q in fam]
    names = [f for f, _, _ in fam]
    with read_set(dev(k), reads) as rs, rs.tnf() as t:
        got = check_vectors(t, ref(k), reads)
    for f in ("empty", "km1") + tuple("n_mod_%d" % r for r in range(k)):
        assert not got[names.index(f)].any(), f
    assert got[names.index("exact")].sum() == 1 and got[names.index("kp1")].sum() == 2
    assert np.count_nonzero(got[names.index("homopolymer_a")]) == 1 and got[names.index("homopolymer_a")].sum() == 200 - k + 1
    assert np.array_equal(np.flatnonzero(got[names.index("homopolymer_a")]), np.flatnonzero(got[names.index("homopolymer_t")]))


@pytest.mark.parametrize("k", (4, 6))
def test_many_short_sequences_in_one_batch(dev, k):
    reads = tc.short_batch(300)
    starts = np.array([0, 100, 100, 300], dtype=np.uint64)
    with read_set(dev(k), reads) as rs, rs.tnf(starts) as t:
        check_vectors(t, ref(k), reads, starts)
        assert t.n_groups == 3


@pytest.mark.parametrize("piece", (64, 65, 0))
@pytest.mark.parametrize("k", (4, 6))
def test_long_sequence_across_pieces(dev, k, piece):
    """a 20 kb contig between short sequences: a k-mer that straddles a piece edge counts once, whatever the piece"""
    reads = [tc.fasta(b"ACGTTGCA" * 3), tc.long_sequence(), tc.fasta(b"GGGCCCAT" * 9)]
    sp = dev(k)
    sp.tune(tnf_piece_bases=piece)
    try:
        with read_set(sp, reads) as rs, rs.tnf() as t:
            got = t.counts()
            lengths = t.lengths()
    finally:
        sp.tune(tnf_piece_bases=0)
    want = np.concatenate([ref(k).read_vectors(reads[:1]), ref_vectors(k, "long"), ref(k).read_vectors(reads[2:])])
    assert np.array_equal(got, want)
    same_bits(lengths, ref(k).lengths(want.astype(F32)))


def test_own_quality_against_window_quality(dev):
    """the middle third of a FASTQ sequence has quality 2: its own vector loses those k-mers, the window over the same bases keeps them"""
    k, r = 4, ref(4)
    s, q = tc.low_middle()
    reads = [(s + b"A", q + b"I")]                        # one base more than the window, so that there is exactly one
    with read_set(dev(k), reads) as rs, rs.tnf() as whole, rs.tnfWindows(len(s), 1000) as win:
        a, b = whole.counts(), win.counts()
    assert np.array_equal(a, r.read_vectors(reads))
    wv, org, _ = r.windows(reads, [0, 1], len(s), 1000, len(s) * 3 // 4)
    assert np.array_equal(b, wv) and b.shape == (1, r.D)
    assert a.sum() < b.sum() == len(s) - k + 1


def test_from_fasta_text(dev):
    k = 4
    reads, names, starts = tc.three_inputs(150, 25)
    reads = reads + [tc.fasta(tc.random_bases(333, 90).lower())]
    names = names + [b"lower_case"]
    with ka.ReadSet.from_fasta(dev(k), tc.fasta_text(reads, names)) as rs, rs.tnf() as t:
        assert rs.arrays()[3] == names
        check_vectors(t, ref(k), reads)


# --------------------------------------------------------------------------------------------------------------------------- windows
def check_windows(t, r, reads, starts, window, step, min_count):
    wv, org, bounds = r.windows(reads, starts, window, step, min_count)
    assert t.n == len(wv) and t.inexact == 0
    assert np.array_equal(t.counts(), wv)
    assert np.array_equal(t.origin(), org)
    assert np.array_equal(t.groups(), bounds)
    same_bits(t.lengths(), r.lengths(wv.astype(F32)))
    return wv, org, bounds


@pytest.mark.parametrize("k", (1, 4, 6))
def test_window_bounds(dev, k):
    window, step = 40, 7
    reads = tc.window_lengths(window, step)
    with read_set(dev(k), reads) as rs, rs.tnfWindows(window, step) as t:
        _, org, _ = check_windows(t, ref(k), reads, [0, len(reads)], window, step, window * 3 // 4)
    assert [int((org[:, 0] == i).sum()) for i in range(len(reads))] == [0, 0, 1, 2, 4]


@pytest.mark.parametrize("min_count,kept", [(0, 6), (-5, 6), (40 * 3 // 4, 4), (38, 0), (10 ** 9, 0)])
def test_window_purge(dev, min_count, kept):
    """the first and the last window are mostly N: window * 3 / 4 drops exactly those two, the order of the others stays"""
    k, window = 4, 40
    reads = [tc.with_gaps(window, 6)]
    with read_set(dev(k), reads) as rs, rs.tnfWindows(window, window, min_count=min_count) as t:
        _, org, _ = check_windows(t, ref(k), reads, [0, 1], window, window, min_count)
    assert t.n == kept
    if kept == 4:
        assert list(org[:, 1]) == [40, 80, 120, 160]


def test_windows_of_three_inputs(dev):
    k, window, step = 4, 40, 7
    reads, starts = tc.no_window_inputs(window, step)
    with read_set(dev(k), reads) as rs, rs.tnfWindows(window, step, input_starts=starts) as t:
        _, _, bounds = check_windows(t, ref(k), reads, starts, window, step, window * 3 // 4)
    assert list(bounds) == [0, 0, 1, t.n] and t.n_groups == 3
    with read_set(dev(k), reads[:1]) as rs, rs.tnfWindows(window, step) as t:
        assert t.n == 0 and t.counts().shape == (0, ref(k).D) and list(t.groups()) == [0, 0]


def test_group_sums(dev):
    k, r = 4, ref(4)
    reads = tc.short_batch(300)
    starts = np.array([0, 100, 100, 300], dtype=np.uint64)
    with read_set(dev(k), reads) as rs, rs.tnf(starts) as t, t.groupSums() as g:
        counts, sums = t.counts(), g.counts()
        assert g.n == 3 and g.inexact == 0 and list(g.groups()) == [0, 1, 2, 3]
        assert np.array_equal(g.origin(), np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=np.uint64))
        want = r.group_sums(counts, starts)
        assert np.array_equal(sums, np.array([counts[0:100].sum(axis=0), counts[100:100].sum(axis=0), counts[100:300].sum(axis=0)]))
        assert np.array_equal(sums.astype(F32), want)          # the reference's float adds, exact below 2^24
        same_bits(g.lengths(), r.lengths(want))
        for formula in FORMULAS:
            same_bits(t.distances(g, formula), r.distances(counts.astype(F32), want, formula))


# ------------------------------------------------------------------------------------------------------------------------- distances
class Sets:
    """the device vectors of the first n sequences of a distance set, made once per (k, which, n)"""

    def __init__(self, dev):
        self.dev, self.t = dev, {}

    def __call__(self, k, which, n):
        key = (k, which, n)
        if key not in self.t:
            with read_set(self.dev(k), tc.distance_set(n, k, 80 if which == "a" else 81)) as rs:
                self.t[key] = rs.tnf()
            assert np.array_equal(self.t[key].counts(), ref_vectors(k, which, n))
        return self.t[key]

    def close(self):
        for t in self.t.values():
            t.close()


@pytest.fixture(scope="module")
def sets(dev):
    s = Sets(dev)
    yield s
    s.close()


@pytest.mark.parametrize("formula", FORMULAS)
@pytest.mark.parametrize("nb", (1, 64, 65))
@pytest.mark.parametrize("na", (1, 2, 63, 64, 65, 130))
def test_distance_rectangles(sets, na, nb, formula):
    k = 4
    got = sets(k, "a", na).distances(sets(k, "b", nb), formula)
    same_bits(got, ref_matrix(k, formula, 130, 65)[:na, :nb])
    assert got.shape == (na, nb)


@pytest.mark.parametrize("formula", FORMULAS)
@pytest.mark.parametrize("k", (1, 6))
def test_distances_at_the_smallest_and_the_largest_k(sets, k, formula):
    """D = 2 and D = 2080: less than one slice of columns, and 65 slices"""
    a, b = sets(k, "a", 66), sets(k, "b", 65)
    same_bits(a.distances(b, formula), ref_matrix(k, formula, 66, 65))
    same_bits(a.distances(None, formula), ref_triangle(k, formula, 66))


@pytest.mark.parametrize("formula", FORMULAS)
def test_triangle_whole_and_in_row_ranges(sets, formula):
    k, n = 4, 130
    a = sets(k, "a", n)
    want = ref_triangle(k, formula, n)
    whole = a.distances(None, formula)
    same_bits(whole, want)
    for cut in (70, 64, 1):                               # 70 splits a tile of 64 rows
        top, rest = a.distances(None, formula, 0, cut), a.distances(None, formula, cut, n - cut)
        assert top.size == cut * (cut - 1) // 2
        same_bits(np.concatenate([top, rest]), want)
    assert a.distances(None, formula, 5, 0).size == 0
    # the fourth sequence repeats the third: distance +0; the second holds no k-mer: length 1
    assert bits(whole)[3 * 2 // 2 + 2] == 0
    assert a.lengths()[1] == 1.0 and not a.counts()[1].any()


def test_heavy_ties_are_in_the_set():
    v = ref_vectors(6, "a", 66)
    assert (v == 0).mean() > 0.8


# ----------------------------------------------------------------------------------------------------------------------- likelihoods
@pytest.mark.parametrize("formula", FORMULAS)
@pytest.mark.parametrize("bins", (1, 7, 100))
@pytest.mark.parametrize("windows", ("equal", "different"))
@pytest.mark.parametrize("inputs", (1, 3))
def test_likelihoods(dev, inputs, windows, bins, formula):
    k, r = 4, ref(4)
    reads, _, starts = tc.three_inputs(150, 25)
    if inputs == 1:
        starts = np.array([0, len(reads)], dtype=np.uint64)
    o = dict(window=150, step=25, bins=bins, formula=formula)
    if windows == "different":
        o.update(window2=200, step2=50)
    want = r.likelihoods(reads, starts, **o)
    with read_set(dev(k), reads) as rs:
        got = rs.tnfLikelihoods(starts, **o)
    assert np.array_equal(got, want)
    # the totals the loops imply, and no outliers among the window pairs
    w1, _, b1 = r.windows(reads, starts, 150, 25, 112)
    w2, _, b2 = (w1, None, b1) if windows == "equal" else r.windows(reads, starts, 200, 50, 150)
    s1, s2 = np.diff(b1).astype(int), np.diff(b2).astype(int)
    G = len(s1)
    intra = sum((s1[g] * (s1[g] - 1) // 2 if windows == "equal" else s1[g] * s2[g]) for g in range(G) if s1[g] > 1)
    inter = sum(s1[i] * s2[j] for i in range(G) for j in range(i if windows == "equal" else G) if i != j)
    assert [int(x) for x in got.sum(axis=1)] == [intra, inter, sum(s for s in s1 if s > 1), (G - 1) * int(s1.sum())]
    assert not got[:2, 0].any() and not got[:2, -1].any()
    if inputs == 3:
        assert s1[1] == 1


def test_likelihoods_refuse_to_subsample(dev):
    reads, _, starts = tc.three_inputs(150, 25)
    assert ref(4).likelihoods(reads, starts, 150, 25, max_samples=30) is None
    with read_set(dev(4), reads) as rs:
        with pytest.raises(ka.KmerSpectrumError, match="UNSUPPORTED.*subsample"):
            rs.tnfLikelihoods(starts, window=150, step=25, max_samples=30)
        assert rs.tnfLikelihoods(starts, window=150, step=25, max_samples=10 ** 6).sum() > 0


# ------------------------------------------------------------------------------------------------------------------------------ text
@pytest.mark.parametrize("formula", FORMULAS)
def test_texts_of_a_three_file_case(dev, formula):
    k, r = 4, ref(4)
    reads, names, starts = tc.three_inputs(150, 25)
    refs, ref_names = [tc.fasta(tc.random_bases(500, 95, gc=0.4)), tc.fasta(tc.random_bases(120, 96, gc=0.6))], [b"ref_a", b"ref_b"]
    o = dict(window=150, step=25, window2=200, step2=50, bins=7)
    sp = dev(k)
    with ka.ReadSet.from_fasta(sp, tc.fasta_text(reads, names)) as rs, ka.ReadSet.from_fasta(sp, tc.fasta_text(refs, ref_names)) as rr:
        plain = ka.TnfDistance(rs, starts, inter_distance=True, intra_inter=o, formula=formula)
        against = ka.TnfDistance(rs, starts, reference=rr, formula=formula)
    assert plain["output"] == r.table(reads, names)
    assert plain["inter_distance"] == r.inter_text(reads, names, formula)
    assert plain["intra_inter"] == r.likelihood_text(r.likelihoods(reads, starts, formula=formula, **o), 150, 200, 7, formula)
    assert against["output"] == r.reference_text(reads, names, refs, formula)
    assert sorted(against) == ["output"] and against["output"].count(b"\n") == len(reads)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    lib = ka.load()
    sp7 = ka.KmerSpectrum(ka.default_config(7, device=0, estimated_raw_kmers=4096))
    try:
        with read_set(sp7, tc.short_batch(3)) as rs:
            with pytest.raises(ka.KmerSpectrumError, match="UNSUPPORTED"):
                rs.tnf()
            with pytest.raises(ka.KmerSpectrumError, match="UNSUPPORTED"):
                rs.tnfWindows(40, 7)
            with pytest.raises(ka.KmerSpectrumError, match="UNSUPPORTED"):
                rs.tnfLikelihoods()
    finally:
        sp7.close()
    sp = dev(4)
    out = C.c_void_p()
    with read_set(sp, tc.short_batch(5)) as rs, rs.tnf() as t:
        assert lib.kmr_tnf_reads(sp.h, None, None, 0, C.byref(out)) == -1 and lib.kmr_tnf_reads(sp.h, rs.r, None, 0, None) == -1
        assert lib.kmr_tnf_windows(sp.h, rs.r, None, 0, 40, 0, 0, C.byref(out)) == -1          # a step of 0
        assert lib.kmr_tnf_group_sums(sp.h, None, C.byref(out)) == -1
        assert lib.kmr_tnf_distances(sp.h, None, None, 0, 0, 0, None) == -1
        assert lib.kmr_tnf_distances(sp.h, t._t, None, 2, 0, t.n, None) == -1                  # no such formula
        assert lib.kmr_tnf_distances(sp.h, t._t, None, 0, 3, t.n, None) == -1                  # rows beyond the set
        assert lib.kmr_tnf_distances(sp.h, t._t, None, 0, 0, t.n, None) == -1                  # nowhere to write
        assert lib.kmr_tnf_likelihoods(sp.h, rs.r, None, 0, None, None) == -1
        assert lib.kmr_tnf_info(None, None, None, None, None) == -1 and lib.kmr_tnf_copy(None, None, None, None, None) == -1
        bad = np.array([0, 9], dtype=np.uint64)
        assert lib.kmr_tnf_reads(sp.h, rs.r, bad.ctypes.data_as(C.POINTER(C.c_uint64)), 1, C.byref(out)) == -1      # does not end at n
        with rs.tnf() as u, u.groupSums() as g:
            with pytest.raises(ka.KmerSpectrumError, match="UNSUPPORTED"):
                g.groupSums()
