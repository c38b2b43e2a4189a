"""The restatement of the bimodal cut (tests/refbimodal.py) and the directed runs (tests/bimodalcases.py), on the CPU: that the
restatement is scoreAndTrimReads itself while the option is off, that its two forms agree, that each misreading it names changes
the result of a read of the family written for it, that the inputs hold what the device test needs of them, and the labels.
The device is held to all of it in tests/test_gpu_bimodal.py."""
import inspect
import math

import numpy as np
import pytest

import bimodalcases as bc
import refbimodal as rb
from refsemantics import score_and_trim

K = 5


@pytest.fixture(scope="module")
def batch():
    return bc.directed_batch(K)


@pytest.fixture(scope="module")
def results(batch):
    """the restatement's answer for every directed read at every sigma (MEDIAN)"""
    return {s: bc.reference(batch, bc.MIN_SCORE, "MEDIAN", s) for s in bc.SIGMAS}


def test_off_is_score_and_trim(batch):
    for scoring in ("SUM", "MEDIAN", "MIN", "MAX", "AVG"):
        for i in range(batch.n):
            want = score_and_trim(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, scoring)
            for sigmas in (-1.0, -0.5, float("-inf")):
                assert rb.score_and_trim_bimodal(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, scoring, sigmas) == want + (0,)


def test_the_fast_form_is_the_plain_form(batch):
    """numpy running sums against the Python loops, bit for bit, on every directed run short enough for the loops"""
    n = 0
    for i in range(batch.n):
        toff, tlen, _, _ = score_and_trim(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, "MIN")
        vals = [float(v) for v in batch.kcounts(i)[toff:toff + max(0, tlen - K + 1)]]
        if 3 <= len(vals) <= 140:
            for s in bc.SIGMAS:
                assert rb.find_partition_fast(vals, s) == rb.find_partition_plain(vals, s), (i, s)
                n += 1
    assert n > 300


def test_mean_std_count_is_the_references():
    m, s, c = rb.mean_std_count([7.0])
    assert (m, s, c) == (7.0, math.sqrt(7.0), 1)          # one value: the mean undivided, variance 0, the floor
    assert rb.mean_std_count([0.0, 0.0]) == (0.0, 0.0, 2)          # no floor under a mean of 0
    m, s, c = rb.mean_std_count([10.0, 70.0, 10.0, 70.0])
    assert (m, s) == (40.0, 1200.0)          # the variance, not its root
    assert rb.split_diff(2.9, 0.2) == 2.0 and rb.split_diff(0.2, 2.9) == 2.0 and rb.split_diff(0.2, 2.9, "float_abs") == 2.9 - 0.2


def test_every_deviant_is_told_apart(batch, results):
    """each misreading changes a read of the family written for it at some sigma, and the list of families is complete"""
    assert set(bc.WRITTEN_FOR) == set(rb.DEVIANTS)
    for deviant, family in bc.WRITTEN_FOR.items():
        changed = {}
        if family == "edge":      # at the two sigmas around each run's flip point
            eb, runs = bc.edge_batch(K)
            for i, (vals, s_lo, s_hi, floored) in enumerate(runs):
                changed[i] = [s for s in (s_lo, s_hi) if rb.score_and_trim_bimodal(eb.kcounts(i), eb.seq(i), K, bc.MIN_SCORE, "MEDIAN", s, deviant)
                              != rb.score_and_trim_bimodal(eb.kcounts(i), eb.seq(i), K, bc.MIN_SCORE, "MEDIAN", s)]
        else:
            mine = [i for i in range(batch.n) if batch.reads[i].cls == family]
            for s in bc.SIGMAS:
                got = rb.reference_of_counts([batch.kcounts(i) for i in mine], [batch.seq(i) for i in mine], K, bc.MIN_SCORE, "MEDIAN", s, deviant)
                changed[s] = [i for j, i in enumerate(mine) if any(got[c][j] != results[s][c][i] for c in range(5))]
        print(deviant, family, {s: len(v) for s, v in changed.items() if v})
        assert any(changed.values()), (deviant, family)


def test_the_inputs_hold_what_the_device_test_needs(batch, results):
    lens = set()
    cut_any, inv_any = np.zeros(batch.n, bool), np.zeros(batch.n, bool)
    for s in bc.SIGMAS:
        to, tl, sc, wt, words = results[s]
        cut = words != 0
        m1, m2 = (words >> np.uint64(32)) & np.uint64(0xffff), words >> np.uint64(48)
        inv = cut & (m1 < m2)
        print("sigmas %s: %d of %d reads cut, %d of them Inv" % (s, cut.sum(), batch.n, inv.sum()))
        assert cut.sum() * 3 >= batch.n and inv.sum() * 4 >= cut.sum() and (cut & ~inv).sum() * 4 >= cut.sum()
        assert wt[cut].all() and (tl[cut] >= K).all()
        cut_any |= cut
        inv_any |= inv
        assert (tl[cut] == K).any()          # a reduced run of one k-mer
    for i in range(batch.n):
        toff, tlen, _, _ = score_and_trim(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, "MIN")
        lens.add(max(0, tlen - K + 1))
    assert set(bc.LENGTHS) | {bc.BM_CAP, bc.BM_CAP + 1} <= lens
    assert cut_any[63] and cut_any[64] and batch.n % 64 and batch.n % bc.BM_WAVES
    fam = lambda f: [i for i, r in enumerate(batch.reads) if r.cls == f]
    assert set(r.cls for r in batch.reads) == set(bc.FAMILIES)
    assert all(cut_any[i] for i in fam("window"))
    # a run that does not start at k-mer 0 and one that a markup ends, both cut
    to0 = results[0.0][0]
    assert all(cut_any[i] for i in fam("offset")) and all(score_and_trim(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, "MIN")[0] > 0 for i in fam("offset"))
    assert all(cut_any[i] for i in fam("markup")) and all(any(c in b"NX." for c in batch.seq(i)) for i in fam("markup"))
    assert to0 is not None
    # sides whose variance is above the floor, and sides where the floor stands in
    w0 = results[0.0][4]
    decided = {f: [rb.threshold([float(v) for v in _run(batch, i)], int(w0[i] & np.uint64(0xffffffff)) - K)[3] for i in fam(f) if w0[i]] for f in ("variance", "floor")}
    assert decided["variance"] and not any(decided["variance"]) and decided["floor"] and all(decided["floor"])


def _run(batch, i):
    toff, tlen, _, _ = score_and_trim(batch.kcounts(i), batch.seq(i), K, bc.MIN_SCORE, "MIN")
    return batch.kcounts(i)[toff:toff + tlen - K + 1]


def test_edge_family_flips_between_adjacent_doubles():
    eb, runs = bc.edge_batch(K)
    assert sum(1 for r in runs if r[3]) == 16 and sum(1 for r in runs if not r[3]) == 16
    for i, (vals, s_lo, s_hi, floored) in enumerate(runs):
        assert math.nextafter(s_lo, math.inf) == s_hi
        a = rb.score_and_trim_bimodal(eb.kcounts(i), eb.seq(i), K, bc.MIN_SCORE, "MEDIAN", s_lo)
        b = rb.score_and_trim_bimodal(eb.kcounts(i), eb.seq(i), K, bc.MIN_SCORE, "MEDIAN", s_hi)
        assert a[4] and a != b, (i, vals, s_lo, a, b)


def test_labels():
    k = 31
    w = rb.word_of(40, k, 38.7, 4.2)
    assert rb.tag_of(w) == b"Bimodal@71:38/4" and rb.tag_of(rb.word_of(3, k, 4.2, 38.7)) == b"InvBimodal@34:4/38" and rb.tag_of(0) == b""
    assert rb.label_of("MEDIAN", 0, 70, 38.0, True, w) == b"Bimodal@71:38/4 Trim:0+70 MedianScore:38"
    assert rb.label_of("AVG", 3, 97, 37.6, True, rb.word_of(3, k, 4.2, 38.7), aftrim=(2, 100)) == b"AFTrim:2+98 InvBimodal@34:4/38 Trim:3+97 AvgScore:38"
    assert rb.label_of("MIN", 0, 100, 12.0, False) == b"MinScore:12" and rb.label_of("MAX", 0, 0, -1.0, True) == b"Trim:0+0 MaxScore:0"
    # through the whole restatement: the head of a 40x / 4x read is kept, the tail of a 4x / 40x read
    head = rb.score_and_trim_bimodal([40] * 30 + [4] * 20, b"A" * (49 + k), k, 2, "MEDIAN", 2.5)
    tail = rb.score_and_trim_bimodal([4] * 20 + [40] * 30, b"A" * (49 + k), k, 2, "MEDIAN", 2.5)
    assert head == (0, 30 + k - 1, 40.0, True, rb.word_of(30, k, 40, 4)) and tail == (20, 30 + k - 1, 40.0, True, rb.word_of(20, k, 4, 40))
    assert rb.label_of("MEDIAN", *head[:5]) == b"Bimodal@61:40/4 Trim:0+60 MedianScore:40"
    assert rb.label_of("MEDIAN", *tail[:5]) == b"InvBimodal@51:4/40 Trim:20+60 MedianScore:40"


def test_the_package_names_the_feature():
    """the three symbols and the keyword of every scoring entry of the Python layer (this fails without the feature)"""
    import kmernator_amd as ka
    from kmernator_amd import _lib
    for name in ("kmr_set_bimodal_sigmas", "kmr_bimodal_copy", "kmr_select_bimodal"):
        assert name in _lib.EXPORTS
    header = open(_lib.LIB_PATH.replace("kmernator_amd/csrc/libkmernator_amd.so", "include/kmernator_amd.h")).read()
    for name in ("kmr_set_bimodal_sigmas", "kmr_bimodal_copy", "kmr_select_bimodal"):
        assert "int %s(kmr_handle *h" % name in header
    for fn in (ka.KmerSpectrum.scoreAndTrimReads, ka.KmerSpectrum.score_counts, ka.ReadSelector.scoreAndTrimReads, ka.ReadSelector.filterReads,
               ka.ReadSelector.selectReads, ka.ReadSelector.pickCoverageNormalizedSubset):
        assert inspect.signature(fn).parameters["bimodal_sigmas"].default == -1.0, fn
    assert callable(ka.KmerSpectrum.setBimodalSigmas) and callable(ka.KmerSpectrum.bimodal)
