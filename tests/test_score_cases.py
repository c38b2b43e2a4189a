"""The generator of the scoring tests (tests/scorecases.py) held to the reference's semantics on the CPU: every read is in the
class it declares, every class is there for every scoring type, the batches lie on the side of the LDS staging threshold they
are meant for -- so the device comparison of tests/test_gpu_score_trim.py cannot pass on cases that drifted away from the edge
they were written for -- and the restatement those tests compare with (tests/refsemantics.score_and_trim) reproduces the
reference's own FilterReads labels from the oracle's lookups alone."""
import functools
import os

import numpy as np
import pytest

import scorecases as sc
from helpers import GOLDEN, OracleSpectrum, default_config, oracle_weighted_kmers, read_fastq
from refsemantics import score_and_trim

KS = (5, 31, 33)


@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("k", KS)
def test_every_read_is_in_its_class_and_every_class_is_there(k, scoring):
    reads = sc.cases(k) + [sc.long_read(k)]
    seen = set()
    for i, rd in enumerate(reads):
        assert rd.cls in sc.CLASSES and rd.at, rd
        assert len(rd.kcounts) == max(0, len(rd.seq) - k + 1) and rd.kcounts.max(initial=0) <= sc.MAX_COUNT, rd
        for ms in rd.at:
            assert ms in sc.MIN_SCORES
            why = sc.in_class(reads, i, k, ms, scoring)
            assert why is None, why
        seen.add(rd.cls)
    assert seen == set(sc.CLASSES)
    # what the minimum scores at either end do to every read that has a k-mer in front of its first markup
    for i, rd in enumerate(reads):
        if sc._cut(rd, k) == 0:
            continue
        o, l, s, t = score_and_trim(rd.kcounts, rd.seq, k, 0, scoring)
        assert (o, l, t) == (0, sc._cut(rd, k) + k - 1, False), rd          # zero counts pass a minimum of 0
        assert score_and_trim(rd.kcounts, rd.seq, k, 70000, scoring) == (0, 0, -1.0, True), rd


@pytest.mark.parametrize("k", KS)
def test_batches_are_on_their_side_of_the_staging_threshold(k):
    for first in (0, 5):
        st, un = sc.staged_batch(k, first), sc.unstaged_batch(k, first)
        assert int(st.offsets[0]) == int(un.offsets[0]) == first
        assert max(st.spans()) <= sc.SC_CAP and min(un.spans()) > sc.SC_CAP
        assert [r.cls for r in un.reads if r.cls != "long"] == [r.cls for r in st.reads]
        assert st.counts.size == int(st.offsets[-1]) and st.bases.size == st.counts.size + sc.PAD
    # offsets[0] = 5: the first 16-byte load starts in front of the first read, and the byte right in front of it is an N
    b5 = sc.staged_batch(k, 5)
    assert b5.bases[:5].tobytes() == b"N.XAN" and b5.seq(0) == sc.cases(k)[0].seq
    # N, X and . in the padding, inside the last load and behind it; the reference never sees them
    pad = b5.bases[int(b5.offsets[-1]):].tobytes()
    assert len(pad) == sc.PAD and pad[0:4] == b"NNNX" and pad[15:18] == b"NN." and pad[-1:] == b"N"
    for layout in ("base", "scan"):
        lo, hi = sc.threshold_batch(k, layout, 0), sc.threshold_batch(k, layout, 1)
        assert lo.n == hi.n == sc.GROUP + 5
        assert lo.spans(layout) == [sc.SC_CAP, lo.spans(layout)[1]] and hi.spans(layout) == [sc.SC_CAP + 1, lo.spans(layout)[1]]
        differ = [i for i in range(lo.n) if lo.seq(i) != hi.seq(i) or not np.array_equal(lo.kcounts(i), hi.kcounts(i))]
        assert differ == [10]
        assert hi.seq(10)[:-1] == lo.seq(10) and np.array_equal(hi.kcounts(10)[:-1], lo.kcounts(10))
        # the group is worth scoring: trimmed and untrimmed reads, ties, markups
        to, tl, s, wt = lo.reference(2, "MEDIAN")
        assert wt.sum() >= 20 and any(b"N" in lo.seq(i) for i in range(sc.GROUP))
        ties = 0
        for i in range(sc.GROUP):
            runs = sc.passing_runs(lo.kcounts(i), 2)
            best = max(ln for _, ln in runs)
            ties += sum(1 for _, ln in runs if ln == best) > 1
        assert ties >= 5


@pytest.mark.parametrize("k", KS)
def test_geometry_batches(k):
    for n in sc.GEOMETRY:
        b = sc.geometry_batch(k, n)
        assert b.n == n
        spans = b.spans()
        assert len(spans) == (n + sc.GROUP - 1) // sc.GROUP
        unstaged = [g for g, s in enumerate(spans) if s > sc.SC_CAP]
        assert unstaged == {65: [1], 193: [1]}.get(n, [])
        for g in range(sc.GROUP, n, sc.GROUP):          # N right in front of a group's range, and right behind the second group's
            assert b.seq(g - 1)[-1:] == b"N" and b.reads[g - 1].cls == "boundary"
            if g == 2 * sc.GROUP:
                assert b.seq(g)[:1] == b"N"
            else:
                assert b.reads[g].cls in ("tie", "long") and b.reference(2, "MEDIAN")[1][g] > 0
    b = sc.geometry_batch(k, 193)
    assert len(b.spans()) > sc.SC_WAVES          # the fourth group goes to the second block
    # the N in front of a group changes nothing in the group behind it: its first read scores as it does alone
    for g in range(sc.GROUP, 193, sc.GROUP):
        r = b.reads[g]
        assert [x[g] for x in b.reference(2, "MEDIAN")] == list(score_and_trim(r.kcounts, r.seq, k, 2, "MEDIAN"))


def test_average_is_the_rounded_exact_quotient():
    b = sc.unstaged_batch(31)
    for ms in sc.MIN_SCORES:
        assert np.array_equal(b.reference(ms, "AVG")[2].view(np.uint32), b.average(ms).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _e2e(k, others):
    rb = sc.end_to_end_reads(k, others=others)
    return rb, sc.oracle_counts(default_config(k, estimated_raw_kmers=int(rb.offsets[-1])), rb)


@pytest.mark.parametrize("others", [True, False])
@pytest.mark.parametrize("k", sc.E2E_KS)
def test_end_to_end_reads_hold_what_the_device_test_needs(k, others):
    rb, counts = _e2e(k, others)
    lens = np.diff(rb.offsets.astype(np.int64))
    assert rb.n == sc.E2E_SHORT + sc.E2E_LONG
    assert (lens == 0).sum() >= 1 and ((lens > 0) & (lens < k)).sum() >= 5
    longs = lens[sc.E2E_LONG_AT:sc.E2E_LONG_AT + sc.E2E_LONG]
    assert longs.min() >= 200 and longs.max() <= 400 and np.delete(lens, np.arange(sc.E2E_LONG_AT, sc.E2E_LONG_AT + sc.E2E_LONG)).max() <= max(100, k + 40)
    text = rb.bases.tobytes()
    assert all(text.count(c) >= 4 for c in ((b"X", b".", b"n", b"R") if others else (b"X", b"."))) and text.count(b"N") >= 50
    assert others or set(text) <= set(b"ACGTNX.")
    for layout in ("base", "scan"):
        spans = sc.read_spans(rb.offsets, k, layout)
        assert spans[2] > sc.SC_CAP, (layout, spans)
        assert min(spans) <= sc.SC_CAP or (layout == "base" and k == 127), (layout, spans)
    for scoring in ("MEDIAN", "AVG"):
        to, tl, s, wt = sc.reference_of_counts(counts, rb, k, 2, scoring)
        assert wt.sum() >= 20 and (~wt).sum() >= 20 and (s == -1).sum() >= 5
        assert ((s >= 2) & wt).sum() >= 20          # trimmed to a run that has a score
        if k <= 65:
            assert ((s >= 2) & ~wt).sum() >= 20
    # an X or a '.' behind a run that has a score (at k = 127 too few reads have one)
    cutting = sum(1 for i in range(rb.n) if any(c in rb.seq(i) for c in b"X.") and tl[i] > 0)
    assert cutting >= 1 or k == 127


def test_score_and_trim_reproduces_the_golden_labels_from_oracle_lookups():
    """the 949 MedianScore / Trim labels of the reference's own FilterReads run (test/1000-Filtered.fastq) from score_and_trim fed
    with the oracle's lookups of the oracle's k-mers: the restatement rests on the reference's output, not on device counts"""
    k = 31
    rb = read_fastq(os.path.join(GOLDEN, "1000.fastq"))
    gold = read_fastq(os.path.join(GOLDEN, "1000-Filtered.fastq"))
    cfg = default_config(k, fastq_start_char=64, estimated_raw_kmers=(76 - k + 1) * 1000)
    s = OracleSpectrum(cfg)
    s.add_reads(rb)
    s.finalize(2)
    checked = trimmed = 0
    for i in range(rb.n):
        if b"AFTrim" in gold.names[i]:
            continue
        keys, _, _ = oracle_weighted_kmers(cfg, rb.seq(i), rb.qual(i))
        to, tl, score, wt = score_and_trim(s.lookup(keys), rb.seq(i), k, 2, "MEDIAN")
        label = (b"Trim:%d+%d " % (to, tl) if wt else b"") + b"MedianScore:%d" % int(score + 0.5)
        assert label == gold.names[i].split(b" ", 1)[1], (i, label, gold.names[i])
        checked += 1
        trimmed += wt
    assert checked == 949 and trimmed >= 1
