"""bimodal_trim_kernel (ReadSelector --bimodal-sigmas) held to the restatement of tests/refbimodal.py, with nothing of the device's
on the reference side.

Injected counts: the directed runs of tests/bimodalcases.py through kmr_score_counts_dev on handles that were only created, for
k = 5 and 33, every scoring type and every sigma, once with the runs staged in LDS and once with every run walked in global memory
(kmr_tune "bimodal_window" 0).  Offsets, lengths, flags and words are compared for equality, scores for equal bits, read by read.
The edge family pins the comparison itself: each run at the two adjacent doubles between which the restatement changes its mind.
End to end: reads that cross a repeat's boundary, scored against an oracle-built spectrum through every scoring entry point, and
the selection's text -- fused and through the host-array forms with kmr_select_bimodal -- equal to the restatement's, tags included."""
import ctypes as C
import functools

import numpy as np
import pytest

import bimodalcases as bc
import kmernator_amd as ka
import refbimodal as rb
import scorecases as sc
from helpers import default_config
from refnormalize import Normalizer, pair_list
from refpartition import partition, round_table

pytestmark = pytest.mark.gpu

KS = (5, 33)


# ---------------------------------------------------------------------------------------------------------- injected counts
@functools.lru_cache(maxsize=None)
def host_batch(kind, k):
    return bc.directed_batch(k) if kind == "directed" else bc.edge_batch(k)[0]


@functools.lru_cache(maxsize=None)
def reference(kind, k, scoring, sigmas, min_score=bc.MIN_SCORE):
    return bc.reference(host_batch(kind, k), min_score, scoring, sigmas)


class Device:
    """one created-only handle per k and every batch's arrays in device memory, for the module's lifetime"""

    def __init__(self):
        self.handles, self.arrays = {}, {}

    def handle(self, k):
        if k not in self.handles:
            self.handles[k] = ka.KmerSpectrum(ka.default_config(k, device=0))
        return self.handles[k]

    def score(self, kind, k, scoring, sigmas, min_score=bc.MIN_SCORE, via_handle=False):
        """(trim_offset, trim_length, score, was_trimmed, words); via_handle: the setting is the handle's, not the call's"""
        import torch
        b, h = host_batch(kind, k), self.handle(k)
        if (kind, k) not in self.arrays:
            bases = torch.from_numpy(b.bases).to("cuda:0")
            offsets = torch.from_numpy(b.offsets.astype(np.int64)).to("cuda:0")
            counts = torch.from_numpy(np.concatenate([b.counts, np.zeros(1, np.uint32)]).view(np.int32)).to("cuda:0")
            assert bases.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            self.arrays[(kind, k)] = (bases, offsets, counts)
        bases, offsets, counts = self.arrays[(kind, k)]
        if via_handle:
            h.setBimodalSigmas(sigmas)
            out = h.score_counts(bases, offsets, b.n, counts, min_score, scoring)
        else:
            out = h.score_counts(bases, offsets, b.n, counts, min_score, scoring, bimodal_sigmas=sigmas)
        return out + (h.bimodal(),)

    def close(self):
        self.arrays.clear()
        for h in self.handles.values():
            h.close()
        self.handles.clear()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def assert_equal(got, want, batch, what, only=None):
    to, tl, s, wt, w = got
    eo, el, es, et, ew = want
    for i in (range(batch.n) if only is None else only):
        g = (int(to[i]), int(tl[i]), float(s[i]), bool(wt[i]), int(w[i]))
        e = (int(eo[i]), int(el[i]), float(es[i]), bool(et[i]), int(ew[i]))
        assert g == e, (what, i, batch.reads[i], rb.tag_of(g[4]), rb.tag_of(e[4]), g, e)
    if only is None:
        assert same_bits(s, es), what


@pytest.mark.parametrize("path", ["staged", "global"])
@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("k", KS)
def test_directed_runs(dev, k, scoring, path):
    """every directed run at every sigma; staged: runs of up to BM_CAP k-mers in LDS and the one beyond it in global memory;
    global: every run in global memory"""
    batch = host_batch("directed", k)
    dev.handle(k).tune(bimodal_window=0 if path == "global" else -1)
    try:
        for sigmas in bc.SIGMAS:
            assert_equal(dev.score("directed", k, scoring, sigmas), reference("directed", k, scoring, sigmas), batch, (k, scoring, path, sigmas))
    finally:
        dev.handle(k).tune(bimodal_window=-1)


def test_runs_where_zero_passes(dev):
    """a minimum score of 0: the failing k-mers of the directed reads join their runs, so sides with a mean of 0 (no floor) occur"""
    for sigmas in (0.0, 2.5):
        want = reference("directed", 5, "AVG", sigmas, 0)
        assert (want[4] != 0).sum() >= 40
        assert_equal(dev.score("directed", 5, "AVG", sigmas, 0), want, host_batch("directed", 5), ("min score 0", sigmas))


@pytest.mark.parametrize("k", KS)
def test_edges_flip_where_the_restatement_does(dev, k):
    """each edge run at the last sigma at which its best split still qualifies and at the next double, where it does not: half of
    the runs are decided by a variance, half by the floor's square root"""
    batch, runs = bc.edge_batch(k)
    for i, (vals, s_lo, s_hi, floored) in enumerate(runs):
        lo = rb.score_and_trim_bimodal(batch.kcounts(i), batch.seq(i), k, bc.MIN_SCORE, "MEDIAN", s_lo)
        hi = rb.score_and_trim_bimodal(batch.kcounts(i), batch.seq(i), k, bc.MIN_SCORE, "MEDIAN", s_hi)
        assert lo != hi
        for sigmas, want in ((s_lo, lo), (s_hi, hi)):
            to, tl, s, wt, w = dev.score("edge", k, "MEDIAN", sigmas)
            got = (int(to[i]), int(tl[i]), float(s[i]), bool(wt[i]), int(w[i]))
            assert got == want, (k, i, vals, floored, sigmas, got, want)


def test_off_after_on_is_an_untouched_handle(dev):
    k = 5
    batch = host_batch("directed", k)
    fresh = ka.KmerSpectrum(ka.default_config(k, device=0))
    try:
        dev.score("directed", k, "MEDIAN", 2.5)
        bases, offsets, counts = dev.arrays[("directed", k)]
        want = fresh.score_counts(bases, offsets, batch.n, counts, bc.MIN_SCORE, "MEDIAN")
        assert not fresh.bimodal().any()
        on = dev.score("directed", k, "MEDIAN", 2.5, via_handle=True)
        assert (on[4] != 0).sum() >= 40 and dev.handle(k).bimodal_sigmas == 2.5
        off = dev.score("directed", k, "MEDIAN", -1.0, via_handle=True)
        for a, b in zip(off[:4], want):
            assert np.array_equal(a, b)
        assert same_bits(off[2], want[2]) and off[4].size == batch.n and not off[4].any()
        eo, el, es, et = batch.reference(bc.MIN_SCORE, "MEDIAN")
        assert np.array_equal(off[0], eo) and np.array_equal(off[1], el) and same_bits(off[2], es) and np.array_equal(off[3], et)
    finally:
        dev.handle(k).setBimodalSigmas(-1.0)
        fresh.close()


def test_argument_errors(dev):
    lib = ka.load()
    sp = ka.KmerSpectrum(ka.default_config(5, device=0))
    try:
        w = np.zeros(8, np.uint64)
        p = w.ctypes.data_as(C.POINTER(C.c_uint64))
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
            sp.setBimodalSigmas(float("nan"))
        assert sp.bimodal_sigmas == -1.0
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
            sp._call("bimodal_copy", sp.h, p, 8)
        assert lib.kmr_set_bimodal_sigmas(None, 1.0) != 0 and lib.kmr_bimodal_copy(None, p, 8) != 0 and lib.kmr_select_bimodal(None, p, 8) != 0
    finally:
        sp.close()
    h = dev.handle(5)
    got = dev.score("edge", 5, "MEDIAN", 2.5)
    n = host_batch("edge", 5).n
    assert got[4].size == n
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        h.bimodal(n + 1)
    assert np.array_equal(h.bimodal(n), got[4])


# --------------------------------------------------------------------------------------------------------------- end to end
E2E_K, E2E_SIGMAS, MRL = 21, (0.5, 2.5), 25.0


@functools.lru_cache(maxsize=None)
def e2e_host():
    reads = bc.boundary_reads(E2E_K)
    cfg = default_config(E2E_K, estimated_raw_kmers=int(reads.offsets[-1]))
    counts = sc.oracle_counts(cfg, reads)
    seqs, quals = [reads.seq(i) for i in range(reads.n)], [reads.qual(i) for i in range(reads.n)]
    names = [b"b%d/%d" % (i // 2, 1 + i % 2) for i in range(reads.n)]
    return reads, cfg, counts, names, seqs, quals


@functools.lru_cache(maxsize=None)
def e2e_want(scoring, sigmas):
    reads, _, counts, names, seqs, quals = e2e_host()
    return rb.reference_of_counts(counts, seqs, E2E_K, 2, scoring, sigmas)


@pytest.fixture(scope="module")
def e2e():
    reads, cfg, counts, names, seqs, quals = e2e_host()
    c = ka.default_config(E2E_K)
    for name, _ in cfg._fields_:
        setattr(c, name, getattr(cfg, name))
    sp = ka.KmerSpectrum(c)
    text = b"".join(b"@" + names[i] + b"\n" + seqs[i] + b"\n+\n" + quals[i] + b"\n" for i in range(reads.n))
    rs = ka.ReadSet(sp, text, input_quality_base=33)
    assert rs.n == reads.n
    sp.buildKmerSpectrumFromReadSet(rs)
    sp.finalize(2)
    yield sp, rs
    rs.close()
    sp.close()


def test_e2e_inputs_are_cut_both_ways():
    for sigmas in E2E_SIGMAS:
        w = e2e_want("MEDIAN", sigmas)[4]
        cut = w != 0
        inv = cut & (((w >> np.uint64(32)) & np.uint64(0xffff)) < (w >> np.uint64(48)))
        assert cut.sum() >= 20 and inv.sum() >= 8 and (cut & ~inv).sum() >= 8 and (~cut).sum() >= 20, (sigmas, cut.sum(), inv.sum())


@pytest.mark.parametrize("scoring", ["MEDIAN", "AVG"])
def test_e2e_scoring_entry_points(e2e, scoring):
    """kmr_score_reads on host arrays and kmr_score_read_batch on the device-resident batch, the setting given with the call and as
    the handle's"""
    sp, rs = e2e
    reads = e2e_host()[0]
    for sigmas in E2E_SIGMAS:
        want = e2e_want(scoring, sigmas)
        got = sp.scoreAndTrimReads(reads.bases, reads.offsets, 2, scoring, bimodal_sigmas=sigmas)
        assert_equal(got + (sp.bimodal(),), want, _Named(reads), ("kmr_score_reads", scoring, sigmas))
        sel = ka.ReadSelector(sp, rs)
        got = sel.scoreAndTrimReads(2, scoring, bimodal_sigmas=sigmas)
        assert_equal(got + (sel.bimodal_words,), want, _Named(reads), ("kmr_score_read_batch", scoring, sigmas))
        sp.setBimodalSigmas(sigmas)
        try:
            got = sel.scoreAndTrimReads(2, scoring)
            assert_equal(got + (sp.bimodal(),), want, _Named(reads), ("kmr_score_read_batch, the handle's setting", scoring, sigmas))
        finally:
            sp.setBimodalSigmas(-1.0)
        sel.close()
    got = sp.scoreAndTrimReads(reads.bases, reads.offsets, 2, scoring)
    assert_equal(got + (sp.bimodal(),), e2e_want(scoring, -1.0), _Named(reads), ("off again", scoring))


class _Named:
    def __init__(self, reads):
        self.n, self.reads = reads.n, ["read %d" % i for i in range(reads.n)]


def _labels(scoring, want):
    to, tl, s, wt, w = want
    return [rb.label_of(scoring, int(to[i]), int(tl[i]), float(s[i]), bool(wt[i]), int(w[i])) for i in range(len(to))]


@pytest.mark.parametrize("sigmas", E2E_SIGMAS)
def test_e2e_text_fused_and_through_the_host_arrays(e2e, sigmas):
    """filterReads, partitioned selectReads and normalized selectReads: the fused call, and scoreAndTrimReads followed by the
    host-array form that takes the tags through kmr_select_bimodal; every text equals the restatement's"""
    sp, rs = e2e
    reads, _, _, names, seqs, quals = e2e_host()
    n = reads.n
    want = e2e_want("MEDIAN", sigmas)
    to, tl, s, wt, w = want
    labels = _labels("MEDIAN", want)
    tagged = sum(1 for lb in labels if b"Bimodal@" in lb)
    assert tagged == int((w != 0).sum()) >= 20 and any(lb.startswith(b"InvBimodal@") for lb in labels) and any(lb.startswith(b"Bimodal@") for lb in labels)
    mate = np.arange(n, dtype=np.int64) ^ 1
    disc = [False] * n
    plain, _, _ = partition(names, seqs, quals, labels, disc, to, tl, s, mate, round_table(2, 0, -1.0, MRL, 1))
    parted, _, _ = partition(names, seqs, quals, labels, disc, to, tl, s, mate, round_table(2, 16, -1.0, MRL, 1))
    r1, r2 = np.arange(0, n, 2, dtype=np.int64), np.arange(1, n, 2, dtype=np.int64)
    normed = Normalizer(6, 2, MRL, True, False, seed=5).run(names, seqs, quals, labels, disc, to, tl, s, pair_list(n, r1, r2))["text"]
    assert plain.count(b"Bimodal@") >= 15 and parted.count(b"Bimodal@") >= 15 and 0 < normed.count(b"Bimodal@") and len(normed) < len(plain)

    def run(sel, kw):
        return {"filterReads": lambda: (sel.filterReads(2, MRL, False, "MEDIAN", **kw) if sel.trims is None else (sel.pickAllPassingPairs(2, MRL, False), sel.writePicks())[1]),
                "partitioned": lambda: sel.selectReads(2, 16, -1.0, MRL, False, "MEDIAN", separate_outputs=False, **kw)[0][1],
                "normalized": lambda: sel.selectReads(2, 0, -1.0, MRL, False, "MEDIAN", separate_outputs=False, max_kmer_output_depth=6, seed=5, **kw)[0][1]}

    expect = {"filterReads": plain, "partitioned": parted, "normalized": normed}
    for what in expect:
        fused = ka.ReadSelector(sp, rs, mate=mate)
        got = run(fused, dict(bimodal_sigmas=sigmas))[what]()
        assert got == expect[what], (what, "fused", sigmas, len(got), len(expect[what]))
        fused.close()
        arrays = ka.ReadSelector(sp, rs, mate=mate)
        arrays.scoreAndTrimReads(2, "MEDIAN", bimodal_sigmas=sigmas)
        got = run(arrays, {})[what]()
        assert got == expect[what], (what, "host arrays", sigmas, len(got), len(expect[what]))
        arrays.close()


def test_select_bimodal_is_consumed_and_checked(e2e):
    sp, rs = e2e
    n = rs.n
    sel = ka.ReadSelector(sp, rs)
    sel.scoreAndTrimReads(2, "MEDIAN", bimodal_sigmas=0.5)
    words = sel.bimodal_words
    hand_in = lambda w: sp._call("select_bimodal", sp.h, None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint64)), 0 if w is None else w.size)
    select = lambda: (sel.pickAllPassingReads(2, MRL), sel.writePicks())[1]
    tagged = select()
    assert tagged.count(b"Bimodal@") >= 20
    sel._tag_args = lambda: None          # from here on the library holds only what this test hands in
    bare = select()                       # the call above consumed its tags
    assert bare.count(b"Bimodal@") == 0 and len(bare) < len(tagged)
    hand_in(words)
    assert select() == tagged and select() == bare
    hand_in(words)
    hand_in(None)                         # NULL takes them back
    assert select() == bare
    hand_in(words[:n - 1].copy())         # a count that is not the batch's is refused by the call that would use it, and does not linger
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        select()
    assert select() == bare
    sel.close()
