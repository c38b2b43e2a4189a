"""score_reads_kernel held to the reference's semantics (tests/refsemantics.score_and_trim, itself held to the reference's golden
labels in tests/test_score_cases.py) with nothing of the device's on the reference side.

Injected counts: kmr_score_counts_dev takes any count per base position on a handle that was only created, so the reads of
tests/scorecases.py reach every edge of the run selection, the median bisection, the markup scan and the group geometry, once
with every group's counts staged in LDS and once with every group walking global memory.  Everything is compared for equality;
the average too: a sum of at most 2^32 integers <= 65535 is exact in f64, and both sides round the quotient once to f32.

End to end: ragged noisy reads through kmr_score_reads and through kmr_score_read_batch as the ReadSelector calls it, with streaming lookups
(counts indexed by base position) and table probes (counts behind an exclusive scan), against an oracle spectrum built from
the same reads and the oracle's own lookups."""
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import scorecases as sc
from helpers import default_config

pytestmark = pytest.mark.gpu

KS = (5, 31, 33)


# ---------------------------------------------------------------------------------------------------------- injected counts
BUILDERS = {"staged": sc.staged_batch, "unstaged": sc.unstaged_batch, "geometry": sc.geometry_batch,
            "threshold": lambda k, over: sc.threshold_batch(k, "base", over)}


@functools.lru_cache(maxsize=None)
def host_batch(kind, k, arg=0):
    return BUILDERS[kind](k, arg)


class Device:
    """one handle per k -- created, never fed and never finalized: kmr_score_counts_dev needs no spectrum -- and every batch's
    arrays in device memory, for the module's lifetime"""

    def __init__(self):
        self.handles, self.arrays = {}, {}

    def score(self, kind, k, arg, min_score, scoring):
        import torch
        b = host_batch(kind, k, arg)
        if k not in self.handles:
            self.handles[k] = ka.KmerSpectrum(ka.default_config(k, device=0))
        if (kind, k, arg) not in self.arrays:
            bases = torch.from_numpy(b.bases).to("cuda:0")
            offsets = torch.from_numpy(b.offsets.astype(np.int64)).to("cuda:0")
            counts = torch.from_numpy(np.concatenate([b.counts, np.zeros(1, np.uint32)]).view(np.int32)).to("cuda:0")
            assert bases.data_ptr() % 16 == 0 and bases.numel() == int(b.offsets[-1]) + sc.PAD and counts.numel() > int(b.offsets[-1])
            torch.cuda.synchronize()
            self.arrays[(kind, k, arg)] = (bases, offsets, counts)
        bases, offsets, counts = self.arrays[(kind, k, arg)]
        return self.handles[k].score_counts(bases, offsets, b.n, counts, min_score, scoring)

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


@functools.lru_cache(maxsize=None)
def reference(kind, k, arg, min_score, scoring):
    return host_batch(kind, k, arg).reference(min_score, scoring)


@functools.lru_cache(maxsize=None)
def average(kind, k, arg, min_score):
    return host_batch(kind, k, arg).average(min_score)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check(dev, kind, k, arg, scoring):
    """every minimum score: offsets, lengths, flags and scores equal to the reference's, read by read"""
    batch = host_batch(kind, k, arg)
    for ms in sc.MIN_SCORES:
        to, tl, s, wt = dev.score(kind, k, arg, ms, scoring)
        eo, el, es, et = reference(kind, k, arg, ms, scoring)
        for i in range(batch.n):
            got, want = (int(to[i]), int(tl[i]), float(s[i]), bool(wt[i])), (int(eo[i]), int(el[i]), float(es[i]), bool(et[i]))
            assert got == want, (kind, k, arg, scoring, ms, i, batch.reads[i], got, want)
        assert same_bits(s, es)
        if scoring == "AVG":
            assert same_bits(s, average(kind, k, arg, ms)), (kind, k, arg, ms)


@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("k", KS)
def test_cases_staged(dev, k, scoring):
    """every class with its group's counts in LDS (score_one_read<uint16_t>), offsets[0] = 0 and 5"""
    for first in (0, 5):
        assert max(host_batch("staged", k, first).spans()) <= sc.SC_CAP
        check(dev, "staged", k, first, scoring)


@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("k", KS)
def test_cases_unstaged(dev, k, scoring):
    """every class, and the long read, in groups that walk global memory (score_one_read<uint32_t>), offsets[0] = 0 and 5"""
    for first in (0, 5):
        assert min(host_batch("unstaged", k, first).spans()) > sc.SC_CAP
        check(dev, "unstaged", k, first, scoring)


@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("n_reads", sc.GEOMETRY)
def test_group_geometry(dev, n_reads, scoring):
    """a single read, a tail group, full groups, a fourth group on the second block, N right outside a group's range, and a group
    out of LDS between groups in it"""
    for k in KS:
        check(dev, "geometry", k, n_reads, scoring)


@pytest.mark.parametrize("scoring", sc.SCORINGS)
@pytest.mark.parametrize("span", [sc.SC_CAP, sc.SC_CAP + 1])
def test_staging_threshold(dev, span, scoring):
    """64 reads of 10240 bases in all are the last group staged, one base more the first that is not"""
    for k in KS:
        assert host_batch("threshold", k, span - sc.SC_CAP).spans()[0] == span
        check(dev, "threshold", k, span - sc.SC_CAP, scoring)


# --------------------------------------------------------------------------------------------------------------- end to end
def device_spectrum(cfg, rb, stream):
    c = ka.default_config(cfg.k)
    for name, _ in cfg._fields_:
        setattr(c, name, getattr(cfg, name))
    sp = ka.KmerSpectrum(c).tune(stream_lookups=stream)
    sp.buildKmerSpectrum(rb.bases, rb.quals, rb.offsets)
    sp.finalize(2)
    return sp


@functools.lru_cache(maxsize=None)
def oracle_side(kind, k, arg=0):
    rb = sc.end_to_end_reads(k, others=bool(arg)) if kind == "ragged" else sc.threshold_reads(k, kind, arg)
    cfg = default_config(k, estimated_raw_kmers=int(rb.offsets[-1]))
    return rb, cfg, sc.oracle_counts(cfg, rb)


@functools.lru_cache(maxsize=None)
def oracle_reference(kind, k, arg, scoring):
    rb, _, counts = oracle_side(kind, k, arg)
    return sc.reference_of_counts(counts, rb, k, 2, scoring)


STREAMED, PROBED, PROBED_FOR_MARKUP = 1, 2, 3          # kmr_build_info "score_path"


def both_routes(sp, rb, scoring, path):
    """kmr_score_reads on host arrays and kmr_score_read_batch on a device-resident ReadSet -- the entry ReadSelector.scoreAndTrimReads
    calls; the fused kmr_filter_read_batch, which keeps the trims on the device, hands none out and is not reached here -- each
    having taken the lookup path `path`"""
    out = {}
    with ka.ReadSet.from_arrays(sp, rb.bases, rb.quals, rb.offsets) as rs:
        out["kmr_score_reads"] = sp.scoreAndTrimReads(rb.bases, rb.offsets, 2, scoring)
        assert sp.build_info("score_path") == path
        out["kmr_score_read_batch"] = ka.ReadSelector(sp, rs).scoreAndTrimReads(2, scoring)
        assert sp.build_info("score_path") == path
    return out


def assert_routes_equal_reference(sp, rb, want, scoring, what, path):
    eo, el, es, et = want
    for route, (to, tl, s, wt) in both_routes(sp, rb, scoring, path).items():
        for i in range(rb.n):
            got, exp = (int(to[i]), int(tl[i]), float(s[i]), bool(wt[i])), (int(eo[i]), int(el[i]), float(es[i]), bool(et[i]))
            assert got == exp, (what, route, scoring, i, len(rb.seq(i)), got, exp)
        assert same_bits(s, es), (what, route, scoring)


@pytest.mark.parametrize("stream,others", [(1, 0), (0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("k", sc.E2E_KS)
def test_ragged_reads_against_the_oracle(k, stream, others):
    """others = 0: N, X and '.' only -- the streaming lookups take the batch where they are asked for, the table probes where not;
    others = 1: an n and an R in some reads, whose k-mers the reference looks up with an A in their place: the batch is probed
    although streaming lookups are asked for (and where they are not, as any batch).  kmr_build_info "score_path" says which path ran."""
    rb, cfg, _ = oracle_side("ragged", k, others)
    for layout in ("base", "scan"):
        assert sc.read_spans(rb.offsets, k, layout)[2] > sc.SC_CAP
    for scoring in ("MEDIAN", "AVG"):
        to, tl, s, wt = oracle_reference("ragged", k, others, scoring)
        assert wt.sum() >= 20 and (~wt).sum() >= 20 and (s == -1).sum() >= 5
    sp = device_spectrum(cfg, rb, stream)
    for scoring in ("MEDIAN", "AVG"):
        assert_routes_equal_reference(sp, rb, oracle_reference("ragged", k, others, scoring), scoring, (k, stream, others),
                                      STREAMED if stream and not others else PROBED_FOR_MARKUP if stream else PROBED)


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("layout,stream", [("base", 1), ("scan", 0)])
def test_threshold_reads_against_the_oracle(layout, stream, over):
    """the staging threshold where the counts come from lookups: 10240 and 10241 bases in a group with streaming lookups,
    10240 and 10241 k-mers with table probes"""
    k = 31
    rb, cfg, _ = oracle_side(layout, k, over)
    assert sc.read_spans(rb.offsets, k, layout)[0] == sc.SC_CAP + over
    sp = device_spectrum(cfg, rb, stream)
    for scoring in ("MEDIAN", "AVG"):
        want = oracle_reference(layout, k, over, scoring)
        assert want[3].sum() >= 20 and (~want[3]).sum() >= 20
        assert_routes_equal_reference(sp, rb, want, scoring, (layout, over), STREAMED if stream else PROBED)
