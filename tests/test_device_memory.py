"""Every device block the library allocates is given back: kmr_build_info("device_blocks_live") counts the blocks of the whole
process, and a probe handle kept open for the whole test reads it before and after each step.  Whole life cycles return to the
baseline, and an error the API returns after it has allocated leaves nothing behind: the second failure of the same call finds
the count where the first one left it."""
import numpy as np
import pytest

import kmernator_amd as ka
from helpers import GOLDEN, KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_EXT, synth_reads

pytestmark = pytest.mark.gpu

N_READS, READ_LEN = 3000, 150


def _live(probe):
    return int(probe.build_info("device_blocks_live"))


def _spectrum(k, mode, ext=False, **kw):
    vk = {"value_kind": KMR_VALUE_EXT} if ext else {}
    return ka.KmerSpectrum(ka.default_config(k, estimated_raw_kmers=N_READS * (READ_LEN - k + 1), device=0, build_mode=mode, **vk, **kw))


@pytest.fixture(scope="module")
def probe():
    p = _spectrum(31, 1)
    yield p
    p.close()


@pytest.fixture(scope="module")
def reads():
    return synth_reads(N_READS, read_len=READ_LEN, seed=5, quality="noisy", n_rate=0.002)


def _packed_keys(p, n=64):
    return np.random.default_rng(1).integers(0, 256, size=(n, p.kb), dtype=np.uint8)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [31, 51])
@pytest.mark.parametrize("ext", [False, True])
def test_life_cycle_returns_every_block(probe, reads, mode, k, ext):
    """create -> build -> finalize -> every lookup form -> score -> image / merge / histogram / digest -> reset -> rebuild -> destroy"""
    base = _live(probe)
    p = _spectrum(k, mode, ext)
    p.buildKmerSpectrum(reads.bases, reads.quals, reads.offsets)
    p.finalize(1)
    keys = _packed_keys(p)
    p.getCount(keys)
    p.getCount(keys, useWeights=True)
    sub = reads.slice(0, 200)
    p.getCountsForReads(sub.bases, sub.offsets)
    p.getCountsForReads(sub.bases, sub.offsets, useWeights=True)
    p.scoreAndTrimReads(sub.bases, sub.offsets, 0.5)
    wi, si = p.image(KMR_MAP_WEAK), p.image(KMR_MAP_SINGLETON)
    p.merge_image(KMR_MAP_WEAK, wi)
    p.histogram()
    p.getHistogram()
    p.digest(KMR_MAP_WEAK)
    p.digest(KMR_MAP_SINGLETON)
    q = _spectrum(k, 1, ext)
    q.load_image(KMR_MAP_WEAK, wi)
    q.load_image(KMR_MAP_SINGLETON, si)
    q.getCount(keys)
    q.close()
    p.reset()
    p.buildKmerSpectrum(reads.bases, reads.quals, reads.offsets)
    p.finalize(2)
    p.getCount(keys)
    assert _live(probe) > base
    p.close()
    assert _live(probe) == base


def test_read_batches_and_artifact_filter_return_every_block(probe, reads):
    base = _live(probe)
    p = _spectrum(31, 3)
    text = open(GOLDEN + "/1000.fastq", "rb").read()
    rs = ka.ReadSet(p, text)
    p.buildKmerSpectrumFromReadSet(rs)
    host = ka.ReadSet.from_arrays(p, reads.bases, reads.quals, reads.offsets)
    tw, to, _, _, _ = rs.twobit()
    offs = rs.arrays()[2]
    p.buildKmerSpectrumTwoBit(tw, to, offs, uniform_quality=ord("I"))
    two = ka.ReadSet.from_twobit(p, tw, to, offs, uniform_quality=ord("I"))
    p.finalize(1)
    p.scoreAndTrimReadSet(rs, 0.5)
    f = ka.FilterKnownOddities(p, open(GOLDEN + "/artifact_sequences.fa", "rb").read())
    _, out = f.applyFilter(rs)
    for r in (out, two, host, rs):
        r.close()
    f.close()
    p.close()
    assert _live(probe) == base


def _twice(probe, call):
    """run a call that fails after it has allocated, twice: the second failure leaves the count where the first one did"""
    counts = []
    for _ in range(2):
        with pytest.raises(ka.KmerSpectrumError):
            call()
        counts.append(_live(probe))
    assert counts[1] == counts[0], counts


def test_errors_after_allocating_leave_nothing_behind(probe, reads):
    base = _live(probe)
    p = _spectrum(31, 3, num_buckets_weak=512, num_buckets_singleton=1024)
    p.buildKmerSpectrum(reads.bases, reads.quals, reads.offsets)
    p.finalize(1)
    _twice(probe, lambda: ka.ReadSet(p, b"@r\nACGT\n+\nIIII\n@s\nACGT\n+\nII\n"))        # malformed FASTQ, found after the line index
    wrong = _spectrum(31, 1, num_buckets_weak=256, num_buckets_singleton=1024)
    sub = reads.slice(0, 10)
    wrong.buildKmerSpectrum(sub.bases, sub.quals, sub.offsets)
    wrong.finalize(1)
    wi = wrong.image(KMR_MAP_WEAK)
    _twice(probe, lambda: p.merge_image(KMR_MAP_WEAK, wi))                                # maps of different bucket counts
    si = p.image(KMR_MAP_SINGLETON)
    _twice(probe, lambda: p.merge_image(KMR_MAP_SINGLETON, si))                           # singleton maps that share k-mers
    wrong.close()
    p.close()
    assert _live(probe) == base


def _stage_spectrum(text):
    """a finalized k=31 spectrum (mode 3, EXT values, so that mergraph works) of the FASTQ `text`, and the text's batch"""
    p = _spectrum(31, 3, ext=True)
    rs = ka.ReadSet(p, text)
    p.buildKmerSpectrumFromReadSet(rs)
    p.finalize(1)
    return p, rs


def test_read_stages_return_every_block(probe):
    """identifyPairs, the selector, the duplicate-fragment filter (its empty branch on 1000.fastq, its consensus branch on
    consensus3.fastq, each with the single pass behind) and the mercount / mergraph text"""
    base = _live(probe)
    p, rs = _stage_spectrum(open(GOLDEN + "/1000.fastq", "rb").read())
    pairs = rs.identifyPairs()
    sel = ka.ReadSelector(p, rs, mate=pairs.mate)
    sel.filterReads()
    assert len(sel.writePicks()) == sel.bytes
    dd = ka.DuplicateFragmentFilter(p, dedup_mode=1).filterDuplicateFragments(rs, pairs, dedup_single=True)
    assert dd.n_groups == 0
    counts, graphs = p.dumpCountsText(1), p.dumpGraphsText(1)
    assert counts.bytes and graphs.bytes
    dup = ka.ReadSet(p, open(GOLDEN + "/consensus3.fastq", "rb").read())
    dup_pairs = dup.identifyPairs()
    dd2 = ka.DuplicateFragmentFilter(p, dedup_mode=1).filterDuplicateFragments(dup, dup_pairs, dedup_single=True)
    assert dd2.n_groups >= 1 and dd2.consensus.n >= 2
    assert _live(probe) > base
    for x in (dd2, dup_pairs, dup, counts, graphs, dd, sel, pairs, rs, p):
        x.close()
    assert _live(probe) == base


def test_read_stage_errors_leave_nothing_behind(probe):
    """a text shorter than the one the batch was ingested from (the name-span error of each stage) and a pair list of another batch"""
    base = _live(probe)
    p, rs = _stage_spectrum(open(GOLDEN + "/consensus3.fastq", "rb").read())
    pairs = rs.identifyPairs()
    dedup = ka.DuplicateFragmentFilter(p, dedup_mode=1)
    full, rs.text = rs.text, rs.text[:10]
    _twice(probe, rs.identifyPairs)
    _twice(probe, lambda: ka.ReadSelector(p, rs, mate=pairs.mate).filterReads())
    _twice(probe, lambda: dedup.filterDuplicateFragments(rs, pairs))
    rs.text = full
    other = ka.ReadSet(p, open(GOLDEN + "/1000.fastq", "rb").read())
    _twice(probe, lambda: dedup.filterDuplicateFragments(other, pairs))        # "pair list belongs"
    for x in (other, pairs, rs, p):
        x.close()
    assert _live(probe) == base
