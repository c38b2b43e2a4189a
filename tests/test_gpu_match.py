"""KmerMatch on the device (kmr_match_*; kmernator_amd/csrc/kmr_match.hpp) held to the restatement of tests/refmatch.py over the directed
contigs and reads of tests/matchcases.py.  Every figure is an integer and every comparison is for equality.  Reads go in as FASTQ text
whose names pair read 2 i with 2 i + 1, so that the mates come from kmr_identify_pairs; the spectrum is built from the same reads."""
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import matchcases as mc
from helpers import default_config
from refmatch import Matcher

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
IDS = ["%s-k%d" % (c["name"], c["k"]) for c in CASES]


# ------------------------------------------------------------------------------------------------------------------- reference side
def matcher_of(c):
    return Matcher(default_config(c["k"]), min_depth=c["min_depth"], max_positions_from_edge=c["edge"], max_read_matches=c["max_read_matches"],
                   include_mate=c["include_mate"], seed=c["seed"])


@functools.lru_cache(maxsize=None)
def want_of(i):
    c = CASES[i]
    return matcher_of(c).match(c["contigs"], mc.batches_of(c))


# ---------------------------------------------------------------------------------------------------------------------- device side
def fastq(reads, lo=0):
    return b"".join(b"@p%d/%d\n%s\n+\n%s\n" % ((lo + i) // 2, 1 + (lo + i) % 2, s, q) for i, (s, q) in enumerate(reads))


def read_set(sp, c, reads, lo=0):
    if c.get("fasta"):
        return ka.ReadSet.from_fasta(sp, b"".join(b">p%d\n%s\n" % (lo + i, s) for i, (s, _) in enumerate(reads)))
    return ka.ReadSet(sp, fastq(reads, lo), 33)


def contig_set(sp, contigs):
    return ka.ReadSet(sp, b"".join(b"@c%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(contigs)), 33)


def spectrum_of(c, **cfg):
    """the finalized spectrum of exactly the case's reads (the discarded ones give no k-mers)"""
    sp = ka.KmerSpectrum(ka.default_config(c["k"], device=0, estimated_raw_kmers=max(4096, sum(len(s) for s, _ in c["reads"])), **cfg))
    with read_set(sp, c, c["reads"]) as rs:
        assert rs.n == len(c["reads"])
        b, q, o, _ = rs.arrays()
        sp.buildKmerSpectrum(np.append(b, np.uint8(0)), np.append(q, np.uint8(0)), o, discarded=np.array(c["discarded"], dtype=np.uint8))
    sp.finalize(c["min_depth"])
    return sp


def device_match(sp, c, cuts=(), contigs=None):
    contigs = c["contigs"] if contigs is None else contigs
    with contig_set(sp, contigs) as cs, ka.KmerMatch(sp, cs, c["edge"], c["max_read_matches"], c["include_mate"], c["seed"]) as km:
        assert cs.n == len(contigs)
        for b in mc.batches_of(c, cuts):
            with read_set(sp, c, b["reads"], b["lo"]) as rs:
                pairs = rs.identifyPairs() if c["paired"] else None
                try:
                    if pairs is not None:
                        assert np.array_equal(pairs.mate, np.array(b["mate"], dtype=np.int64))
                    km.addReads(rs, b["first"], pairs, np.array(b["discarded"], dtype=np.uint8))
                finally:
                    if pairs is not None:
                        pairs.close()
        res = km.finish()
        return res, (km.n_contigs, km.n_edge_kmers, km.n_distinct_keys, km.n_keys_in_spectrum)


def same(got, want):
    for f in ("offsets", "reads", "size_before_sampling", "size_after_sampling"):
        g, w = getattr(got, f), want[f]
        assert g.dtype == np.uint64 and np.array_equal(g, w), (f, g[:16], w[:16])
    assert got.n_sampled_contigs == want["n_sampled_contigs"]
    assert len(got) == len(want["offsets"]) - 1
    for i in range(len(got)):
        assert np.array_equal(got[i], want["reads"][int(want["offsets"][i]):int(want["offsets"][i + 1])])


# ----------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_families_equal_the_restatement(i):
    """from one batch and from the cut batches; edge_info equals the restatement's counts"""
    c = CASES[i]
    want = want_of(i)
    sp = spectrum_of(c)
    try:
        got, info = device_match(sp, c)
        same(got, want)
        assert info == want["edge_info"]
        for cuts in mc.cut_layouts(c)[:2] if len(c["reads"]) <= 100 else mc.cut_layouts(c)[1:2]:
            same(device_match(sp, c, cuts)[0], want)
    finally:
        sp.close()


@pytest.mark.parametrize("variant", [dict(separate_singletons=0), dict(value_kind=ka.KMR_VALUE_EXT), dict(num_buckets_weak=64, num_buckets_singleton=16)],
                         ids=["one_map", "ext_values", "few_buckets"])
@pytest.mark.parametrize("min_depth", [1, 2])
def test_spectrum_variants(variant, min_depth):
    """the key filter reads whatever maps the handle keeps"""
    c = mc.mixed(22, min_depth=min_depth)
    sp = spectrum_of(c, **variant)
    try:
        same(device_match(sp, c)[0], matcher_of(c).match(c["contigs"], mc.batches_of(c)))
    finally:
        sp.close()


@pytest.mark.parametrize("cap", [1, 7, 50])
def test_hit_buffers_grow(cap):
    """a capacity so low that the first attempt overflows: in the first batch, and in a later one that must keep the earlier records"""
    c = mc.many(21, 71, max_read_matches=35)
    want = matcher_of(c).match(c["contigs"], mc.batches_of(c))
    sp = spectrum_of(c)
    try:
        sp.tune(match_hit_capacity=cap)
        got, _ = device_match(sp, c)
        assert sp.build_info("match_add_attempts") == 2
        same(got, want)
        same(device_match(sp, c, (20, 60))[0], want)
        sp.tune(match_hit_capacity=0)
        same(device_match(sp, c)[0], want)
        assert sp.build_info("match_add_attempts") == 1
    finally:
        sp.close()


def test_refusals():
    c = mc.mixed(21)
    sp = spectrum_of(c)
    raw = ka.KmerSpectrum(ka.default_config(21, device=0, estimated_raw_kmers=4096))
    try:
        with contig_set(sp, c["contigs"]) as cs, ka.ReadSet(sp, fastq(c["reads"]), 33) as rs:
            with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
                ka.KmerMatch(raw, cs)                                            # not finalized
            for part in (dict(world_size=2, rank=1), dict(num_parts=2, part_idx=1), dict(kmer_subsample=3)):
                p = spectrum_of(c, **part)
                try:
                    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_UNSUPPORTED"):
                        ka.KmerMatch(p, cs)                                      # a part of a spectrum
                finally:
                    p.close()
            with ka.KmerMatch(sp, cs, c["edge"]) as km:
                with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
                    sp._call("match_copy", km._m, None, None, None, None)       # copy before finish
                with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
                    sp._call("match_info", km._m, None, None, None)
                with ka.ReadSet(sp, fastq(c["reads"][:4]), 33) as few, few.identifyPairs() as foreign:
                    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
                        km.addReads(rs, 0, foreign)                              # the pairing of another batch
                with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_UNSUPPORTED"):
                    km.addReads(rs, 1 << 40)                                     # beyond the packed record's read bits
                km.addReads(rs, 0, None, c["discarded"])
                km.finish()
                with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
                    km.addReads(rs, 0)                                           # add after finish
                with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
                    km.finish()
    finally:
        sp.close()
        raw.close()


def test_empty_inputs_are_valid():
    c = mc.mixed(21)
    sp = spectrum_of(c)
    try:
        # no contigs
        got, info = device_match(sp, c, contigs=[])
        assert len(got) == 0 and got.offsets.tolist() == [0] and got.reads.size == 0 and info == (0, 0, 0, 0)
        # contigs shorter than k only
        got, info = device_match(sp, c, contigs=[b"ACGT", b"A" * 20])
        assert len(got) == 2 and got.offsets.tolist() == [0, 0, 0] and info == (2, 0, 0, 0)
        # zero hits: foreign contigs
        foreign = [mc.R(60, 901), mc.R(45, 902)]
        got, info = device_match(sp, c, contigs=foreign)
        assert got.offsets.tolist() == [0, 0, 0] and got.size_before_sampling.tolist() == [0, 0] and info[2] > 0 and info[3] == 0
        # no batch at all, and an empty batch
        with contig_set(sp, c["contigs"]) as cs:
            with ka.KmerMatch(sp, cs, c["edge"]) as km:
                res = km.finish()
                assert len(res) == len(c["contigs"]) and res.reads.size == 0 and not res.offsets.any()
            with ka.KmerMatch(sp, cs, c["edge"]) as km, ka.ReadSet(sp, b"", 33) as empty:
                km.addReads(empty, 5)
                res = km.finish()
                assert res.reads.size == 0 and res.n_sampled_contigs == 0
                assert all(p != 0 for p in km.device_ptrs())
    finally:
        sp.close()
