"""CompareSpectrums restated from the reference's source (apps/CompareSpectrums.cpp; ReadSet::circularize, src/ReadSet.cpp:120-130),
in plain Python over dicts: what the device code of kmernator_amd/csrc/kmr_compare.hpp is held to.

A map is {canonical key bytes: count}.  A read's map comes from helpers.oracle_weighted_kmers (the reference's buildWeightedKmers)
and the weight test of TrackingData::isDiscard; a set's map from OracleSpectrum.entries().  Every rule a family of
tests/comparecases.py is written for is a method, so that a test can change one and see the family notice."""
import numpy as np

from helpers import OracleSpectrum, ReadBatch, default_config, oracle_weighted_kmers

FIELDS = ("size1", "size2", "common", "common_count1", "common_count2", "total_count1", "total_count2", "saturated")
HEADER = b"\nSet 1\tSet 2\tCommon\t%Uniq1\t%Tot1\t%Uniq2\t%Tot2\n"      # :211-212


def percent(num, den):
    """os << setprecision(4) << num * 100.0 / den: %.4g; 0.0 / 0.0 prints as -nan from an x86-64 glibc build"""
    if den == 0:
        return b"-nan"
    return ("%.4g" % (num * 100.0 / den)).encode()


def line(rec, label=b""):
    """:235-240"""
    return b"\t".join([str(int(rec["size1"])).encode(), str(int(rec["size2"])).encode(), str(int(rec["common"])).encode(),
                       percent(int(rec["common"]), int(rec["size1"])), percent(int(rec["common_count1"]), int(rec["total_count1"])),
                       percent(int(rec["common"]), int(rec["size2"])), percent(int(rec["common_count2"]), int(rec["total_count2"])), bytes(label)]) + b"\n"


def count_common_kmers(m1, m2):
    """:146-162: (common, count1 of the common keys, count2 of them, all of count1, all of count2)"""
    ret = [0, 0, 0, 0, 0]
    for key, c in m1.items():
        ret[3] += c
        if key in m2:
            ret[0] += 1
            ret[1] += c
            ret[2] += m2[key]
    for c in m2.values():
        ret[4] += c
    return ret


def evaluate(m1, m2):
    """:225-242 as a record"""
    c = count_common_kmers(m1, m2)
    return dict(size1=len(m1), size2=len(m2), common=c[0], common_count1=c[1], common_count2=c[2], total_count1=c[3], total_count2=c[4], saturated=0)


class Comparer:
    """the rules of a read's map (TrackingDataMinimal4 in a solid-only spectrum, src/KmerTrackingData.h:1132-1212)"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.k = cfg.k

    def passes(self, w):
        """TrackingData::isDiscard: f32 |weight| > min-kmer-quality; a k-mer over a markup weighs 0"""
        return bool(np.float32(abs(w)) > np.float32(self.cfg.min_weight))

    def key(self, canonical, forward_text):
        return canonical

    def add(self, m, key):
        m[key] = m.get(key, 0) + 1

    def circular_extra(self):
        """CompareSpectrums passes the k-mer length itself (:191-192), not k - 1"""
        return self.k

    def read_map(self, seq, qual):
        keys, w, _ = oracle_weighted_kmers(self.cfg, bytes(seq), bytes(qual))
        m = {}
        for i in range(keys.shape[0]):
            if self.passes(w[i]):
                self.add(m, self.key(keys[i].tobytes(), bytes(seq[i:i + self.k])))
        return m

    def set_map(self, reads):
        """the solid map of (seq, qual) reads, as the sum of their maps"""
        m = {}
        for seq, qual in reads:
            for key, c in self.read_map(seq, qual).items():
                m[key] = m.get(key, 0) + c
        return m

    def per_read(self, reads, m2):
        """evaluatePerRead :243-257"""
        return [evaluate(self.read_map(seq, qual), m2) for seq, qual in reads]

    def circularize(self, reads, extra=None):
        """ReadSet::circularize: bases + bases[0 : min(extra, L)], the qualities alike"""
        extra = self.circular_extra() if extra is None else extra
        return [(seq + seq[:min(extra, len(seq))], qual + qual[:min(extra, len(seq))]) for seq, qual in reads]


def oracle_set_map(cfg, reads, min_depth=1):
    """the same solid map by another route: the oracle's spectrum (no singleton split) and its entries"""
    c = default_config(cfg.k, min_weight=cfg.min_weight, min_quality_score=cfg.min_quality_score, fastq_start_char=cfg.fastq_start_char,
                       separate_singletons=0, estimated_raw_kmers=max(1024, sum(len(s) for s, _ in reads)))
    o = OracleSpectrum(c)
    if reads:
        o.add_reads(ReadBatch([bytes(s) for s, _ in reads], [bytes(q) for _, q in reads]))
    o.finalize(min_depth)
    keys, count, _, _, _ = o.entries()
    m = {keys[i].tobytes(): int(count[i]) for i in range(keys.shape[0])}
    o.close()
    return m


def records_array(recs):
    """a list of records as the structured array KmerSpectrum.compareReads answers with"""
    out = np.zeros(len(recs), dtype=np.dtype([(n, np.uint64) for n in FIELDS]))
    for i, r in enumerate(recs):
        for n in FIELDS:
            out[i][n] = r[n]
    return out
