"""KmerMatch restated from the reference's source in the reference's own direction: KmerMatch::_matchLocal (src/KmerMatch.h:122-181),
the mates of exchangeGlobalReadIdxs (src/MatcherInterface.h:772-792), sampleMatches (:280-287) and getLocalReads (:311-321), in plain
Python.  A dict from key to the list of (global read, position) instances stands for the spectrum of TrackingDataWithAllReads
(src/KmerTrackingData.h:779-887), built from helpers.oracle_weighted_kmers and the weight test and purged by depth as purgeMinDepth
does (src/KmerSpectrum.h:1805-1815); every contig's edge k-mers are then looked up in it.  The device code
(kmernator_amd/csrc/kmr_match.hpp) joins the other way round -- a table of the contigs' keys that the reads probe -- and shares no
structure with this.  The reference's time-seeded random stream is replaced by Philox as the issue states (refnormalize.philox4x32_10).

Every rule a family of tests/matchcases.py is written for is a method, so that a test can change one and see the family notice.

A batch is a dict(first=global index of its first read, reads=[(bases, quals)], mate=[index in the batch or -1] or None,
discarded=[flags] or None)."""
import numpy as np

from helpers import oracle_weighted_kmers
from refnormalize import M32, philox4x32_10

_ACGT = frozenset(b"ACGTacgt")


class Matcher:
    def __init__(self, cfg, min_depth=2, max_positions_from_edge=500, max_read_matches=450, include_mate=True, seed=0):
        self.cfg, self.k = cfg, cfg.k
        self.min_depth, self.edge, self.max_read_matches, self.include_mate, self.seed = int(min_depth), int(max_positions_from_edge), int(max_read_matches), bool(include_mate), int(seed)

    # ---- the reference's choices
    def passes(self, w):
        """TrackingData::isDiscard: f32 |weight| > min-kmer-quality; a k-mer over a markup weighs 0"""
        return bool(np.float32(abs(w)) > np.float32(self.cfg.min_weight))

    def holds(self, instances):
        """purgeMinDepth(minDepth): at <= 1 the singleton map counts (KmerMatch.h:155-161), at 2 it is gone, above 2 the weak entries
        below the depth are gone too"""
        return len(instances) >= max(1, self.min_depth)

    def contig_keys(self, seq):
        """KmerWeights(twoBit, len, true) (KmerMatch.h:136): every window of the packed sequence, a non-ACGT base packed as A; one
        canonical key per window (None would be a window that is not looked up)"""
        packed = bytes(c if c in _ACGT else ord("A") for c in bytes(seq))
        keys, _, _ = oracle_weighted_kmers(self.cfg, packed, b"I" * len(packed))
        return [keys[i].tobytes() for i in range(keys.shape[0])]

    def max_kmers_from_edge(self):
        """int maxKmersFromEdge = maxPositionsFromEdge - KmerSizer::getSequenceLength() + 1 (:125)"""
        return self.edge - self.k + 1

    def considered(self, n):
        """:137-149: j <= (unsigned) maxKmersFromEdge || j >= upperMinKmer"""
        M = self.max_kmers_from_edge()
        lower = M & M32                                  # unsigned int lowerMaxKmer = maxKmersFromEdge
        upper = n - M if n > M else 0                    # (int) kmers.size() > maxKmersFromEdge
        return [j for j in range(n) if j <= lower or j >= upper]

    def add_hits(self, hits, instances):
        """_addResults (:114-120): mhs.insert(globalReadIdx) -- a set"""
        for read, _ in instances:
            hits[read] = 1

    def size(self, hits):
        return len(hits)

    def max_hits(self):
        return np.float32(2 * self.max_read_matches)     # float maxHits = 2 * getMaxReadMatches() (:127)

    def is_sampled(self, size):
        """:168; max_read_matches = 0 means no sampling (the option's help), not the reference's fraction of 0"""
        return self.max_read_matches != 0 and bool(np.float32(size) > self.max_hits())

    def fraction(self, size):
        return self.max_hits() / np.float32(size)        # maxHits / (float) size (:169), f32

    def uniform(self, read, contig):
        draw = philox4x32_10((read & M32, (read >> 32) & M32, contig & M32, 1), (self.seed & M32, (self.seed >> 32) & M32))[0]
        return np.float32(draw >> 8) * np.float32(2.0 ** -24)

    def keeps(self, read, contig, size):
        return bool(self.uniform(read, contig) <= self.fraction(size))      # myRand.getRand() <= fraction (MatcherInterface.h:284)

    def drops(self, read, discarded):
        return read in discarded                                            # !read.isDiscarded() (:319)

    def sample_then_mates(self, contig, hits, mate):
        """:163-171, then MatcherInterface.h:785-791 for the reads that are left: (kept reads, the set with their mates)"""
        size = self.size(hits)
        reads = sorted(hits)
        kept = [r for r in reads if self.keeps(r, contig, size)] if self.is_sampled(size) else reads
        out = set(kept)
        if self.include_mate:
            out |= set(mate[r] for r in kept if r in mate)
        return size, kept, out

    # ---- the spectrum of instances
    def instance_map(self, batches):
        """key -> [(global read, position)] of every occurrence that passes the weight test; a discarded read gives none"""
        inst = {}
        for b in batches:
            for i, (seq, qual) in enumerate(b["reads"]):
                if b.get("discarded") is not None and b["discarded"][i]:
                    continue
                keys, w, _ = oracle_weighted_kmers(self.cfg, bytes(seq), bytes(qual))
                for p in range(keys.shape[0]):
                    if self.passes(w[p]):
                        inst.setdefault(keys[p].tobytes(), []).append((b["first"] + i, p))
        return inst

    def spectrum(self, batches):
        return {key: v for key, v in self.instance_map(batches).items() if self.holds(v)}

    # ---- the match
    def match(self, contigs, batches):
        """dict(offsets, reads, size_before_sampling, size_after_sampling, n_sampled_contigs, edge_info = (contigs, considered k-mers,
        distinct keys, keys the spectrum holds))"""
        spec = self.spectrum(batches)
        mate, discarded = {}, set()
        for b in batches:
            if b.get("mate") is not None:
                mate.update({b["first"] + i: b["first"] + int(m) for i, m in enumerate(b["mate"]) if int(m) >= 0})
            if b.get("discarded") is not None:
                discarded |= set(b["first"] + i for i, d in enumerate(b["discarded"]) if d)
        offsets, reads, before, after, n_sampled = [0], [], [], [], 0
        n_edge, edge_keys = 0, set()
        for c, seq in enumerate(contigs):
            keys = self.contig_keys(seq)
            hits = {}
            for j in self.considered(len(keys)):
                if keys[j] is None:
                    continue
                n_edge += 1
                edge_keys.add(keys[j])
                if keys[j] in spec:
                    self.add_hits(hits, spec[keys[j]])
            size, kept, out = self.sample_then_mates(c, hits, mate)
            n_sampled += 1 if self.is_sampled(size) else 0
            before.append(size)
            after.append(len(kept))
            reads += [r for r in sorted(out) if not self.drops(r, discarded)]
            offsets.append(len(reads))
        return dict(offsets=np.array(offsets, dtype=np.uint64), reads=np.array(reads, dtype=np.uint64), size_before_sampling=np.array(before, dtype=np.uint64),
                    size_after_sampling=np.array(after, dtype=np.uint64), n_sampled_contigs=n_sampled,
                    edge_info=(len(contigs), n_edge, len(edge_keys), sum(1 for key in edge_keys if key in spec)))


def same_result(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("offsets", "reads", "size_before_sampling", "size_after_sampling")) and a["n_sampled_contigs"] == b["n_sampled_contigs"]
