"""selectReads' normalizing branch (--max-kmer-output-depth, RANDOM) restated on the CPU from the reference's source:
apps/FilterReads.h:168-206 (the branch and its file names), src/ReadSelector.h:661-672 (chooseRead), :673-749
(pickCoverageNormalizedSubset), :550-568 (isPassingRead, isPassingPair), :1212-1221 (optimizePickOrder), :1242-1262 (writePicks)
and src/ReadSet.h:118-123 (Pair::operator<).  The reference's random stream (one mt19937 per OpenMP thread, seeded with the time)
repeats in no run; the issue replaces it with word 0 of Philox4x32-10 over (seed, global read index), restated here in plain
integers from the algorithm's paper.  Record text comes from refpartition.record_text.  Helper of the normalization tests; nothing
here is derived from the device code.

Normalizer's small methods are the places where the reference makes a choice; the tests subclass it to see that every family of
cases notices a deviation there."""
import bisect

import numpy as np

from refpartition import SUFFIX, passes_length, record_text

M32 = 0xffffffff
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): ten rounds; in each the two 64-bit products of the multipliers with words 0 and 2
    give the new words, their high halves xored with words 1 and 3 and the key; the key moves by the Weyl constants between
    rounds.  counter: four 32-bit words, key: two; returns four words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, g):
    """the random number of global read index g: what IntRand::rand() is to chooseRead (:665)"""
    g &= 2 ** 64 - 1
    return philox4x32_10((g & M32, g >> 32, 0, 0), (seed & M32, (seed >> 32) & M32))[0]


def output_name(output, min_depth, target_depth, separate_outputs=True):
    """what selectReads hands getOFM (apps/FilterReads.h:170-181)"""
    if not separate_outputs:
        return output
    return output + "-MinDepth%d" % min_depth + "-MaxDepth%d" % target_depth      # :173, :180


def file_name(output, min_depth, target_depth, prefix, separate_outputs=True, fasta=False):
    """OfstreamMap: name + key + suffix; the key "-" + getReadFileNamePrefix(read) and the format's suffix only with
    --separate-outputs (src/ReadSelector.h:1256-1259, apps/FilterReads.h:171-176)"""
    if not separate_outputs:
        return output
    return output_name(output, min_depth, target_depth) + "-" + prefix + SUFFIX[bool(fasta)]


def pair_list(n, read1=None, read2=None):
    """the pairs the loop of :682 walks: those of the list, and a half pair (read, -1) for every read no pair names (a set
    without identified pairs holds every read as a half pair of its own)"""
    pairs = [] if read1 is None else [(int(a), int(b)) for a, b in zip(read1, read2)]
    named = set(x for p in pairs for x in p if x >= 0)
    return pairs + [(i, -1) for i in range(n) if i not in named]


class Normalizer:
    def __init__(self, target_depth, min_score, min_read_length, by_pair, both_pass, seed=0, first_read_idx=0):
        self.T, self.min_score, self.mrl = int(target_depth), np.float32(min_score), min_read_length
        self.by_pair, self.both_pass, self.seed, self.first = bool(by_pair), bool(both_pass), int(seed), int(first_read_idx)

    # ---- the reference's choices
    def score_long(self, score):
        """(long) of a float score (:685-686): truncation towards zero (saturating where the C++ cast is undefined)"""
        return max(I64_MIN, min(I64_MAX, int(np.float32(score))))

    def draw_keeps(self, choice, target):
        return choice <= target                                                    # :669, inclusive

    def both_pass_skips(self, s1, s2):
        return s1 <= 0 or s2 <= 0                                                  # :698, drops every half pair too

    def g_of_pair(self, a, b):
        return min(x for x in (a, b) if x >= 0)                                    # the issue: the pair's lower read index

    def order(self, picks):
        """optimizePickOrder: sort by Pair::lesser (src/ReadSet.h:118-123; MAX_READ_IDX for a missing side); then read1, read2
        of every pick (:1245-1250)"""
        out = []
        for a, b in sorted(picks, key=lambda p: min(x for x in p if x >= 0)):
            out += [x for x in (a, b) if x >= 0]
        return out

    # ---- the loop
    def choose(self, s, read, info):
        """chooseRead(score, targetDepth, false) (:661-672)"""
        info["n_candidates"] += 1
        if s <= self.T:
            return True
        info["n_draws"] += 1
        return self.draw_keeps(draw(self.seed, self.first + read) % s, self.T)

    def pick(self, n, pairs, passing):
        """pickCoverageNormalizedSubset (:682-734) over the pairs; passing(i) = isPassingRead; returns (picks, info), a pick
        being (read1, read2) with -1 for a side that is missing or, with by_pair off, was not chosen"""
        info = dict(n_picks=0, n_candidates=0, n_draws=0)
        picks = []
        for a, b in pairs:
            p1, p2 = a >= 0 and passing(a), b >= 0 and passing(b)
            s1 = self.score_long(self.sc[a]) if p1 else -1                         # :685
            s2 = self.score_long(self.sc[b]) if p2 else -1                         # :686
            if self.by_pair:
                ok = (p1 and p2) if (a >= 0 and b >= 0 and self.both_pass) else (p1 or p2)     # isPassingPair :558-568
                if not ok:
                    continue                                                       # :689-692
                if self.both_pass and self.both_pass_skips(s1, s2):
                    continue                                                       # :697-702
                if s1 <= 0 and s2 <= 0:
                    continue                                                       # :703-706
                if self.choose(max(s1, s2), self.g_of_pair(a, b), info):           # :707-708
                    picks.append((a, b))                                           # :710
            else:
                k1 = s1 > 0 and self.choose(s1, a, info)                           # :718
                k2 = s2 > 0 and self.choose(s2, b, info)                           # :724
                if k1 or k2:
                    picks.append((a if k1 else -1, b if k2 else -1))               # :731-732
        info["n_picks"] = len(picks)
        return picks, info

    def run(self, names, seqs, quals, labels, disc, to, tl, sc, pairs, input_starts=None, shift=0, out_base=33, fasta=False):
        """The branch over one read set.  pairs: list of (read1, read2), -1 = none (pair_list).  Returns dict(text, table,
        read_segment, info, picks): the text is the inputs' files one after the other (one round), table[input] = (first pick,
        picks, first byte, bytes) counting records, read_segment the input of every picked read or -1."""
        n = len(names)
        self.sc = np.asarray(sc, dtype=np.float32)
        lens = [len(s) for s in seqs]

        def passing(i):
            return (not disc[i]) and bool(self.sc[i] >= self.min_score) and passes_length(float(tl[i]), lens[i], self.mrl)
        picks, info = self.pick(n, pairs, passing)
        reads = self.order(picks)
        starts = [0, n] if input_starts is None else [int(x) for x in input_starts]
        n_inputs = len(starts) - 1
        read_segment = np.full(n, -1, dtype=np.int32)
        out, table, n_rec, n_bytes = [], [], 0, 0
        for f in range(n_inputs):
            mine = [i for i in reads if bisect.bisect_right(starts, i) - 1 == f] if n_inputs > 1 else reads      # writePick :1252-1262
            text = b"".join(record_text(names[i], seqs[i], quals[i], labels[i], disc[i], to[i], tl[i], shift, out_base, fasta) for i in mine)
            for i in mine:
                read_segment[i] = f
            table.append((n_rec, len(mine), n_bytes, len(text)))
            n_rec += len(mine)
            n_bytes += len(text)
            out.append(text)
        return dict(text=b"".join(out), table=table, read_segment=read_segment, info=info, picks=picks, reads=reads)
