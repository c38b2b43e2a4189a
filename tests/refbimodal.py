"""Pure-Python restatement of the bimodal cut of ReadSelector::trimReadByMinimumKmerScore (src/ReadSelector.h:981-1008) with
Statistics::MeanStdCount and Statistics::findBimodalPartition (src/Utils.h:1000-1056), written from the reference's source text.
Python floats are IEEE doubles, every operation is rounded on its own (nothing is contracted to a fused multiply-add) and
math.sqrt is correctly rounded, so this is the bit-level reference of the device pass.  Test infrastructure only.

One point is decided by the toolchain rather than by the source text: `abs(first.mean - second.mean)` (src/Utils.h:1043) is an
unqualified call on a double with <cstdlib> and <cmath> included and no using-directive in scope, which resolves to C's
int abs(int): the difference is truncated toward zero to an int before it is compared.  That reading is the contract.

DEVIANTS are readings a port could take by mistake; each changes the result of some read (tests/test_bimodal_cases.py shows
which), so a device that took one would be told apart:
  float_abs     fabs instead of the int abs
  last_tie      `diff >= bestDiff`: the last of equal diffs instead of the first
  no_floor      no Poisson floor under the variance
  rooted        a real standard deviation (the reference's "stdDev" is the variance, never rooted)
  closed_form   the variance from sum(x) and sum(x^2) instead of the pass over (x - mean)^2"""
import math

import numpy as np

from refsemantics import score_and_trim

DEVIANTS = ("float_abs", "last_tie", "no_floor", "rooted", "closed_form")
SCORE_LABEL = {"SUM": b"Score", "MEDIAN": b"MedianScore", "MIN": b"MinScore", "MAX": b"MaxScore", "AVG": b"AvgScore"}


def mean_std_count(vals, deviant=None):
    """MeanStdCount(begin, end, isPoisson = true) (:1008-1028): (mean, "stdDev", count)"""
    count, mean, std = 0, 0.0, 0.0
    for x in vals:
        count += 1
        mean += float(x)
    if count > 1:
        mean /= float(count)
        if deviant == "closed_form":
            sq = 0.0
            for x in vals:
                sq += float(x) * float(x)
            std = (sq - float(count) * mean * mean) / float(count - 1)
        else:
            for x in vals:
                d = float(x) - mean
                std += d * d
            std /= float(count - 1)
        if deviant == "rooted":
            std = math.sqrt(std) if std > 0.0 else 0.0
    if deviant != "no_floor" and mean > 0.0:
        poisson = math.sqrt(mean)
        if std < poisson:
            std = poisson
    return mean, std, count


def split_diff(m1, m2, deviant=None):
    """abs(first.mean - second.mean): int abs(int), the double truncated toward zero on the way in"""
    if deviant == "float_abs":
        return abs(m1 - m2)
    return float(abs(int(m1 - m2)))


FAST_ABOVE = 200      # runs longer than this take find_partition_fast (the plain loops are quadratic in Python)


def _msc_fast(x):
    """mean_std_count of a float64 array with the same roundings in the same order: np.cumsum is a running sum, one addition per
    element in index order (np.sum is pairwise and is not used)"""
    count = x.size
    mean = float(np.cumsum(x)[-1])
    std = 0.0
    if count > 1:
        mean /= float(count)
        d = x - mean
        std = float(np.cumsum(d * d)[-1]) / float(count - 1)
    if mean > 0.0:
        poisson = math.sqrt(mean)
        if std < poisson:
            std = poisson
    return mean, std, count


def find_partition_fast(vals, sigmas):
    """find_partition with numpy running sums in place of the Python loops; tests/test_bimodal_cases.py holds the two equal"""
    x = np.asarray(vals, dtype=np.float64)
    best, best_diff = None, 0.0
    for p in range(1, x.size):
        first, second = _msc_fast(x[:p]), _msc_fast(x[p:])
        diff = split_diff(first[0], second[0])
        if diff > sigmas * max(first[1], second[1]) and diff > best_diff:
            best_diff, best = diff, (p, first, second)
    return best


_found = {}


def find_partition(vals, sigmas, deviant=None):
    """findBimodalPartition (:1031-1056): (p, first, second) of the winning split, or None; first / second = mean_std_count.
    Answers are remembered by (values, sigmas, deviant): the tests ask for the same run under every k and scoring type."""
    key = (tuple(vals), float(sigmas), deviant)
    if key not in _found:
        _found[key] = find_partition_fast(vals, sigmas) if deviant is None and len(vals) > FAST_ABOVE else find_partition_plain(vals, sigmas, deviant)
    return _found[key]


def find_partition_plain(vals, sigmas, deviant=None):
    """the reference's loop, line by line"""
    n = len(vals)
    best, best_diff = None, 0.0
    for p in range(1, n):
        first, second = mean_std_count(vals[:p], deviant), mean_std_count(vals[p:], deviant)
        if first[2] == 1 and second[2] == 1:
            continue
        diff = split_diff(first[0], second[0], deviant)
        if diff > sigmas * max(first[1], second[1]):
            if diff > best_diff or (deviant == "last_tie" and best is not None and diff >= best_diff):
                best_diff, best = diff, (p, first, second)
    return best


def threshold(vals, p):
    """diff / max(stdDev) of the split at p, as (diff, the larger "stdDev", which side holds it and whether that is its floor)"""
    first, second = mean_std_count(vals[:p]), mean_std_count(vals[p:])
    raw1, raw2 = mean_std_count(vals[:p], "no_floor"), mean_std_count(vals[p:], "no_floor")
    sd = max(first[1], second[1])
    side = 0 if first[1] >= second[1] else 1
    floored = (first[1], second[1])[side] != (raw1[1], raw2[1])[side]
    return split_diff(first[0], second[0]), sd, side, floored


def word_of(p, k, m1, m2):
    """what the device keeps of a cut: p + k in bits 0-31, (int)first.mean in 32-47, (int)second.mean in 48-63"""
    return (p + k) | (int(m1) << 32) | (int(m2) << 48)


def tag_of(word):
    """"Bimodal@<p + k>:<(int)first.mean>/<(int)second.mean>" (:987-989), "Inv" in front where the head went (:1005); b"" for 0"""
    if not word:
        return b""
    m1, m2 = (word >> 32) & 0xffff, word >> 48
    return (b"Inv" if m1 < m2 else b"") + b"Bimodal@%d:%d/%d" % (word & 0xffffffff, m1, m2)


def score_and_trim_bimodal(counts, seq, k, min_score, scoring, sigmas, deviant=None):
    """scoreAndTrimReads for one read with --bimodal-sigmas: (trim_offset, trim_length_in_bases, score, was_trimmed, word).
    The run is the one score_and_trim selects; with sigmas >= 0 and a run of >= 3 k-mers the split is searched, a found split
    keeps the side of the larger mean (:991-1006), was_trimmed = trimLength < numKmers holds after any cut (:1012), and the run
    that is left is scored (scoreReadByKmers :1056-1057)."""
    toff, tlen, sc, trimmed = score_and_trim(counts, seq, k, min_score, scoring)
    n = tlen - k + 1 if tlen else 0
    if n < 3 or not sigmas >= 0.0:
        return toff, tlen, sc, trimmed, 0
    vals = [float(c) for c in counts[toff:toff + n]]
    found = find_partition(vals, sigmas, deviant)
    if found is None:
        return toff, tlen, sc, trimmed, 0
    p, first, second = found
    if first[0] > second[0]:
        off, ln = toff, p
    else:
        off, ln = toff + p, n - p
    # the score of the reduced run: score_and_trim over it alone (no markup, everything passes a minimum of 0)
    sc = score_and_trim([int(v) for v in counts[off:off + ln]], b"", k, 0, scoring)[2]
    return off, ln + k - 1, sc, True, word_of(p, k, first[0], second[0])


def label_of(scoring, toff, tlen, score, trimmed, word=0, aftrim=None):
    """the label of a scored read as it is printed: [AFTrim:<lo>+<hi - lo>] [Bimodal@..|InvBimodal@..] [Trim:<o>+<l>] <Label>:<score>
    (the artifact filter's part first, then what trimReadByMinimumKmerScore left in trim.label, then setTrimHeaders :1015-1035)"""
    parts = []
    if aftrim is not None:
        parts.append(b"AFTrim:%d+%d" % (aftrim[0], aftrim[1] - aftrim[0]))
    if word:
        parts.append(tag_of(word))
    if trimmed:
        parts.append(b"Trim:%d+%d" % (toff, tlen))
    parts.append(SCORE_LABEL[scoring] + b":%d" % int(float(score) + 0.5))
    return b" ".join(parts)


def reference_of_counts(counts, seqs, k, min_score, scoring, sigmas, deviant=None):
    """score_and_trim_bimodal over per-read counts and sequences, as (trim_offset u32, trim_length u32, score f32, was_trimmed bool,
    words u64)"""
    res = [score_and_trim_bimodal(counts[i], seqs[i], k, min_score, scoring, sigmas, deviant) for i in range(len(seqs))]
    return (np.array([x[0] for x in res], np.uint32), np.array([x[1] for x in res], np.uint32), np.array([x[2] for x in res], np.float32),
            np.array([x[3] for x in res], bool), np.array([x[4] for x in res], np.uint64))
