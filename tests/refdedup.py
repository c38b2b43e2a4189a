"""A plain sequential restatement of one DuplicateFragmentFilter::_filterDuplicateFragments (src/DuplicateFragmentFilter.h:505-559)
with edit distance 0, consensus on and cutoff 2, as a single thread runs it, and of what it calls: ReadSet::getConsensusRead
(src/ReadSet.cpp:572-629), Read::getProbabilityBases (src/Sequence.cpp:563-582), ProbabilityBase / BaseQual (src/Sequence.h:293-338,
src/Sequence.cpp:807-967).  Strings, a dict and Python floats (IEEE doubles), math.log10 where the reference calls log10.  The oracle of
the duplicate-fragment tests, with the cases worked by hand and the seeded generator both the CPU and the GPU tests use.

A read is (name line without '@', bases, qualities), all str; a pair list is refpairs.identify_pairs(...).pairs."""
import math

import numpy as np

import refpairs

NONE = refpairs.NONE
PRINT_REF_QUAL = 103          # src/Sequence.h: qualities from here on mean "no quality data"

# ---- named deviations: every function below takes `deviation` (None, a name or a set of names); each name switches one rule of the
# restatement to a plausible wrong one, so that tests/test_dedup_cases.py can prove that the directed cases of tests/dedupcases.py
# notice it.  Without a deviation nothing below changes.
DEVIATIONS = (
    "key_window_shifted",                # the window starts a base late
    "x_before_window_ignored",           # an X in front of start_offset does not make the read too short
    "n_is_its_own_code",                 # N does not pack as A
    "last_key_word_ignored",             # the last 64-bit word of the key takes no part in the grouping
    "canonical_first_word_only",         # mode 2 compares only the first 64-bit word of the forward and the reverse key
    "canonical_tie_takes_reverse",       # a key equal to its reverse complement counts as flipped
    "members_not_in_pair_order",         # a group's members in descending pair position
    "flip_sides_not_swapped",            # a flipped member still gives read 1 to side 1
    "name_of_unflipped_first_read",      # the consensus is named after read 1 (side 1) / read 2 (side 2) of a flipped first member
    "low_quality_skips",                 # getProbabilityBases goes on behind a quality below the minimum
    "no_floor",                          # no 0.2501 floor
    "ref_qual_not_one",                  # qualities from 103 upward follow the formula
    "count_is_int",                      # the member count does not wrap as a short
    "copy_does_not_raise_top",           # the copy inside operator+ leaves `top` alone
    "set_top_not_strict",                # setTop with <=
    "tree_not_strict",                   # getBaseQual's tree with >=
    "get_ignores_best",                  # getA .. getT answer `top` whatever `best` names
    "qual_rounds",                       # probToQual rounds
    "forty_from_0_9999_off",             # getQualChar's shortcut to 40 only from 1.0
    "name_cut_at_blank_only",            # a tab stays in the printed name
    "count_digits_fixed",                # the member count printed as three digits
    "groups_in_key_order",               # groups come out in key order, not by first member
    "cutoff_three",                      # a group needs three members
    "pair_short_counted_twice",          # a pair with both ends too short counts twice
)
# Deviations that cannot change any output and are therefore not listed:
#  - `self.top < x * self.count` with <= in getA .. getT: equality needs top == x * count.  top is at most the largest single sum
#    the position has held, so equality needs count == 1 (or all sums 0, where top == x == 0), and there both branches answer x.
#  - testing the flags as the pass goes instead of the flags handed in: a read stands in one pair record only, so no record can
#    see a flag that an earlier record of the same pass set; and the flags are only set behind the loop over the pair list.
#  - the order of the discard test and the too-short test is observable (P family, one count), the order of the two too-short
#    tests of a pair is not: either way the pair counts once.


def _dev(deviation):
    if deviation is None:
        return frozenset()
    d = frozenset([deviation]) if isinstance(deviation, str) else frozenset(deviation)
    assert d <= set(DEVIATIONS), d - set(DEVIATIONS)
    return d


def quality_to_probability(min_quality, start_char, deviation=None):
    """Read::initializeQualityToProbability (src/Sequence.cpp:522-540)"""
    t = [0.0] * 256
    for i in range(start_char + min_quality, PRINT_REF_QUAL):
        t[i] = 1.0 - math.pow(10.0, (start_char - i) / 10.0)
    for i in range(PRINT_REF_QUAL, 256):
        t[i] = 1.0 - math.pow(10.0, (start_char - i) / 10.0) if "ref_qual_not_one" in _dev(deviation) and i >= start_char + min_quality else 1.0
    return t


def prob_to_qual(prob, deviation=None):
    """probToQual (src/Sequence.cpp:807-809): (char) truncates toward zero"""
    if "qual_rounds" in _dev(deviation):
        return int(round(-10. * math.log10(1.0 - prob)))
    return int(-10. * math.log10(1.0 - prob))


def get_qual_char(prob, start_char=33, deviation=None):
    """BaseQual::getQualChar(prob, ignoreLow = false) (src/Sequence.cpp:811-819) as a character code"""
    if prob >= (1.0 if "forty_from_0_9999_off" in _dev(deviation) else 0.9999):
        return start_char + 40
    return start_char + prob_to_qual(prob, deviation)


class ProbabilityBase:
    """src/Sequence.h:304-338"""

    def __init__(self, dev=frozenset()):
        self.a = self.c = self.g = self.t = 0.0
        self.top = 0.0
        self.best = " "
        self.count = 0
        self.dev = dev

    def copy(self):
        """the copy constructor (src/Sequence.h:313-315): the fields, then setTop(*this)"""
        o = ProbabilityBase(self.dev)
        o.a, o.c, o.g, o.t, o.top, o.best, o.count = self.a, self.c, self.g, self.t, self.top, self.best, self.count
        if "copy_does_not_raise_top" not in self.dev:
            o.set_top(o.a, o.c, o.g, o.t)
        return o

    def observe(self, nuc, prob):
        """src/Sequence.cpp:870-884"""
        other = (1.0 - prob) / 3.0
        if nuc in "Aa":
            self.a += prob; self.c += other; self.g += other; self.t += other
        elif nuc in "Cc":
            self.c += prob; self.a += other; self.g += other; self.t += other
        elif nuc in "Gg":
            self.g += prob; self.a += other; self.c += other; self.t += other
        elif nuc in "Tt":
            self.t += prob; self.a += other; self.c += other; self.g += other
        self.count += 1

    def set_top(self, a, c, g, t):
        """src/Sequence.cpp:886-903"""
        if "set_top_not_strict" in self.dev:
            for x, name in ((a, "A"), (c, "C"), (g, "G"), (t, "T")):
                if self.top <= x:
                    self.top, self.best = x, name
            return
        if self.top < a:
            self.top, self.best = a, "A"
        if self.top < c:
            self.top, self.best = c, "C"
        if self.top < g:
            self.top, self.best = g, "G"
        if self.top < t:
            self.top, self.best = t, "T"

    def plus(self, other):
        """operator+ (src/Sequence.cpp:833-842); operator+= assigns its result field by field (:843-847, :823-832)"""
        tmp = self.copy()
        tmp.a += other.a; tmp.c += other.c; tmp.g += other.g; tmp.t += other.t
        tmp.count = tmp.count + other.count
        if "count_is_int" not in self.dev:
            tmp.count = ((tmp.count + 32768) % 65536) - 32768          # a short
        tmp.set_top(other.a, other.c, other.g, other.t)
        return tmp

    def _get(self, base, x):
        """getA .. getT (src/Sequence.cpp:905-928)"""
        if (self.best == base or "get_ignores_best" in self.dev) and self.top < x * self.count:
            return self.top
        return x

    def get_base_qual(self):
        """getBaseQual (src/Sequence.cpp:930-965): (base, the value handed to getQualChar)"""
        a, c, g, t = self.a, self.c, self.g, self.t
        if "tree_not_strict" in self.dev:
            if a >= c:
                if a >= g:
                    return ("A", self._get("A", a)) if a >= t else ("T", self._get("T", t))
                return ("G", self._get("G", g)) if g >= t else ("T", self._get("T", t))
            if c >= g:
                return ("C", self._get("C", c)) if c >= t else ("T", self._get("T", t))
            return ("G", self._get("G", g)) if g >= t else ("T", self._get("T", t))
        if a > c:
            if a > g:
                return ("A", self._get("A", a)) if a > t else ("T", self._get("T", t))
            return ("G", self._get("G", g)) if g > t else ("T", self._get("T", t))
        if c > g:
            return ("C", self._get("C", c)) if c > t else ("T", self._get("T", t))
        return ("G", self._get("G", g)) if g > t else ("T", self._get("T", t))


def read_probability_bases(bases, quals, min_quality, start_char, table, deviation=None):
    """Read::getProbabilityBases (src/Sequence.cpp:563-582)"""
    dev = _dev(deviation)
    probs = [ProbabilityBase(dev) for _ in bases]
    for i, nuc in enumerate(bases):
        q = ord(quals[i])
        if q < min_quality + start_char:
            if "low_quality_skips" in dev:
                continue
            break
        prob = table[q]
        if prob < 0.2501 and "no_floor" not in dev:
            prob = 0.2501
        probs[i].observe(nuc, prob)
    return probs


def consensus_read(reads, min_quality, start_char=33, table=None, deviation=None, name_from=None):
    """ReadSet::getConsensusRead(minQual) (src/ReadSet.cpp:599-629) over ReadSet::getProbabilityBases (:572-579) and
    ProbabilityBases::operator+= (src/Sequence.cpp:986-995): (name, bases, qualities)"""
    dev = _dev(deviation)
    if table is None:
        table = quality_to_probability(min_quality, start_char, dev)
    probs = []
    for _, bases, quals in reads:
        other = read_probability_bases(bases, quals, min_quality, start_char, table, dev)
        while len(probs) < len(other):
            probs.append(ProbabilityBase(dev))
        for i in range(len(other)):
            probs[i] = probs[i].plus(other[i])
    count = "%03d" % (len(reads) % 1000) if "count_digits_fixed" in dev else "%d" % len(reads)
    name = "C%s-%s" % (count, read_name((reads[0] if name_from is None else name_from)[0], dev))
    out_b, out_q = [], []
    for p in probs:
        base, value = p.get_base_qual()
        out_b.append(base)
        out_q.append(chr(get_qual_char(value, start_char, dev)))
    return name, "".join(out_b), "".join(out_q)


def read_name(name_line, deviation=None):
    """what is printed of a name: up to the first blank or tab (the span kmr_select_reads prints; the Casava rewrite is not covered)"""
    stops = " " if "name_cut_at_blank_only" in _dev(deviation) else " \t"
    for i, ch in enumerate(name_line):
        if ch in stops:
            return name_line[:i]
    return name_line


def first_markup_x_length(bases):
    """Sequence::getFirstMarkupXLength (src/Sequence.cpp:432-439)"""
    for i, ch in enumerate(bases):
        if ch in "Xx":
            return i
    return len(bases)


_CODE = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}


def two_bit(bases):
    """TwoBitSequence::compressSequence (src/TwoBitSequence.cpp:242-269) as a list of codes: anything but ACGT packs as 0"""
    return [_CODE.get(ch, 0) for ch in bases]


def reverse_complement(codes):
    return [3 - v for v in reversed(codes)]


def key_bytes(codes):
    """the bytes memcmp sees (four bases a byte, the first in the high bits); len(codes) is a multiple of 4"""
    return bytes((codes[i] << 6) | (codes[i + 1] << 4) | (codes[i + 2] << 2) | codes[i + 3] for i in range(0, len(codes), 4))


class Result:
    def __init__(self, n):
        self.discarded = [0] * n
        self.skipped = [0, 0, 0, 0]          # discard, too short, unpaired, invalid
        self.affected = 0
        self.groups = []                     # (pair position of the first member, members), ascending first member
        self.consensus = []                  # (name, bases, quals); two per group in the paired pass
        self.flipped = 0

    def discarded_array(self):
        return np.array(self.discarded, dtype=np.uint8)

    def group_array(self):
        return np.array(self.groups, dtype=np.int64).reshape(-1, 2)


def _window_key(bases, start_offset, need, dev):
    """the 2-bit codes of the window [start_offset, need) of one read"""
    if "key_window_shifted" in dev:
        w = (bases + "A")[start_offset + 1:need + 1]
    else:
        w = bases[start_offset:need]
    if "n_is_its_own_code" in dev:
        return [4 if ch in "Nn" else c for ch, c in zip(w, two_bit(w))]
    return two_bit(w)


def _rc(codes):
    return [3 - v if v < 4 else v for v in reversed(codes)]


def _key(codes, dev):
    """key_bytes; with n_is_its_own_code a code does not fit two bits: one byte per base, which compares in the same order"""
    return bytes(codes) if "n_is_its_own_code" in dev else key_bytes(codes)


def _too_short(bases, start_offset, need, dev):
    if "x_before_window_ignored" in dev:
        return len(bases) < need or first_markup_x_length(bases[start_offset:]) < need - start_offset
    return first_markup_x_length(bases) < need


def filter_duplicate_fragments(reads, pairs, discarded=None, dedup_mode=1, paired=True, dedup_length=24, start_offset=0, min_quality=3, start_char=33, deviation=None):
    """_buildDuplicateFragmentMap (:172-292) with one thread, then _buildConsensusPairedReads (:420-503) or
    _buildConsensusUnPairedReads (:361-418); groups in ascending position of their first member"""
    dev = _dev(deviation)
    n = len(reads)
    res = Result(n)
    if discarded is not None:
        res.discarded = [1 if d else 0 for d in discarded]
    before = list(res.discarded)
    length = dedup_length if paired else 2 * dedup_length          # :188-190
    need = length + start_offset
    table = quality_to_probability(min_quality, start_char, dev)
    per_base = 1 if "n_is_its_own_code" in dev else 4              # bases a key byte holds
    word = 8 * 4 // per_base                                       # key bytes of one 64-bit word

    def grouping(key):
        if "last_key_word_ignored" in dev:
            return key[:(len(key) - 1) // word * word]
        return key
    groups = {}                                                    # key -> [(pair position, flipped)], in the order met
    for pos, (r1, r2) in enumerate(pairs):
        if paired and r1 != NONE and r2 != NONE:
            if not (r1 < n and r2 < n):
                res.skipped[3] += 1
                continue
            if before[r1] or before[r2]:
                res.skipped[0] += 1
                continue
            s1, s2 = _too_short(reads[r1][1], start_offset, need, dev), _too_short(reads[r2][1], start_offset, need, dev)
            if s1 or s2:
                res.skipped[1] += 2 if (s1 and s2 and "pair_short_counted_twice" in dev) else 1
                continue
            fwd = _window_key(reads[r1][1], start_offset, need, dev) + _rc(_window_key(reads[r2][1], start_offset, need, dev))
            key, flipped = _key(fwd, dev), False
            if dedup_mode == 2:
                rev = _key(_rc(fwd), dev)
                if "canonical_first_word_only" in dev:
                    least = key[:word] <= rev[:word]
                elif "canonical_tie_takes_reverse" in dev:
                    least = key < rev
                else:
                    least = key <= rev                             # Kmer::buildLeastComplement (src/Kmer.h:356-364)
                if not least:
                    key, flipped = rev, True
            groups.setdefault(grouping(key), []).append((pos, flipped))
        elif (not paired) and (r1 != NONE) != (r2 != NONE):
            rid = r1 if r1 != NONE else r2
            if not rid < n:
                res.skipped[3] += 1
                continue
            if before[rid]:
                res.skipped[0] += 1
                continue
            if _too_short(reads[rid][1], start_offset, need, dev):
                res.skipped[1] += 1
                continue
            groups.setdefault(grouping(_key(_window_key(reads[rid][1], start_offset, need, dev), dev)), []).append((pos, False))
        else:
            res.skipped[2] += 1
    order = sorted(groups) if "groups_in_key_order" in dev else list(groups)
    for key in order:
        members = groups[key]
        if len(members) < (3 if "cutoff_three" in dev else 2):
            continue
        if "members_not_in_pair_order" in dev:
            members = members[::-1]
        res.groups.append((members[0][0], len(members)))
        if paired:
            side1, side2 = [], []
            for pos, flipped in members:
                r1, r2 = pairs[pos]
                if flipped:
                    res.flipped += 1
                    if "flip_sides_not_swapped" not in dev:
                        r1, r2 = r2, r1
                side1.append(reads[r1]); side2.append(reads[r2])
            named = (None, None)
            if "name_of_unflipped_first_read" in dev:
                named = tuple(reads[r] for r in pairs[members[0][0]])
            res.consensus.append(consensus_read(side1, min_quality, start_char, table, dev, named[0]))
            res.consensus.append(consensus_read(side2, min_quality, start_char, table, dev, named[1]))
            res.affected += 2 * len(members)
            for pos, _ in members:
                res.discarded[pairs[pos][0]] = res.discarded[pairs[pos][1]] = 1
        else:
            rids = [pairs[pos][0] if pairs[pos][0] != NONE else pairs[pos][1] for pos, _ in members]
            res.consensus.append(consensus_read([reads[r] for r in rids], min_quality, start_char, table, dev))
            res.affected += len(members)
            for r in rids:
                res.discarded[r] = 1
    return res


def fastq_text(reads):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in reads).encode()


def parse_fastq(text):
    lines = text.decode().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def pair_list(reads, store_comment=1):
    return refpairs.identify_pairs([r[0] for r in reads], store_comment).pairs


# ---- cases worked by hand: dedup_length 4, qualities 'I' = Q40 (probability 0.9999) unless said, min quality 3, start char 33.
# With m members of probability p agreeing on a base the sum is m * p, `top` is the sum before the last member ((m - 1) * p, from the
# copy inside operator+, or p for m = 2) and getX answers `top`, which is at least 0.9999: 'I'.  Two members that disagree leave
# p + o on both bases (o = (1 - p) / 3): the > tree keeps the later letter of the alphabet on a tie, `best` still names the first
# member's base, so the sum itself (above 0.9999) is answered: 'I' again.
def _case(label, reads, expect, discarded=None, **cfg):
    c = dict(dedup_mode=1, paired=True, dedup_length=4, start_offset=0)
    c.update(cfg)
    return (label, reads, c, discarded, expect)


def _pairs_of(*ends):
    """interleaved pairs named p0/1 p0/2 p1/1 ...: ends = (bases1, bases2) or (bases1, quals1, bases2, quals2)"""
    out = []
    for i, e in enumerate(ends):
        if len(e) == 2:
            e = (e[0], "I" * len(e[0]), e[1], "I" * len(e[1]))
        out.append(("p%d/1" % i, e[0], e[1]))
        out.append(("p%d/2" % i, e[2], e[3]))
    return out


_FLIP = _pairs_of(("ACGTAA", "GGGGCC"), ("GGGGTT", "ACGTCC"))
HAND_CASES = [
    # p1 is p0's fragment read from the other strand: key(p0) = ACGT CCCC, key(p1) = GGGG ACGT whose reverse complement is p0's
    _case("flipped_duplicate_mode2", _FLIP, dict(groups=[(0, 2)], skipped=[0, 0, 0, 0], discarded=[1, 1, 1, 1], affected=4,
          consensus=[("C2-p0/1", "ACGTCC", "IIIIII"), ("C2-p0/2", "GGGGTT", "IIIIII")]), dedup_mode=2),
    _case("flipped_duplicate_missed_in_mode1", _FLIP, dict(groups=[], skipped=[0, 0, 0, 0], discarded=[0, 0, 0, 0], affected=0, consensus=[])),
    # p2 has an X inside the window (too short), p3 one behind it (takes part; the X adds nothing to the sums but counts)
    _case("x_inside_the_window", _pairs_of(("ACGTAA", "GGGGCC"), ("ACGTAA", "GGGGCC"), ("ACXTAA", "GGGGCC"), ("ACGTXA", "GGGGCC")),
          dict(groups=[(0, 3)], skipped=[0, 1, 0, 0], discarded=[1, 1, 1, 1, 0, 0, 1, 1], affected=6,
               consensus=[("C3-p0/1", "ACGTAA", "IIIIII"), ("C3-p0/2", "GGGGCC", "IIIIII")])),
    # start_offset 4: a read must hold 8 bases; p2's read 1 and p3's read 2 hold 7
    _case("exactly_long_enough_and_a_base_shorter", _pairs_of(("TTTTACGT", "CCCCGGGG"), ("TTTTACGT", "CCCCGGGG"), ("TTTTACG", "CCCCGGGG"), ("TTTTACGT", "CCCCGGG")),
          dict(groups=[(0, 2)], skipped=[0, 2, 0, 0], discarded=[1, 1, 1, 1, 0, 0, 0, 0], affected=4,
               consensus=[("C2-p0/1", "TTTTACGT", "IIIIIIII"), ("C2-p0/2", "CCCCGGGG", "IIIIIIII")]), start_offset=4),
    _case("discarded_mate", _pairs_of(("ACGTAA", "GGGGCC"), ("ACGTAA", "GGGGCC"), ("ACGTAA", "GGGGCC")),
          dict(groups=[(0, 2)], skipped=[1, 0, 0, 0], discarded=[1, 1, 0, 1, 1, 1], affected=4,
               consensus=[("C2-p0/1", "ACGTAA", "IIIIII"), ("C2-p0/2", "GGGGCC", "IIIIII")]), discarded=[0, 0, 0, 1, 0, 0]),
    # key = ACGT + revcomp(ACGT) = ACGTACGT is its own reverse complement: the forward key stays, nobody is flipped
    _case("key_equal_to_its_reverse_complement", _pairs_of(("ACGTAA", "ACGTCC"), ("ACGTAA", "ACGTCC")),
          dict(groups=[(0, 2)], skipped=[0, 0, 0, 0], discarded=[1, 1, 1, 1], affected=4,
               consensus=[("C2-p0/1", "ACGTAA", "IIIIII"), ("C2-p0/2", "ACGTCC", "IIIIII")]), dedup_mode=2),
    # every member shows N at positions 4 and 5: the four sums stay equal (0), the > tree ends at T, getT answers 0: quality 0
    _case("all_sums_equal_gives_t", _pairs_of(("ACGTNN", "GGGGCC"), ("ACGTNN", "GGGGCC")),
          dict(groups=[(0, 2)], skipped=[0, 0, 0, 0], discarded=[1, 1, 1, 1], affected=4,
               consensus=[("C2-p0/1", "ACGTTT", "IIII!!"), ("C2-p0/2", "GGGGCC", "IIIIII")])),
    # '#' = Q2 is below the minimum of 3: reading a member stops there, and nobody observes positions 4 to 7 of side 1
    _case("unobserved_tail", _pairs_of(("ACGTAAAA", "IIII#III", "GGGGCC", "IIIIII"), ("ACGTAAA", "IIII#II", "GGGGCC", "IIIIII")),
          dict(groups=[(0, 2)], skipped=[0, 0, 0, 0], discarded=[1, 1, 1, 1], affected=4,
               consensus=[("C2-p0/1", "ACGTTTTT", "IIII!!!!"), ("C2-p0/2", "GGGGCC", "IIIIII")])),
    # the --dedup-single pass: window of 2 * 4 bases; the pair list is (p/1, p/2), s0, s1: the pair is counted as unpaired, the blank ends the printed name
    _case("single_pass", [("s0 first", "ACGTACGTAA", "IIIIIIIIII"), ("p/1", "ACGTACGT", "IIIIIIII"), ("p/2", "ACGTACGT", "IIIIIIII"), ("s1", "ACGTACGTAA", "IIIIIIIIII")],
          dict(groups=[(1, 2)], skipped=[0, 0, 1, 0], discarded=[1, 0, 0, 1], affected=2, consensus=[("C2-s0", "ACGTACGTAA", "IIIIIIIIII")]), paired=False),
]


def run_case(case):
    label, reads, cfg, discarded, expect = case
    return filter_duplicate_fragments(reads, pair_list(reads), discarded, **cfg)


# ---- the seeded generator
def _revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def generate(seed, n_fragments=700, genome_len=5000):
    """About 2 000 pair records from a random genome: fragments duplicated 1 to 5 times with substitutions inside and outside the key
    window, noisy qualities with values below the minimum mid-read, read lengths 30 to 150 mixed inside a group, some duplicates given
    as (B, A), single reads (some duplicated), X runs.  Returns (reads, discarded flags)."""
    rng = np.random.default_rng(seed)
    genome = "".join("ACGT"[v] for v in rng.integers(0, 4, genome_len))
    reads = []

    def mutate(s):
        s = list(s)
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(0, len(s)))
            s[at] = "ACGTN"[int(rng.integers(0, 5))]
        if rng.random() < 0.05:
            at = int(rng.integers(0, len(s)))
            for k in range(at, min(len(s), at + int(rng.integers(1, 4)))):
                s[k] = "X"
        return "".join(s)

    def quals(n):
        q = rng.integers(20, 41, n)
        noisy = rng.random(n) < 0.04
        q[noisy] = rng.integers(0, 12, int(noisy.sum()))
        return "".join(chr(33 + int(v)) for v in q)

    frag = 0
    for _ in range(n_fragments):
        start = int(rng.integers(0, genome_len - 400))
        span = int(rng.integers(160, 400))
        copies = int(rng.integers(1, 6)) if rng.random() < 0.6 else 1
        single = rng.random() < 0.15
        for _ in range(copies):
            l1, l2 = int(rng.integers(30, 151)), int(rng.integers(30, 151))
            a = mutate(genome[start:start + l1])
            b = mutate(_revcomp_str(genome[start + span - l2:start + span]))
            name = "f%d" % frag
            frag += 1
            if single:
                reads.append((name, a, quals(len(a))))
                continue
            if rng.random() < 0.3:
                a, b = b, a
            reads.append((name + "/1", a, quals(len(a))))
            reads.append((name + "/2", b, quals(len(b))))
    discarded = (rng.random(len(reads)) < 0.03).astype(np.uint8)
    return reads, discarded
