"""The selection of FilterReads and the text of a picked read, restated from the reference's source alone over Python bytes and
numpy.float32: ReadSelectorUtil::passesLength (src/ReadSelector.h:219-228), isPassingRead / isPassingPair (:550-568),
pickAllPassingReads / pickAllPassingPairs (:576-596) with optimizePickOrder (:1212-1221), the label FilterKnownOddities
(src/FilterKnownOddities.h:328), trimReadByMinimumKmerScore (src/ReadSelector.h:987-1005) and setTrimHeaders (:1015-1036) leave,
Sequence::getFasta (src/Sequence.cpp:305-328), Read::setRead's rule for quality-less reads (:652-655), Read::getQuals (:729-759) and
Read::toFastq / toFasta (:761-779).  Nothing here is derived from kmr_select.hpp or from refsemantics.filterreads_output;
tests/selectcases.py holds the directed cases, tests/test_select_cases.py proves that they notice every rule below.

A read is (name line without its lead character, bases, qualities), all bytes; the qualities are the batch's, at `in_base` (the
reference keeps its reads at the output base and rescales on the way in, src/ReadSet.cpp:324-337; the batch keeps them as they
came and moves them by out_base - in_base on the way out, which is the same byte for every real quality).  Read::REF_QUAL (127)
is not a quality and is not moved: a read whose first stored quality is 127 has none (setRead), and getQuals prints
PRINT_REF_QUAL (103, src/config.h:140) for every base of such a read and of a slice whose first byte is 127.

Where the reference is undefined, asserts, or does something the batch cannot repeat, the restatement holds this project's rule and
says so -- no parity is claimed there:
  - with in_base != out_base the reference's serial readers rescale every quality byte on the way in, a 127 too
    (src/ReadSet.cpp:324-337, src/Sequence.h:443-447; only the threaded reader spares it, src/ReadSet.h:694), so there a 127 of the
    input is 96 or 158 before setRead and getQuals see it and neither test for REF_QUAL fires.  The batch keeps the 127, and the 127
    rule holds at any pair of bases: parity where in_base == out_base, the project's own rule where they differ (the Q cases
    33 -> 64 and 64 -> 33);
  - (int)(score + 0.5) of a NaN or of a sum outside int is undefined in C++: the project prints 0 for NaN and clamps to
    [-2147483648, 2147483647] (score_int reports such a score as not defined by the reference);
  - getFasta and getQuals assert trimOffset <= length (src/Sequence.cpp:315, 737).  An offset equal to the length is inside the
    reference: the clamp leaves no base, the masked N.  Past the read the unsigned len - trimOffset wraps; the project cuts the slice
    to nothing there too;
  - FilterKnownOddities asserts maxPass > minPass (src/FilterKnownOddities.h:322); without the assert the unsigned difference wraps.
    The project prints the signed difference;
  - a bimodal word with equal means cannot come out of the cut (its truncated difference is at least 1); the word's contract is
    "Inv where the first is the smaller" (include/kmernator_amd.h), so equal means print without Inv."""
import bisect

import numpy as np

REF_QUAL = 127                # src/config.h:141
PRINT_REF_QUAL = 103          # src/config.h:140
SCORE_LABEL = (b"Score", b"MedianScore", b"MinScore", b"MaxScore", b"AvgScore")      # getKmerScoringTypeLabel :248-257
F = np.float32

# ---- named rules: every function takes `wrong` (None, a name or a set of names); each name switches one rule to a plausible wrong one
RULES = (
    "product_in_double",           # readLength * minimumLength not rounded to float
    "fraction_strict",             # < for <= in the fraction branch of passesLength
    "absolute_strict",             # < for <= in the absolute branch
    "score_strict",                # > for >= on the score
    "score_truncates",             # (int) score
    "score_half_even",             # round-half-even
    "score_half_in_float",         # score + 0.5f, rounded to float before the cast
    "mask_at_zero",                # the mask at trimLength == 0 instead of <= 1
    "no_slice_clamp",              # trimLength is not cut to the read's end
    "aftrim_unsigned",             # the AFTrim difference as a wrapped u32
    "inv_on_equal",                # Inv on m1 <= m2
    "label_parts_swapped",         # Trim in front of the bimodal tag
    "name_ends_at_blank_only",     # a tab stays in the printed name
    "masked_qual_from_input_base",  # the masked quality is in_base + 1
    "shift_wrong_sign",            # qualities move by in_base - out_base
    "ref_qual_shifted",            # 127 moves like any quality
    "ref_qual_every_byte",         # 127 becomes 103 byte by byte instead of by the first byte's test
    "both_pass_as_either",         # --min-passing-in-pair 2 decides like 1
    "failed_mate_left_out",        # only the passing reads of a passing pair are picked
)


def _wrong(wrong):
    if wrong is None:
        return frozenset()
    w = frozenset([wrong]) if isinstance(wrong, str) else frozenset(wrong)
    assert w <= set(RULES), w - set(RULES)
    return w


def passes_length(length, read_length, minimum_length, wrong=None):
    """:219-228.  length and minimumLength are float parameters; readLength * minimumLength is unsigned times float = float"""
    w = _wrong(wrong)
    length, minimum_length = F(length), F(minimum_length)
    if length <= F(1.0):
        return False
    if minimum_length <= F(1.0):
        product = float(read_length) * float(minimum_length) if "product_in_double" in w else float(F(read_length) * minimum_length)
        return product < float(length) if "fraction_strict" in w else product <= float(length)      # compared as Python floats: both sides exact
    return bool(minimum_length < length) if "absolute_strict" in w else bool(minimum_length <= length)


def is_passing_read(discarded, score, trim_length, read_length, min_score, min_read_length, wrong=None):
    """:550-557 without availability (one round): trim.score >= minimumScore, both ScoreType = float; a NaN score fails"""
    if discarded:
        return False
    s, m = F(score), F(min_score)
    ok = bool(s > m) if "score_strict" in _wrong(wrong) else bool(s >= m)
    return ok and passes_length(float(trim_length), read_length, min_read_length, wrong)


def score_int(score, wrong=None):
    """(int)(trim.score + 0.5) (:1033): float + double literal = double, truncated toward zero.  Returns (the number printed, whether
    the reference defines it)"""
    w = _wrong(wrong)
    s = float(F(score))
    if s != s:
        return 0, False
    if "score_truncates" in w:
        v = s
    elif "score_half_even" in w:
        v = float(np.rint(s))
    elif "score_half_in_float" in w:
        v = float(F(score) + F(0.5))
    else:
        v = s + 0.5
    if v >= 2147483648.0:
        return 2147483647, False
    if v <= -2147483649.0:
        return -2147483648, False
    return int(v), True


def label(af, word, was_trimmed, trim_off, trim_len, score, scoring, wrong=None):
    """what Read::toFastq is handed as `label`, parts joined by LABEL_SEP; af = (min_pass, max_pass) of a trim by the artifact
    filter or None, word = the bimodal cut (0: none)"""
    w = _wrong(wrong)
    parts = []
    if af is not None:
        diff = int(af[1]) - int(af[0])
        parts.append(b"AFTrim:%d+%d" % (af[0], diff & 0xffffffff if "aftrim_unsigned" in w else diff))
    tag = None
    if word:
        m1, m2 = (word >> 32) & 0xffff, word >> 48
        inv = m1 <= m2 if "inv_on_equal" in w else m1 < m2
        tag = (b"Inv" if inv else b"") + b"Bimodal@%d:%d/%d" % (word & 0xffffffff, m1, m2)
    trim = b"Trim:%d+%d" % (trim_off, trim_len) if was_trimmed else None      # :1026-1030
    parts += [p for p in ((trim, tag) if "label_parts_swapped" in w else (tag, trim)) if p is not None]
    parts.append(SCORE_LABEL[scoring] + b":%d" % score_int(score, wrong)[0])
    return b" ".join(parts)


def printed_name(name_line, wrong=None):
    """the name ends at the first blank or tab of its line (the comment behind it is not printed)"""
    name = name_line.split(b" ")[0]
    return name if "name_ends_at_blank_only" in _wrong(wrong) else name.split(b"\t")[0]


def slice_of(read_length, discarded, trim_off, trim_len, wrong=None):
    """Sequence::getFasta :305-321 and Read::getQuals :729-741 decide alike: masked (the single N), or [from, from + length)"""
    w = _wrong(wrong)
    tl = int(trim_len)
    lowest = 0 if "mask_at_zero" in w else 1
    if discarded or tl <= lowest:
        return None
    if "no_slice_clamp" not in w:
        tl = min(tl, max(0, read_length - int(trim_off)))
    if tl <= lowest:
        return None
    return int(trim_off), tl


def quals_printed(qual, sl, in_base, out_base, wrong=None):
    """Read::getQuals(trimOffset, trimLength, forPrinting = true) (:729-759)"""
    w = _wrong(wrong)
    if sl is None:
        return bytes([(in_base if "masked_qual_from_input_base" in w else out_base) + 1])
    to, tl = sl
    shift = in_base - out_base if "shift_wrong_sign" in w else out_base - in_base
    q = qual[to:to + tl]
    moved = bytes((c + shift) & 0xff for c in q)
    if "ref_qual_shifted" in w:
        return moved
    if "ref_qual_every_byte" in w:
        return bytes(PRINT_REF_QUAL if c == REF_QUAL else m for c, m in zip(q, moved))
    has_quals = not (len(qual) > 1 and qual[0] == REF_QUAL)      # setRead :652-655
    if not has_quals or (q and q[0] == REF_QUAL):                # :744
        return bytes([PRINT_REF_QUAL]) * len(q)
    return moved


def record(read, lab, discarded, trim_off, trim_len, in_base, out_base, fasta, wrong=None):
    """Read::toFastq / toFasta (:761-779) with unmasked = false; a discarded read has no label"""
    name_line, seq, qual = read
    sl = slice_of(len(seq), discarded, trim_off, trim_len, wrong)
    bases = b"N" if sl is None else seq[sl[0]:sl[0] + sl[1]]
    head = printed_name(name_line, wrong) + ((b" " + lab) if lab else b"")
    if fasta:
        return b">" + head + b"\n" + bases + b"\n"
    return b"@" + head + b"\n" + bases + b"\n+\n" + quals_printed(qual, sl, in_base, out_base, wrong) + b"\n"


class Selection:
    """text, picked (bool per read), n_picked, bytes, table[input] = (first pick, picks, first byte, bytes), read_segment"""


def select(reads, mate, af, to, tl, sc, wt, words, cfg, wrong=None):
    """One round of selectReads over a batch: the pair decision per read (pickAllPassingPairs over the pairs of `mate`; mate None or
    -1: pickAllPassingReads), every read of a passing pair picked, the picks in ascending read index, each written to the output
    of its input (cfg["input_starts"], None = one).  af = (action, min_pass, max_pass) or None; words = bimodal words or None.
    cfg: min_score, min_read_length, both_pass, scoring, in_base, out_base, fasta, input_starts."""
    w = _wrong(wrong)
    n = len(reads)
    disc = [af is not None and int(af[0][i]) == 2 for i in range(n)]
    passing = [is_passing_read(disc[i], sc[i], tl[i], len(reads[i][1]), cfg["min_score"], cfg["min_read_length"], wrong) for i in range(n)]
    both = cfg["both_pass"] and "both_pass_as_either" not in w
    picked = np.zeros(n, dtype=bool)
    for i in range(n):
        j = -1 if mate is None else int(mate[i])
        if j < 0:
            picked[i] = passing[i]
        else:
            pair = (passing[i] and passing[j]) if both else (passing[i] or passing[j])
            picked[i] = pair and (passing[i] or "failed_mate_left_out" not in w)
    starts = [0, n] if cfg.get("input_starts") is None else [int(x) for x in cfg["input_starts"]]
    res = Selection()
    res.picked, res.table, res.read_segment = picked, [], np.full(n, -1, dtype=np.int32)
    out, n_picks, n_bytes = [], 0, 0
    for f in range(len(starts) - 1):
        mine = [i for i in range(n) if picked[i] and bisect.bisect_right(starts, i) - 1 == f]
        recs = []
        for i in mine:
            lab = b"" if disc[i] else label((af[1][i], af[2][i]) if af is not None and int(af[0][i]) == 1 else None, 0 if words is None else int(words[i]),
                                            bool(wt[i]), int(to[i]), int(tl[i]), sc[i], cfg["scoring"], wrong)
            recs.append(record(reads[i], lab, disc[i], to[i], tl[i], cfg["in_base"], cfg["out_base"], cfg["fasta"], wrong))
            res.read_segment[i] = f
        text = b"".join(recs)
        res.table.append((n_picks, len(mine), n_bytes, len(text)))
        n_picks += len(mine)
        n_bytes += len(text)
        out.append(text)
    res.text = b"".join(out)
    res.n_picked, res.bytes = n_picks, n_bytes
    return res
