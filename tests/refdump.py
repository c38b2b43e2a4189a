"""MeraculousCounter's two texts restated plainly over strings, lists and ints: what kmr_dump_text, kmr_dump_text_size,
kmr_dump_mercount and kmr_dump_mergraph are held to (tests/test_gpu_dump_edges.py) and what the oracle's dump is held to
(tests/test_dump_cases.py).  Nothing here comes from kmernator_amd or from the oracle.

Written from the reference:
  dumpCounts / dumpGraphs                       src/Meraculous.h:107-133        for every weak entry in the map's iteration order: skipped if
                                                                                (int)count < minDepth; else the k-mer's line and its reverse
                                                                                complement's line
  ExtensionTracking::toTextValues               src/KmerTrackingData.h:207-218  _extensionCounts[Left][A C G T N X], then [Right][...], a blank
                                                                                between them, then " 0"
  ExtensionTracking::getReverseComplement       src/KmerTrackingData.h:219-226  rev[Left][rc(i)] = [Right][i], rev[Right][rc(i)] = [Left][i]
  Extension::getReverseComplement               src/KmerTrackingData.h:80-92    A <-> T, C <-> G, anything else itself
  toFasta (TwoBitSequence::uncompressSequence)  src/TwoBitSequence.cpp:272-292  four bases a byte, the first in the top two bits, "ACGT"[code]
  buildReverseComplement                        src/TwoBitSequence.cpp:395-409  the bases in reverse order, each complemented

A parsed image is refimage.parse's (nb, mask, buckets): buckets[b] a list of (key_bytes, value) in stored order, a weak value
(count, weighted_bits, direction_bias, tallies, padding).  The map's iteration order is bucket by bucket, stored order inside a
bucket.  The twelve tallies of a value are _extensionCounts in memory order: Left A C G T N X, Right A C G T N X.

`wrong` names a deliberately wrong variant of one rule (WRONG): tests/test_dump_cases.py shows that each of them changes the
expected text of at least one family of tests/dumpcases.py."""

WRONG = ("rc_tallies_unpermuted", "rc_sides_not_swapped", "rc_n_x_swapped", "rc_left_n_only", "rc_not_complemented", "rc_not_reversed",
         "strict_min_depth", "unsigned_min_depth", "count_is_direction_bias", "stored_order_ignored", "no_trailing_zero")

A, C, G, T, N, X = range(6)
LEFT, RIGHT = 0, 1


def fasta(key, k):
    """toFasta of a packed k-mer"""
    return "".join("ACGT"[(key[p >> 2] >> (6 - 2 * (p & 3))) & 3] for p in range(k))


def reverse_complement(seq, wrong=None):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    if wrong != "rc_not_reversed":
        seq = seq[::-1]
    if wrong != "rc_not_complemented":
        seq = "".join(comp[c] for c in seq)
    return seq


def extension_rc(i, wrong=None):
    """Extension::getReverseComplement of an index"""
    if i == A:
        return T
    if i == C:
        return G
    if i == G:
        return C
    if i == T:
        return A
    if wrong == "rc_n_x_swapped":
        return X if i == N else N
    return i


def tallies_rc(tallies, wrong=None):
    """ExtensionTracking::getReverseComplement, by its loop"""
    if wrong == "rc_tallies_unpermuted":
        return tuple(tallies)
    counts = [list(tallies[:6]), list(tallies[6:])]
    rev = [[0] * 6, [0] * 6]
    for i in range(6):
        if wrong == "rc_sides_not_swapped":
            rev[LEFT][extension_rc(i, wrong)] = counts[LEFT][i]
            rev[RIGHT][extension_rc(i, wrong)] = counts[RIGHT][i]
        else:
            rev[LEFT][extension_rc(i, wrong)] = counts[RIGHT][i]
            rev[RIGHT][extension_rc(i, wrong)] = counts[LEFT][i]
    if wrong == "rc_left_n_only":
        rev[LEFT][N] = counts[LEFT][N]
    return tuple(rev[LEFT] + rev[RIGHT])


def text_values(tallies, wrong=None):
    """ExtensionTracking::toTextValues"""
    s = ""
    for j in range(2):
        for i in range(6):
            if i + j != 0:
                s += " "
            s += str(tallies[6 * j + i])
    return s if wrong == "no_trailing_zero" else s + " 0"


def as_int32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def kept(count, min_depth, wrong=None):
    """not ((int)count < (int)minDepth); min_depth arrives as the C ABI's uint32_t"""
    if wrong == "unsigned_min_depth":
        return not count < (min_depth & 0xffffffff)
    if wrong == "strict_min_depth":
        return not count <= as_int32(min_depth)
    return not count < as_int32(min_depth)


def entries_of(parsed, wrong=None):
    nb, _, buckets = parsed
    flat = [kv for b in buckets for kv in b]
    return sorted(flat, key=lambda kv: kv[0]) if wrong == "stored_order_ignored" else flat


def entry_text(key, value, k, graph, wrong=None):
    count, _, direction_bias, tallies, _ = value
    fwd = fasta(key, k)
    rev = reverse_complement(fwd, wrong)
    if graph:
        assert len(tallies) == 12, "mergraph needs the extension tallies"
        return "%s\t%s\n%s\t%s\n" % (fwd, text_values(tallies, wrong), rev, text_values(tallies_rc(tallies, wrong), wrong))
    c = direction_bias          # long count = getDirectionBias(); long revCount = getCount() - count; both lines print their sum
    rev_count = count - c
    if wrong == "count_is_direction_bias":
        rev_count = 0
    return "%s\t%d\n%s\t%d\n" % (fwd, c + rev_count, rev, rev_count + c)


def pieces(parsed, k, kind, min_depth, graph, lo=0, hi=None, wrong=None):
    """the text of every entry of [lo, hi) in iteration order, b"" for an entry that is not kept"""
    assert kind in ("weak", "weak_ext") and (not graph or kind == "weak_ext")
    entries = entries_of(parsed, wrong)
    hi = len(entries) if hi is None else min(hi, len(entries))
    return [entry_text(key, v, k, graph, wrong).encode() if kept(v[0], min_depth, wrong) else b"" for key, v in entries[lo:hi]]


def text(parsed, k, kind, min_depth, graph, lo=0, hi=None, wrong=None):
    return b"".join(pieces(parsed, k, kind, min_depth, graph, lo, hi, wrong))


def offsets(parsed, k, kind, min_depth, graph, lo=0, hi=None, wrong=None):
    """the byte offset of every entry of [lo, hi) in the text of that range, and the text's length as the last value"""
    off = [0]
    for p in pieces(parsed, k, kind, min_depth, graph, lo, hi, wrong):
        off.append(off[-1] + len(p))
    return off
