"""Directed cases for the duplicate-fragment collapse (kmr_dedup_fragments*, kmernator_amd/csrc/kmr_dedup.hpp): small batches built
by rule, no random search at test time, each family aimed at one part of the stage's exact arithmetic.  A family is a function that
returns a list of cases

    (label, reads, discarded, cfg, handle_cfg, deviations_it_must_notice)

reads = [(name line, bases, qualities)] as tests/refdedup.py takes them; discarded = flags per read or None; cfg = dedup_mode,
dedup_length, start_offset, plus `passes` ("paired", "single", or "both" = the paired pass and then the single pass on its discards,
what --dedup-single runs), `named` (False: the batch has no names and goes to the device through ReadSet.from_arrays, every read a
half pair of its own -- the way for bytes FASTQ text cannot carry) and `store_comment`; handle_cfg = min_quality_score and
fastq_start_char of the handle; the last entry names the deviations of refdedup.DEVIATIONS that this case's result must change
under.  tests/test_dedup_cases.py proves on the CPU that it does and that every family reaches what it is written for;
tests/test_gpu_dedup_edges.py runs every case on the device.

    G  geometry: every dedup_length x start_offset x mode, the window's two ends from inside and outside, lengths, X, N
    K  multi-word keys: one-base differences at both ends of every key word, canonical ties, palindromes, interleaved groups
    Q  the quality ladder: one observation at every input quality, which sits on the steps of probToQual
    D  disagreement: two and three members at every pair of qualities, the tie branches of getBaseQual's tree
    S  stops and lengths: wavefront borders, low qualities, unobserved positions, characters
    W  the member count as a short
    F  flips, sides and names
    P  pair-list shapes and the skip counters
    M  more (group, side) tasks than one grid of the consensus kernel holds"""
import functools
import random

import refdedup
import refpairs

NONE = refdedup.NONE
HANDLE = dict(min_quality_score=3, fastq_start_char=33)
LENGTHS = tuple(range(4, 65, 4))
OFFSETS = (0, 4, 60, 64)
FAMILIES = "GKQDSWFPM"


def _case(label, reads, notice, discarded=None, handle=None, **cfg):
    c = dict(dedup_mode=1, dedup_length=4, start_offset=0, passes="paired", named=True, store_comment=1)
    c.update(cfg)
    h = dict(HANDLE)
    h.update(handle or {})
    return (label, reads, discarded, c, h, tuple(notice))


def _rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _other(ch):
    """another base, never the one N packs as by accident: A -> C -> G -> T -> A"""
    return "CGTA"["ACGT".index(ch)]


def _sub(s, at, ch=None):
    return s[:at] + (_other(s[at]) if ch is None else ch) + s[at + 1:]


def _q(n, start_char=33, q=40):
    return chr(start_char + q) * n


# ---- what a case's batch is on both sides of the comparison
def pair_list(case):
    _, reads, _, cfg, _, _ = case
    if not cfg["named"]:
        return [(i, NONE) for i in range(len(reads))]          # pairs_single_kernel: every read a half pair on side 1
    return refpairs.identify_pairs([r[0] for r in reads], cfg["store_comment"]).pairs


def run(case, deviation=None):
    """the restatement's results of the case's passes, in order"""
    _, reads, discarded, cfg, handle, _ = case
    kw = dict(dedup_mode=cfg["dedup_mode"], dedup_length=cfg["dedup_length"], start_offset=cfg["start_offset"],
              min_quality=handle["min_quality_score"], start_char=handle["fastq_start_char"], deviation=deviation)
    pairs = pair_list(case)
    out = []
    if cfg["passes"] in ("paired", "both"):
        out.append(refdedup.filter_duplicate_fragments(reads, pairs, discarded, paired=True, **kw))
        discarded = out[0].discarded if cfg["passes"] == "both" else discarded
    if cfg["passes"] in ("single", "both"):
        out.append(refdedup.filter_duplicate_fragments(reads, pairs, discarded, paired=False, **kw))
    return out


def signature(results):
    return [(r.discarded, r.skipped, r.affected, r.groups, r.consensus) for r in results]


# ---- G: geometry
def _g_variants(frag, so, L, tag):
    """(tag, bases) of one side: the fragment and its neighbours around the window [so, so + L)"""
    need = so + L
    a_at = so + L // 2
    assert frag[a_at] == "A" and len(frag) == need + 5
    v = [("same", frag), ("first", _sub(frag, so)), ("last", _sub(frag, need - 1)), ("behind", _sub(frag, need)),
         ("exact", frag[:need]), ("short", frag[:need - 1]), ("X-last", _sub(frag, need - 1, "X")), ("x-behind", _sub(frag, need, "x")),
         ("x-last", _sub(frag, need - 1, "x")), ("X-behind", _sub(frag, need, "X")), ("N-for-A", _sub(frag, a_at, "N")), ("n-for-A", _sub(frag, a_at, "n"))]
    if so:
        v += [("before", _sub(frag, so - 1)), ("X-before", _sub(frag, so - 1, "X")), ("x-first-base", _sub(frag, 0, "x"))]
    return [(tag + "-" + t, b) for t, b in v]


def _g_fragment(rng, so, L):
    f = _rnd(rng, so + L + 5)
    return _sub(f, so + L // 2, "A")


def G(lengths=LENGTHS):
    cases = []
    for L in lengths:
        for so in OFFSETS:
            rng = random.Random(1000 * L + so)
            f1, f2, s = _g_fragment(rng, so, L), _g_fragment(rng, so, L), _g_fragment(rng, so, 2 * L)
            pairs = [("same", f1, f2), ("dup", f1, f2), ("swapped", f2, f1)]
            pairs += [(t, b, f2) for t, b in _g_variants(f1, so, L, "r1")[1:]] + [(t, f1, b) for t, b in _g_variants(f2, so, L, "r2")[1:]]
            singles = [("dup", s)] + _g_variants(s, so, 2 * L, "s") + [("s-mid-left", _sub(s, so + L - 1)), ("s-mid-right", _sub(s, so + L))]
            reads = []
            for i, (t, a, b) in enumerate(pairs):
                reads.append(("g%d-%s/1" % (i, t), a, _q(len(a))))
                reads.append(("g%d-%s/2" % (i, t), b, _q(len(b))))
            for i, (t, a) in enumerate(singles):
                reads.append(("s%d-%s" % (i, t), a, _q(len(a))))
            for mode in (1, 2):
                notice = ["key_window_shifted", "n_is_its_own_code", "last_key_word_ignored"] + (["x_before_window_ignored"] if so else [])
                cases.append(_case("G-len%d-off%d-mode%d" % (L, so, mode), reads, notice, dedup_mode=mode, dedup_length=L, start_offset=so, passes="both"))
    return cases


# ---- K: multi-word keys
K_LENGTHS = (20, 36, 52, 64)


def key_of(bases1, bases2, L, so=0):
    """the forward key of a pair as a string of bases: window 1, then the reverse complement of window 2"""
    return bases1[so:so + L] + revcomp(bases2[so:so + L])


def _split_key(key):
    """the two windows whose forward key is `key`"""
    L = len(key) // 2
    return key[:L], revcomp(key[L:])


def _tie_key(rng, n, w, forward_less):
    """a key of n bases that agrees with its reverse complement in words 0 .. w - 1 (bases 0 .. 32 w - 1) and differs in word w,
    at that word's first base, the forward key being the smaller one or not.  K[i] == comp(K[n - 1 - i]) for i < 32 w."""
    assert 32 * w < n // 2          # agreement up to half the key's bases is equality: no later word can decide
    k = list(_rnd(rng, n))
    for i in range(32 * w):
        k[n - 1 - i] = revcomp(k[i])
    i = 32 * w                     # rc(K)[i] = comp(K[n - 1 - i]): forward 'A' against reverse 'C', or the other way round
    k[i], k[n - 1 - i] = ("A", "G") if forward_less else ("C", "T")
    return "".join(k)


def _palindrome(rng, n):
    half = _rnd(rng, n // 2)
    return half + revcomp(half)


def K_ties(L):
    """[(word that decides, forward key is the smaller, key)] for dedup_length L"""
    rng = random.Random(77 + L)
    n = 2 * L
    return [(w, fl, _tie_key(rng, n, w, fl)) for w in range(4) if 32 * w < n // 2 for fl in (True, False)]


def K():
    cases = []
    for L in K_LENGTHS:
        n = 2 * L
        W = (n + 31) // 32
        rng = random.Random(500 + L)
        base = _rnd(rng, n)
        frags = [("base", base)]          # (tag, key): every one becomes a group of two
        for w in range(W):
            first, last = 32 * w, min(32 * w + 31, n - 1)
            frags += [("w%d-first" % w, _sub(base, first)), ("w%d-last" % w, _sub(base, last))]
        frags += [("pal", _palindrome(rng, n))]
        ties = K_ties(L)
        # four groups whose members interleave, met in descending order of their forward keys
        inter = ["T" + _rnd(rng, n - 2) + "G", "G" + _rnd(rng, n - 2) + "G", "C" + _rnd(rng, n - 2) + "G", "A" + _rnd(rng, n - 2) + "G"]
        reads, j = [], 0

        def add_pair(tag, key, swap=False):
            nonlocal j
            w1, w2 = _split_key(key)
            t1, t2 = _rnd(rng, 1 + j % 5), _rnd(rng, 2 + j % 3)          # tails differ between members and sides
            a, b = (w1 + t1, w2 + t2) if not swap else (w2 + t2, w1 + t1)
            reads.append(("k%d-%s/1" % (j, tag), a, _q(len(a), q=20 + j % 20)))
            reads.append(("k%d-%s/2" % (j, tag), b, _q(len(b), q=39 - j % 20)))
            j += 1

        def add_single(tag, key):
            nonlocal j
            a = key + _rnd(rng, 1 + j % 4)
            reads.append(("k%d-%s" % (j, tag), a, _q(len(a), q=20 + j % 20)))
            j += 1
        for rnd_ in range(3):          # interleaved: member order a b c d a b c d a b c d
            for g, key in enumerate(inter):
                add_pair("inter%d" % g, key)
        for tag, key in frags:
            add_pair(tag, key); add_pair(tag, key)
        for w, fl, key in ties:        # the fragment as (A, B) and as (B, A): one group in mode 2
            add_pair("tie%d%s" % (w, "lt" if fl else "gt"), key); add_pair("tie%d%s" % (w, "lt" if fl else "gt"), key, swap=True)
        for rnd_ in range(2):
            for g, key in enumerate(inter):
                add_single("sinter%d" % g, key)
        for tag, key in frags:
            add_single("s" + tag, key); add_single("s" + tag, key)
        for mode in (1, 2):
            notice = ["last_key_word_ignored", "members_not_in_pair_order", "groups_in_key_order"]
            if mode == 2:
                notice += ["canonical_tie_takes_reverse", "flip_sides_not_swapped"] + (["canonical_first_word_only"] if any(w > 0 for w, _, _ in ties) else [])
            cases.append(_case("K-len%d-mode%d" % (L, mode), reads, notice, dedup_mode=mode, dedup_length=L, passes="both"))
    return cases


# ---- Q: the quality ladder
def Q_bytes(min_q, start_char):
    """quality bytes from the minimum to Q42, then Q69 and Q70 (bytes 102 and 103 at base 33) and the bytes 102, 103, 126, 127, 255"""
    b = list(range(start_char + min_q, start_char + 43))
    for x in (start_char + 69, start_char + 70, 102, 103, 126, 127, 255):
        if x not in b and start_char + min_q <= x <= 255:
            b.append(x)
    return b


def Q():
    """Two members without names, one pass over single reads, window "ACGTACGT".  Behind it member 1 shows A at every quality byte
    in turn and member 2 shows N at Q40, which counts and adds nothing: `top` is member 1's probability, best is A, count is 2, so
    getA answers exactly 1 - 10^(-q/10) (or the 0.2501 floor), and that sits on a step of probToQual."""
    cases = []
    for min_q, start_char in ((0, 33), (1, 33), (3, 33), (10, 33), (3, 64)):
        qb = Q_bytes(min_q, start_char)
        w = "ACGTACGT"
        reads = [("", w + "A" * len(qb), _q(8, start_char) + "".join(chr(x) for x in qb)), ("", w + "N" * len(qb), _q(8 + len(qb), start_char))]
        # (at base 64 Q39 is byte 103 already: probability 1.0, so nothing lies between 0.9999 and 1.0 there)
        notice = ["qual_rounds"] + (["no_floor"] if min_q < 2 else []) + (["ref_qual_not_one"] if start_char == 64 else ["forty_from_0_9999_off"])
        cases.append(_case("Q-min%d-base%d" % (min_q, start_char), reads, notice, handle=dict(min_quality_score=min_q, fastq_start_char=start_char),
                           passes="single", named=False))
    return cases


# ---- D: disagreement
D_QUALS = tuple(range(3, 42))
D_COARSE = (3, 10, 20, 30, 41)


def _index_key(i, n):
    """n bases that spell i in base 4"""
    return "".join("ACGT"[(i >> (2 * (n - 1 - p))) & 3] for p in range(n))


def D():
    """Paired pass, dedup_length 8; read 2 is the window alone.  Group g of the grid: member 1 shows A at quality 3 + g at every
    position behind the window, member 2 shows C at quality 3 + p at position p: every (q1, q2)."""
    reads, g = [], 0

    def group(columns):
        """columns = [(base, quality) per member] per position"""
        nonlocal g
        w1, w2 = _index_key(g, 8), "ACGTACGT"
        for m in range(len(columns[0])):
            reads.append(("d%d-%d/1" % (g, m), w1 + "".join(c[m][0] for c in columns), _q(8) + "".join(chr(33 + c[m][1]) for c in columns)))
            reads.append(("d%d-%d/2" % (g, m), w2, _q(8)))
        g += 1
    for q1 in D_QUALS:
        group([(("A", q1), ("C", q2)) for q2 in D_QUALS])
    coarse = [(a, b, c) for a in D_COARSE for b in D_COARSE for c in D_COARSE]
    for pattern in ("AAC", "ACA", "CAA", "ACG", "GTC", "TTA"):          # majority in every seat, and three-way splits
        group([tuple(zip(pattern, qs)) for qs in coarse])
    grid = _case("D-grid", reads, ["copy_does_not_raise_top", "get_ignores_best", "members_not_in_pair_order", "tree_not_strict", "qual_rounds"], dedup_length=8)
    # the tie branches: every ordered pair and triple of distinct bases at equal quality
    reads, g = [], 1000
    pairs = [(a, b) for a in "ACGT" for b in "ACGT" if a != b]
    triples = [(a, b, c) for a in "ACGT" for b in "ACGT" for c in "ACGT" if len({a, b, c}) == 3]
    group([tuple((b, q) for b in p) for q in (3, 20, 40) for p in pairs] + [(("N", 40), ("N", 40)), (("n", 3), ("N", 3))])          # and nothing: T at quality 0
    group([tuple((b, q) for b in t) for q in (3, 20, 40) for t in triples])
    group([tuple((b, q) for b in "ACGT"[r:] + "ACGT"[:r]) for q in (3, 20, 40) for r in range(4)])          # all four
    ties = _case("D-ties", reads, ["tree_not_strict", "set_top_not_strict", "members_not_in_pair_order"], dedup_length=8)
    return [grid, ties]


# ---- S: stops and lengths
S_LENGTHS = (63, 200, 4, 64, 129, 65, 127, 128)          # (a member holds at least start_offset + dedup_length = 4 bases: 1 cannot occur)
S_STOPS = (0, 63, 64, 65, 129, None)                     # in reads of 130 bases: 129 is the last base, None = nowhere


def S():
    rng = random.Random(9)
    reads = []
    body1, body2 = "ACGT" + _rnd(rng, 196), "GGCA" + _rnd(rng, 196)

    def noisy(s, i):          # one substitution per member behind the window, at a place of its own
        return _sub(s, 4 + 7 * i) if len(s) > 4 + 7 * i else s
    for i, n in enumerate(S_LENGTHS):          # lengths mixed inside one group, the longest not first; side 2 in another order
        a, b = noisy(body1[:n], i), noisy(body2[:S_LENGTHS[-1 - i]], i)
        reads.append(("len%d/1" % i, a, "".join(chr(33 + 3 + (5 * i + p) % 38) for p in range(len(a)))))
        reads.append(("len%d/2" % i, b, "".join(chr(33 + 40 - (3 * i + p) % 38) for p in range(len(b)))))
    body1, body2 = "CCAT" + _rnd(rng, 126), "TTAG" + _rnd(rng, 126)
    for i, stop in enumerate(S_STOPS):         # the first low quality at a wavefront border, at the ends, nowhere
        q = [chr(33 + 10 + (i + p) % 30) for p in range(130)]
        if stop is not None:
            q[stop] = "#"                      # Q2, below the minimum of 3
            if stop + 3 < 130:
                q[stop + 3] = "!"
        reads.append(("stop%d/1" % i, noisy(body1, i), "".join(q)))
        reads.append(("stop%d/2" % i, noisy(body2, i), "".join(q[::-1])))
    for i in range(3):                         # positions 6 .. 9 are inside every member's length and nobody observes them
        reads.append(("dark%d/1" % i, "GATTACAGATTA"[:12 - i], "IIIIII\"IIIII"[:12 - i]))
        reads.append(("dark%d/2" % i, "TGCATGCATG", "!IIIIIIIII"))          # stopped at position 0: every position of side 2 is dark
    named = _case("S-lengths-and-stops", reads, ["low_quality_skips", "members_not_in_pair_order"], dedup_length=4)
    # characters: lower case inside and behind the window, other characters behind it (raw bytes, so without names, single pass)
    tails = ["acgtnACGTN.R-*xX", "ACGTNacgtn.R-*Xx", "NNNNNnnnnn....XX", "tgcanTGCAN-R.*xx"]
    reads = [("", w + t, _q(8) + "".join(chr(33 + 5 + (7 * i + p) % 36) for p in range(len(t)))) for i, (w, t) in enumerate(zip(("ACGTACGT", "acgtacgt", "AcGtNCGT", "nCgTaCgT"), tails))]
    reads += [("", "ACGTACxT" + tails[0], _q(8 + 16)), ("", "ACGTACGTx", _q(9)), ("", "ACGTACGTX", _q(9))]
    chars = _case("S-characters", reads, ["n_is_its_own_code", "members_not_in_pair_order"], dedup_length=4, passes="single", named=False)
    return [named, chars]


# ---- W: the wrapped count
W_SIZES = (32767, 32768, 65537)
W_QUALS = {32767: "$", 32768: ";", 65537: "$"}


def _w_reads(m, early_a=False):
    reads = []
    for i in range(m):
        last = i >= m - 2
        b, q = ("ACGTA", "IIII$") if last or (early_a and i == 1) else ("ACGTN", "IIIII")
        reads.append(("w%d/1" % i, b, q))
        reads.append(("w%d/2" % i, "TTGCA", "IIIII"))
    return reads


def W(sizes=W_SIZES, variant=True):
    """One group of m pair records of 5-base reads.  Position 4 of side 1: N at Q40 from all but the last two members, who show A
    at Q3 (probability p).  The A sum is 2 p, `top` is p, and getA answers `top` if top < 2 p * count: with count 32 767 or 1
    (65 537 as a short, or as an int) that holds, quality 3; with count -32 768 it does not, and the sum 2 p gives quality 26.
    So 32 768 tells a short from anything wider, and 32 767 and 65 537 hold the two neighbours of the wrap in place."""
    cases = [_case("W-%d" % m, _w_reads(m), ["count_is_int"] if m == 32768 else []) for m in sizes]
    if variant:          # member 1 shows A at Q3 as well: the N of the 32 765 others has to count for the wrap to fall here (3 p: quality 40)
        cases.append(_case("W-32768-early-A", _w_reads(32768, True), ["count_is_int"]))
    return cases


# ---- F: flips, sides and names
F_SIZES = (2, 9, 10, 99, 100, 999, 1000)
F_NAME_LENGTHS = (1, 63, 64, 65, 200)


def F():
    rng = random.Random(21)
    cases = []
    # mode 2: members alternate (A, B) and (B, A); the two sides differ in length and quality; one group begins with a flipped member
    reads = []
    for f in range(4):
        a, b = _rnd(rng, 8), _rnd(rng, 8)
        for m in range(4):
            x = (a + _rnd(rng, 3 + m + 60 * (f % 2)), 25 + m)
            y = (b + _rnd(rng, 9 - m), 38 - 3 * m)
            if (m + f) % 2:
                x, y = y, x
            reads.append(("f%d-%d/1" % (f, m), x[0], _q(len(x[0]), q=x[1])))
            reads.append(("f%d-%d/2" % (f, m), y[0], _q(len(y[0]), q=y[1])))
    cases.append(_case("F-flips", reads, ["flip_sides_not_swapped", "name_of_unflipped_first_read", "members_not_in_pair_order"], dedup_mode=2, dedup_length=8))
    # names: a group of two single reads per name, the first member carrying it; Casava pairs under both store_comment settings
    for sc in (1, 0):
        reads = []
        names = ["b%d blank and more" % sc, "t%d\ttab and more" % sc, "bt%d \tboth" % sc, "tb%d\t both" % sc] + [("n%03d" % n).ljust(n, "x")[-n:] for n in F_NAME_LENGTHS]
        for i, name in enumerate(names):
            w = _index_key(i, 8)
            reads.append((name, w + "AC", _q(10)))
            reads.append(("second%d" % i, w + "AC", _q(10)))
        for i in range(2):          # two Casava-1.8 pairs of one fragment
            reads.append(("cas%d 1:N:0:ACGT" % i, "GGCAT" + "A" * i, _q(5 + i)))
            reads.append(("cas%d 2:N:0:ACGT" % i, "TTCAG" + "C" * i, _q(5 + i)))
        cases.append(_case("F-names-comment%d" % sc, reads, ["name_cut_at_blank_only", "cutoff_three"], dedup_length=4, passes="both", store_comment=sc))
    # the member count's digits
    reads = []
    for g, m in enumerate(F_SIZES):
        for i in range(m):
            reads.append(("z%d-%d" % (g, i), _index_key(g, 8) + "ACGT"[i % 4], _q(9, q=30 + i % 10)))
    cases.append(_case("F-sizes", reads, ["count_digits_fixed", "cutoff_three"], dedup_length=4, passes="single"))
    # no names at all
    reads = [("", "ACGTACGT" + "ACG"[:i], _q(8 + i)) for i in (1, 3, 2)] + [("", "TTTTACGT", _q(8))]
    cases.append(_case("F-nameless", reads, ["count_digits_fixed"], dedup_length=4, passes="single", named=False))
    return cases


# ---- P: pair-list shapes and skips
def P():
    reads, disc = [], []

    def add(name, bases, d=0):
        reads.append((name, bases, _q(len(bases))))
        disc.append(d)
    for i in range(3):                                   # a plain group of three pairs
        add("p%d/1" % i, "ACGTAC"); add("p%d/2" % i, "GGCATT")
    for i, (d1, d2) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):          # every combination of flags on a pair
        add("d%d/1" % i, "ACGTAA", d1); add("d%d/2" % i, "GGCAAA", d2)
    add("ds/1", "ACG", 1); add("ds/2", "GGCATT")          # discarded and too short: counted as discarded, the test that comes first
    add("sd/1", "ACG"); add("sd/2", "GGCATT", 1)
    add("ss/1", "ACG"); add("ss/2", "GG")                 # both ends too short: one count
    add("s1/1", "ACX"); add("s1/2", "GGCATT")
    add("s2/1", "ACGTAC"); add("s2/2", "GGC")
    for i in range(3):                                   # half pairs on side 1 and on side 2, groups in the single pass
        add("h%d/1" % i, "TTGCAACGT" + "A" * i)
    for i in range(2):
        add("k%d/2" % i, "CCATGGTAC" + "C" * i)
    add("hd/1", "TTGCAACGT", 1); add("ks/2", "CCATGGT")   # a discarded one and a short one (the single window is 8 bases)
    for i in range(2):                                   # reads without a read number
        add("u%d" % i, "GATTACAGA")
    return [_case("P-shapes", reads, ["pair_short_counted_twice", "cutoff_three"], discarded=disc, dedup_length=4, passes="both"),
            _case("P-shapes-mode2", reads, ["pair_short_counted_twice", "cutoff_three"], discarded=disc, dedup_mode=2, dedup_length=4, passes="both")]


# ---- M: many groups
def M_groups(cus, sides):
    return 2 * 8 * cus * 4 // sides + 1


def M(cus=256):
    """More (group, side) tasks than two grids of dedup_consensus_kernel hold (8 x CUs blocks of four wavefronts): groups of two
    members of 8-base reads, the second members a whole batch behind the first and the keys in another order than the members"""
    cases = []
    for passes, sides in (("paired", 2), ("single", 1)):
        G_ = M_groups(cus, sides)
        assert G_ <= 65536
        keys = [_index_key((g * 7919) % 65536, 8) for g in range(G_)]
        reads = []
        for m in range(2):
            for g, k in enumerate(keys):
                tail = "ACGT"[(g + m) % 4] * 4
                if sides == 2:
                    reads.append(("m%d-%d/1" % (g, m), k[:4] + tail, "IIII" + chr(33 + 3 + g % 38) * 4))
                    reads.append(("m%d-%d/2" % (g, m), revcomp(k[4:]) + tail, "IIII" + chr(33 + 40 - g % 38) * 4))
                else:
                    reads.append(("m%d-%d" % (g, m), k, "IIII" + chr(33 + 3 + (g + m) % 38) * 4))
        cases.append(_case("M-%s" % passes, reads, ["groups_in_key_order", "members_not_in_pair_order", "cutoff_three"], dedup_length=4, passes=passes))
    return cases


@functools.lru_cache(maxsize=None)
def family(name, *args):
    return {"G": G, "K": K, "Q": Q, "D": D, "S": S, "W": W, "F": F, "P": P, "M": M}[name](*args)
