"""Directed batches for the selection and its output text: what tests/test_select_cases.py proves on the CPU to reach every rule of
tests/refselect.py, and what tests/test_gpu_select_edges.py sends through kmr_select_reads and kmr_partition_reads.  No spectrum is
built: the trims, scores, artifact results, bimodal words and mates are host arrays, as the entry points take them.

A case is a dict: label; kind ("fastq", "fasta": the text the batch is ingested from, or "arrays": kmr_reads_from_host, no names);
reads = [(name line, bases, qualities)] as refselect takes them; mate (None = none given); use_mate (False: pickAllPassingReads
over a selector that has mates); af = (action, min_pass, max_pass) or None; to, tl, sc, wt; words (bimodal) or None; cfg (refselect.select's);
rules = the names of refselect.RULES the case is written to notice."""
import functools

import numpy as np

import refselect

FAMILIES = ("L", "S", "B", "G", "C", "Q", "P")
SCORINGS = ("SUM", "MEDIAN", "MIN", "MAX", "AVG")          # kmr_scoring's order
F = np.float32
U32MAX = 4294967295
# every decimal width 1 .. 10 at both ends
WIDTHS = (0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999,
          1000000000, U32MAX)
NAME_LENGTHS = (1, 62, 63, 64, 65, 127, 128, 200)
HEADER_NAME_LENGTHS = (47, 48, 49, 50)          # with the 14-byte label " MedianScore:5": the header's newline on lanes 62, 63, 0, 1
LANES = (0, 1, 62, 63)


def _bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def _quals(rng, n, base):
    return bytes((base + 2 + rng.integers(0, 39, n)).astype(np.uint8))          # inside [base, base + 40]: the base detection leaves the batch alone


def _name(i, length):
    s = b"r%d" % i
    return (s + b"x" * length)[:length] if length >= len(s) else bytes([ord("a") + i % 26]) * length


def config(**kw):
    cfg = dict(min_score=2.0, min_read_length=0.4, both_pass=False, scoring=1, in_base=33, out_base=33, fasta=False, input_starts=None)
    assert set(kw) <= set(cfg)
    cfg.update(kw)
    return cfg


def make(label, reads, rules, kind="fastq", mate=None, use_mate=True, af=None, to=None, tl=None, sc=None, wt=None, words=None, **cfg):
    n = len(reads)
    u32 = lambda a, d: np.array(d if a is None else a, dtype=np.uint32)
    case = dict(label=label, kind=kind, reads=reads, rules=tuple(rules), use_mate=use_mate,
                mate=None if mate is None else np.array(mate, dtype=np.int64),
                af=None if af is None else (np.array(af[0], np.uint8), np.array(af[1], np.uint32), np.array(af[2], np.uint32)),
                to=u32(to, [0] * n), tl=u32(tl, [len(r[1]) for r in reads]), sc=np.array([5.0] * n if sc is None else sc, dtype=np.float32),
                wt=np.array([0] * n if wt is None else wt, dtype=np.uint8), words=None if words is None else np.array(words, dtype=np.uint64), cfg=config(**cfg))
    assert all(len(a) == n for a in (case["to"], case["tl"], case["sc"], case["wt"])) and all(len(r[1]) == len(r[2]) for r in reads)
    assert set(rules) <= set(refselect.RULES)
    return case


def text_of(case):
    """the text a "fastq" or "fasta" case is ingested from (its names point into it); b"" for arrays"""
    if case["kind"] == "fastq":
        return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in case["reads"])
    if case["kind"] == "fasta":
        return b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in case["reads"])
    return b""


def run(case, wrong=None, input_starts=False):
    """the restatement's answer; input_starts False: one input whatever the case says (what kmr_select_reads computes)"""
    cfg = dict(case["cfg"])
    if not input_starts:
        cfg["input_starts"] = None
    return refselect.select(case["reads"], case["mate"] if case["use_mate"] else None, case["af"], case["to"], case["tl"], case["sc"], case["wt"], case["words"], cfg, wrong)


def signature(res):
    return res.text, res.picked.tobytes(), res.n_picked, res.bytes, tuple(res.table), res.read_segment.tobytes()


def _plain(rng, n, length, base=33, first=0):
    return [(b"r%d" % (first + i), _bases(rng, length), _quals(rng, length, base)) for i in range(n)]


def _beside_a_passing_mate(rng, reads, base=33):
    """every read followed by a plain read that passes: with both_pass off the pair is picked whatever the first read does"""
    out, mate = [], []
    for i, r in enumerate(reads):
        out += [r, (b"m%d" % i, _bases(rng, 12), _quals(rng, 12, base))]
        mate += [2 * i + 1, 2 * i]
    return out, mate


def _spread(values, n, fill):
    """`values` for the even reads (the reads under test), `fill` for their mates"""
    out = []
    for v in values:
        out += [v, fill]
    assert len(out) == n
    return out


# ---- L: passesLength
def _L():
    rng = np.random.default_rng(11)
    cases = []

    def one(label, mrl, shapes, rules):
        reads = [(b"l%d" % i, _bases(rng, L), _quals(rng, L, 33)) for i, (L, _) in enumerate(shapes)]
        cases.append(make("L-" + label, reads, rules, tl=[t for _, t in shapes], wt=[1] * len(shapes), min_read_length=float(F(mrl))))

    one("0.1", 0.1, [(150, 14), (150, 15), (150, 16), (149, 15), (151, 15)], ("product_in_double", "fraction_strict"))
    one("0.6", 0.6, [(150, 89), (150, 90), (150, 91), (149, 90), (151, 90)], ("product_in_double", "fraction_strict"))
    one("0.4", 0.4, [(5, 1), (5, 2), (5, 3), (4, 2), (6, 2), (2, 2), (1, 1)], ("product_in_double", "fraction_strict"))
    one("one", 1.0, [(150, 149), (150, 150), (2, 2), (2, 1), (1, 1), (3, 2)], ("fraction_strict",))
    one("above-one", np.nextafter(F(1.0), F(2.0)), [(150, 149), (150, 2), (150, 1), (2, 2), (1, 1)], ())
    one("25", 25.0, [(150, 24), (150, 25), (150, 26), (25, 25), (24, 24)], ("absolute_strict",))
    one("zero", 0.0, [(150, 0), (150, 1), (150, 2), (2, 2), (1, 1), (1, 0)], ())
    return cases


# ---- S: the score's threshold and its rounding
ROUNDING = (2.5, 2.4999998, 0.49999997, -0.4, -0.6, -1.0, 0.5, 1.5, 3.5, 0.0, 7.4, 65535.0)


def _S():
    rng = np.random.default_rng(12)
    cases = []
    t = F(2.5)
    sc = [np.nextafter(t, F(0.0)), t, np.nextafter(t, F(9.0)), -1.0, float("nan"), 3e38, -3e38, float("inf"), float("-inf")]
    cases.append(make("S-threshold", _plain(rng, len(sc), 20), ("score_strict",), sc=sc, min_score=2.5))
    # the same scores beside a passing mate: all are printed, the NaN and the huge ones under the project's own rule
    reads, mate = _beside_a_passing_mate(rng, _plain(rng, len(sc), 20))
    cases.append(make("S-pinned", reads, (), mate=mate, sc=_spread(sc, len(reads), 5.0), min_score=2.5))
    for s, name in enumerate(SCORINGS):
        cases.append(make("S-round-" + name, _plain(rng, len(ROUNDING), 20), ("score_truncates", "score_half_even", "score_half_in_float"),
                          sc=ROUNDING, scoring=s, min_score=-5.0))
    return cases


# ---- B: labels
MEANS = ((0, 1), (1, 0), (1, 1), (0, 65535), (65535, 0), (65535, 65535), (1, 65535), (65535, 1), (0, 0))
LONGEST = dict(af=(U32MAX, 0), word=U32MAX | (10000 << 32) | (65535 << 48), to=U32MAX, tl=U32MAX, sc=-2147483648.0)


def _B(cus=256):
    rng = np.random.default_rng(13)
    cases = []
    n = len(WIDTHS)
    reads, mate = _beside_a_passing_mate(rng, _plain(rng, 2 * n, 40))
    # max_pass - min_pass of every width and both signs: first min + d, then min - d as the smaller of the two
    lo = list(WIDTHS) + [WIDTHS[j] + WIDTHS[n - 1 - j] for j in range(n)]
    hi = [WIDTHS[j] + WIDTHS[n - 1 - j] for j in range(n)] + list(WIDTHS)
    assert max(lo + hi) <= U32MAX
    to = list(WIDTHS) + list(reversed(WIDTHS))
    tl = list(reversed(WIDTHS)) + list(WIDTHS)
    sc = [float(min(v, 2147483000)) for v in WIDTHS] + [-float(min(v, 2147483000)) for v in WIDTHS]
    words = [WIDTHS[j % n] | (MEANS[j % 9][0] << 32) | (MEANS[j % 9][1] << 48) for j in range(2 * n)]
    words[n - 1] = U32MAX | (1 << 32) | (1 << 48)          # equal means on a word that is not 0
    m = len(reads)
    for s, name in enumerate(SCORINGS):
        cases.append(make("B-widths-" + name, reads, ("aftrim_unsigned", "inv_on_equal", "label_parts_swapped"), mate=mate,
                          af=(_spread([1] * (2 * n), m, 0), _spread(lo, m, 0), _spread(hi, m, 0)), to=_spread(to, m, 0), tl=_spread(tl, m, 12),
                          sc=_spread(sc, m, 5.0), wt=_spread([1] * (2 * n), m, 0), words=_spread(words, m, 0), scoring=s, min_read_length=0.0))
    # The writer deals pick p to wavefront p mod (its grid's wavefronts): select_writer (kmr_stages.hip) launches
    # min(ceil(picks / SEL_WAVES), 8 x CUs) blocks of SEL_WAVES = 4 wavefronts.  G picks with the longest label, then G with a one-part
    # label: every wavefront writes a short label into the LDS bytes that held a long one.  This is the one case above a few hundred
    # reads; tests/test_select_cases.py holds the launch to that formula, so the size cannot go stale unnoticed.
    G = 4 * 8 * cus
    long_read, short_read = (b"a", b"ACGTAC", b"IIIIII"), (b"b", b"ACGTAC", b"555555")
    reads = [long_read] * G + [short_read] * G
    mate = [i + G for i in range(G)] + list(range(G))          # the long reads are masked (trim_off past the read) and ride on their mates
    X = LONGEST
    cases.append(make("B-longest", reads, (), mate=mate, af=([1] * G + [0] * G, [X["af"][0]] * G + [0] * G, [X["af"][1]] * G + [0] * G),
                      to=[X["to"]] * G + [0] * G, tl=[X["tl"]] * G + [6] * G, sc=[X["sc"]] * G + [5.0] * G, wt=[1] * G + [0] * G,
                      words=[X["word"]] * G + [0] * G))
    return cases


# ---- G: the record's sections against the wavefront's 64 lanes
def _G():
    rng = np.random.default_rng(14)
    shapes = [(1, bl) for bl in range(2, 66)] + [(2, bl) for bl in range(2, 66)]
    shapes += [(nl, bl) for nl in NAME_LENGTHS + HEADER_NAME_LENGTHS for bl in (2, 37)]
    cases = []
    for label, in_base, out_base, fasta in (("33-33", 33, 33, False), ("33-64", 33, 64, False), ("64-33", 64, 33, False), ("64-64", 64, 64, False), ("fasta", 33, 33, True)):
        reads, to, tl = [], [], []
        for i, (nl, bl) in enumerate(shapes):
            name = _name(i, nl)
            line = name + (b"", b" c x", b"\tc x", b"\tc x y", b" c\tx")[i % 5]          # the name ends at the line's end, a blank, a tab
            reads.append((line, _bases(rng, bl + 3), _quals(rng, bl + 3, in_base)))
            to.append(i % 3)
            tl.append(bl)
        rules = ("name_ends_at_blank_only",) + (("shift_wrong_sign",) if in_base != out_base else ())
        cases.append(make("G-" + label, reads, rules, to=to, tl=tl, in_base=in_base, out_base=out_base, fasta=fasta, min_read_length=0.0))
    return cases


# ---- C: slice clamps and masks
def _C():
    rng = np.random.default_rng(15)
    L = 30
    shapes = [(L - 1, 5), (L, 5), (L + 5, 5), (10, 21), (0, L + 1), (0, 0), (3, 0), (0, 1), (7, 1), (0, 2), (L - 2, 2), (L - 2, 3), (L - 1, 1), (U32MAX, 2), (2, U32MAX)]
    n = len(shapes)
    under_test = _plain(rng, n + 1, L)
    reads, mate = _beside_a_passing_mate(rng, under_test)
    act = _spread([0] * n + [2], len(reads), 0)          # the last read under test was discarded by the artifact filter
    # two pairs nobody picks: both reads masked by their trims; one discarded beside one trimmed to a base
    reads += _plain(rng, 4, L, first=100)
    k = len(reads)
    mate += [k - 3, k - 4, k - 1, k - 2]
    act += [0, 0, 2, 0]
    to = _spread([s[0] for s in shapes] + [0], 2 * (n + 1), 0) + [0, 0, 0, 0]
    tl = _spread([s[1] for s in shapes] + [L], 2 * (n + 1), 12) + [1, 0, L, 1]
    cases = []
    for label, out_base, fasta in (("33-33", 33, False), ("33-64", 33 + 31, False), ("fasta", 33, True)):
        rules = ("mask_at_zero", "no_slice_clamp") + (("masked_qual_from_input_base",) if out_base != 33 else ())
        cases.append(make("C-" + label, reads, rules, mate=mate, af=(act, [0] * k, [0] * k), to=to, tl=tl, wt=[1] * k, out_base=out_base, fasta=fasta, min_read_length=0.0))
    return cases


# ---- Q: reads without qualities (Read::REF_QUAL)
def _Q():
    rng = np.random.default_rng(16)
    cases = []
    R = refselect.REF_QUAL
    # from FASTA text: every quality is 127
    lengths = (2, 3, 40, 63, 64, 65, 130, 1)
    reads = [(b"contig%d c" % i, _bases(rng, L), bytes([R]) * L) for i, L in enumerate(lengths)]
    to = [0, 1, 5, 0, 0, 1, 64, 0]
    tl = [2, 2, 30, 63, 64, 64, 66, 1]
    for in_base, out_base in ((33, 33), (33, 64), (64, 33)):
        cases.append(make("Q-fasta-%d-%d" % (in_base, out_base), reads, ("ref_qual_shifted",), kind="fasta", to=to, tl=tl, wt=[1] * len(reads),
                          in_base=in_base, out_base=out_base, min_read_length=0.0))
    # from arrays: 127 first and real qualities behind it; real first and 127 behind; a slice that starts on a 127 inside a read
    # that has qualities, and one that ends on it; a read all real; a read of one base
    L = 20
    real = lambda n: _quals(rng, n, 33)
    quals = [bytes([R]) + real(L - 1), bytes([R]) + real(L - 1), real(1) + bytes([R]) * (L - 1), real(8) + bytes([R]) + real(L - 9), real(8) + bytes([R]) + real(L - 9),
             real(8) + bytes([R]) + real(L - 9), real(L), bytes([R]), bytes([R, R]), real(1) + bytes([R])]
    to = [0, 4, 0, 8, 2, 9, 0, 0, 0, 0]
    tl = [L, 10, L, 6, 7, 5, L, 1, 2, 2]
    reads = [(b"", _bases(rng, len(q)), q) for q in quals]
    for out_base in (33, 64):
        cases.append(make("Q-arrays-33-%d" % out_base, reads, ("ref_qual_shifted", "ref_qual_every_byte"), kind="arrays", to=to, tl=tl, wt=[1] * len(reads),
                          out_base=out_base, min_read_length=0.0))
    return cases


# ---- P: pairs, singles and inputs
def _P():
    rng = np.random.default_rng(17)
    n = 14
    reads = _plain(rng, n, 20)
    #        0  1  2  3  4  5  6  7   8   9  10  11  12  13
    mate = [1, 0, 3, 2, 5, 4, 7, 6, -1, -1, 13, 12, 11, 10]
    ok = [1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0]          # which read passes (a failing one: a trim of 3 of 20 bases)
    tl = [20 if p else 3 for p in ok]
    wt = [0 if p else 1 for p in ok]
    cases = []
    for label, both in (("either", False), ("both", True)):
        rules = ("both_pass_as_either",) if both else ("failed_mate_left_out",)          # under both_pass no picked pair has a failing read
        cases.append(make("P-" + label, reads, rules, mate=mate, tl=tl, wt=wt, both_pass=both))
        cases.append(make("P-" + label + "-two-inputs", reads, rules, mate=mate, tl=tl, wt=wt, both_pass=both, input_starts=[0, 5, n]))
    cases.append(make("P-reads", reads, (), mate=mate, use_mate=False, tl=tl, wt=wt, both_pass=True))
    # in another output format writePicks selects again: still without the mates
    cases.append(make("P-reads-base64", reads, (), mate=mate, use_mate=False, tl=tl, wt=wt, both_pass=True, out_base=64))
    cases.append(make("P-reads-three-inputs", reads, (), mate=mate, use_mate=False, tl=tl, wt=wt, input_starts=[0, 0, 5, n]))
    return cases


@functools.lru_cache(maxsize=None)
def family(name, cus=256):
    return {"L": _L, "S": _S, "G": _G, "C": _C, "Q": _Q, "P": _P}[name]() if name != "B" else _B(cus)
