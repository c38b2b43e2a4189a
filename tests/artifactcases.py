"""Directed reads for the artifact filter (FilterKnownOddities): every threshold, tie, wrap and border of applyFilterToRead /
recordAffectedRead and of the device kernels that restate them (artifact_screen, artifact_action, artifact_gather), as families
of small deterministic batches.  tests/test_artifact_cases.py proves on the CPU that the families hold what they are meant to
hold and would notice each deliberate deviation of tests/refartifact.py; tests/test_gpu_artifact_edges.py runs them on the device.

The FASTA table is made here (nothing of the reference's tables): three adapters, two of them two substitutions apart, a
sequence shorter than the match length, an all-A sequence of exactly the match length, two simple repeats, a stand-in PhiX and
a reference-class sequence, in the order the reference appends them, with the class ranges."""
import functools

import numpy as np

import refartifact as ra

GOOD, LOW = b"I", b"#"                                        # good and low at start char 33 and at 64, min quality 3


def lcg_bases(n, seed):
    x, out = seed, bytearray()
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        out.append(b"ACGT"[x >> 62])
    return bytes(out)


def revcomp(s):
    return bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def other(base, step=1):
    """another base than `base` (a byte value), deterministic"""
    return b"ACGT"[(b"ACGT".index(bytes((base,)).upper()) + step) % 4]


BG = lcg_bases(8192, 1)
AD_A = lcg_bases(50, 11)
NEAR = (20, 30)                                               # where adapter_b differs from adapter_a
AD_B = bytearray(AD_A)
for _p in NEAR:
    AD_B[_p] = other(AD_A[_p], 2)
AD_B = bytes(AD_B)
AD_C = lcg_bases(41, 13)
SHORT_SEQ = lcg_bases(10, 17)
POLY_A = b"A" * 24
REP_AC, REP_AAT = b"AC" * 20, b"AAT" * 14
PHIX = lcg_bases(120, 19)
REFERENCE = lcg_bases(90, 23)
TABLE = [(b"adapter_a", AD_A), (b"adapter_b", AD_B), (b"adapter_c", AD_C), (b"short", SHORT_SEQ), (b"poly_a", POLY_A),
         (b"repeat_ac", REP_AC), (b"repeat_aat", REP_AAT), (b"phix", PHIX), (b"reference", REFERENCE)]
FASTA = b"".join(b">" + n + b" made for the tests\n" + s[:30] + b"\n" + s[30:] + b"\n" for n, s in TABLE)
IDX = {n: i + 1 for i, (n, _) in enumerate(TABLE)}
N_SEQ = len(TABLE) + 1
CLASSES = dict(simple_repeat_begin=6, simple_repeat_end=8, phix_idx=8, reference_begin=9)


def bg(n, k):
    at = (k * 37) % (len(BG) - 160)
    return BG[at:at + n]


class Batch:
    def __init__(self):
        self.seqs, self.quals, self.tags, self.mate, self.names = [], [], [], None, None

    def add(self, seq, qual, tag=""):
        assert len(seq) == len(qual)
        self.seqs.append(bytes(seq))
        self.quals.append(bytes(qual))
        self.tags.append(tag)
        return len(self.seqs) - 1

    @property
    def n(self):
        return len(self.seqs)

    def arrays(self):
        """bases, quals, offsets as the device takes them; the last read ends where the arrays end"""
        off = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        return np.frombuffer(b"".join(self.seqs), dtype=np.uint8).copy(), np.frombuffer(b"".join(self.quals), dtype=np.uint8).copy(), off

    def fastq(self):
        return b"".join(b"@" + nm + b"\n" + s + b"\n+\n" + q + b"\n" for nm, s, q in zip(self.names, self.seqs, self.quals))


def quals(n, low_prefix=0, low_suffix=0, low_at=()):
    q = bytearray(GOOD * n)
    q[:low_prefix] = LOW * min(low_prefix, n)
    if low_suffix:
        q[n - low_suffix:] = LOW * low_suffix
    for i in low_at:
        q[i] = LOW[0]
    return bytes(q)


def planted(L, k, piece, at):
    s = bytearray(bg(L, k))
    s[at:at + len(piece)] = piece
    assert len(s) == L
    return bytes(s)


# ------------------------------------------------------------------------------------------------------------------- runs
RUN_MIN_LENGTHS = (0.0, 0.40, 0.5, 0.85, 1.0, 2.0, 25.0)


def runs_batch(kw):
    """every mask of low-quality positions for every length 0..12, and runs at, below and above L * min_read_length for L = 5, 10,
    .. 150 (the same reads at every min_read_length); no table"""
    b = Batch()
    for L in range(13):
        for mask in range(1 << L):
            b.add(bg(L, mask), bytes(LOW[0] if (mask >> i) & 1 else GOOD[0] for i in range(L)), "mask")
    k = 0
    for L in range(5, 151, 5):
        for m in (0.40, 0.5, 0.85, 1.0):
            t = int(L * m + 1e-9)
            for r in sorted({t - 1, t, t + 1, t + 2}):
                if r < 2 or r > L:
                    continue
                k += 1
                b.add(bg(L, k), quals(L, low_suffix=L - r), "pin-best")
                b.add(bg(L, k), quals(L, low_prefix=L - r), "pin-best-end")
                if L - r - 1 > r:
                    b.add(bg(L, k), quals(L, low_at=(L - r - 1,)), "pin-second")
    return b


# ---------------------------------------------------------------------------------------------------------- quality bytes
QUALITY_CONFIGS = [dict(fastq_start_char=33, min_quality=3), dict(fastq_start_char=64, min_quality=3),
                   dict(fastq_start_char=33, min_quality=100), dict(fastq_start_char=64, min_quality=66)]      # 133 and 130: above 127


def quality_batch(kw):
    thr = (kw["fastq_start_char"] + kw["min_quality"]) & 0xff
    special = [thr, (thr - 1) & 0xff, (thr + 1) & 0xff, 0x7f, 0x80, 0xff]
    b, k = Batch(), 0
    for L in (30, 31):
        for x in special:
            for at in (0, 7, 15, L - 1):
                k += 1
                q = bytearray(b"\x7e" * L)                    # 126: not below any of the thresholds, signed or not
                q[at] = x
                b.add(bg(L, k), q, "one")
        for x in special:
            for y in special:
                k += 1
                q = bytearray(b"\x7e" * L)
                q[10], q[20] = x, y
                b.add(planted(L, k, AD_C[:24], 4) if k % 3 == 0 else bg(L, k), q, "two")
    return b


# ---------------------------------------------------------------------------------------------------------------- windows
def windows_batch(kw):
    """an exact piece of adapter_a at every start of reads of match length .. match length + 9 and 76..79 bases, with good
    qualities, a low prefix of 1..9 (minPass % 4 takes every value: the pointer quirk) and a low suffix of 1..9 (maxPass and the hops)"""
    M = kw.get("match_length", 24)
    piece = (AD_A + AD_A)[3:3 + M]
    b, k = Batch(), 0
    for L in list(range(M, M + 10)) + [76, 77, 78, 79]:
        for s in range(L - M + 1):
            k += 1
            seq = planted(L, k, piece, s)
            b.add(seq, quals(L), "good")
            for p in range(1, 10):
                b.add(seq, quals(L, low_prefix=p), "prefix")
                b.add(seq, quals(L, low_suffix=p), "suffix")
    return b


# ------------------------------------------------------------------------------------------------------------------ sides
def sides_batch(kw):
    b, k = Batch(), 0
    piece = AD_C[:24]
    for L in (64, 65, 66, 67, 80):
        for p in (0, 1, 2, 3, 4, 5, 6, 7, 9, 16, 21):
            for u in (0, 1, 2, 3, 5, 12):
                for s in range(0, L - 24 + 1, 4):
                    k += 1
                    b.add(planted(L, k, piece, s), quals(L, low_prefix=p, low_suffix=u), "grid")
    for L in range(32, 112, 8):                               # the hit exactly in the middle: left == right
        k += 1
        b.add(planted(L, k, piece, (L - 24) // 2), quals(L), "tie")
        b.add(planted(L, k, piece, (L - 24) // 2 + 4), quals(L), "tie+4")
        b.add(planted(L, k, piece, (L - 24) // 2 - 4), quals(L), "tie-4")
    for L in range(24, 51):                                   # the read is adapter from end to end: the hits cover the pass range
        for p in (0, 1, 5):
            b.add((AD_A + AD_A)[:L], quals(L, low_prefix=p), "whole")
    for L in (28, 32, 36):                                    # ... and reach over both of its ends
        for p in (1, 2, 3):
            for u in (1, 2, 3):
                b.add((AD_A + AD_A)[:L], quals(L, low_prefix=p, low_suffix=u), "astride")
    for s in range(0, 41, 4):                                 # hits of several windows in a row
        k += 1
        b.add(planted(80, k, (AD_A + AD_A)[7:47], s), quals(80), "long-piece")
    return b


# ------------------------------------------------------------------------------------------------------------------ edits
def _fwd_is_least(w):
    c = ra.compress_sequence(w)
    return ra.least_complement(c) == c


@functools.lru_cache(maxsize=None)
def strand_flips():
    """(window of an adapter, position, base): one substitution after which the other strand is the canonical one -- the
    reference permutes the canonical query without re-canonicalising and so cannot reach the stored key"""
    out = []
    flt = ra.Filter(ra.Config(edit_distance=1, build_edits=0), FASTA)
    for name, seq in TABLE[:3]:
        circ = seq + seq[:24]
        for j in range(0, len(seq), 3):
            x = circ[j:j + 24]
            if ra.compress_sequence(x) == ra.compress_sequence(revcomp(x)):
                continue
            for pos in (0, 23, 1, 22):
                for step in (1, 2, 3):
                    w = bytearray(x)
                    w[pos] = other(x[pos], step)
                    if _fwd_is_least(bytes(w)) != _fwd_is_least(x) and not flt.screen(bytes(w), quals(24))["hits"]:
                        out.append((x, pos, w[pos]))          # (a few flips are still found: by way of a neighbouring window or of adapter_b)
    assert len(out) >= 20, len(out)
    return out[:60]


def edits_batch(kw):
    """query-time edits (build_edits = 0): reads of 36 bases with the piece at base 4 (the second window)"""
    ed = kw["edit_distance"]
    thin = 1 if ed == 1 else 3
    b, k = Batch(), 0
    flt = ra.Filter(ra.Config(edit_distance=1, build_edits=0), FASTA)
    x = (AD_A + AD_A)[31:55]                                  # clear of the two places where adapter_b differs

    def put(piece, tag):
        nonlocal k
        k += 1
        b.add(planted(36, k, piece, 4), quals(36), tag)

    put(x, "exact")
    put(revcomp(x), "exact-rc")
    n = 0
    for pos in range(24):
        for step in (1, 2, 3):
            n += 1
            if n % thin:
                continue
            w = bytearray(x)
            w[pos] = other(x[pos], step)
            put(w, "one")
            put(revcomp(w), "one-rc")
    for p1, p2 in ((0, 23), (0, 1), (11, 12), (22, 23), (3, 17), (5, 20), (8, 9), (2, 13)):
        for s1, s2 in ((1, 1), (2, 3)):
            w = bytearray(x)
            w[p1], w[p2] = other(x[p1], s1), other(x[p2], s2)
            put(w, "two")
            put(revcomp(w), "two-rc")
    w = bytearray(x)
    for pos in (1, 12, 22):
        w[pos] = other(x[pos], 1)
    flt2 = ra.Filter(ra.Config(edit_distance=2, build_edits=0), FASTA)
    for piece, tag in ((bytes(w), "three"), (revcomp(w), "three-rc")):
        k += 1
        while flt2.screen(planted(36, k, piece, 4), quals(36))["hits"]:      # the windows beside the piece hold two of the three
            k += 1
        k -= 1
        put(piece, tag)
    for i, (xw, pos, base) in enumerate(strand_flips()):
        if i % (1 if ed == 1 else 3) == 0:
            w = bytearray(xw)
            w[pos] = base
            k += 1
            while flt.screen(planted(36, k, w, 4), quals(36))["hits"]:      # background that leaves the windows beside the piece out of reach
                k += 1
            k -= 1
            put(w, "flip")
    for j in range(NEAR[1] - 23, NEAR[0] + 1):                # windows of adapter_a that cover both places where adapter_b differs
        for which in (0, 1):
            if (j + which) % (1 if ed == 1 else 3):
                continue
            w = bytearray(AD_A[j:j + 24])
            w[NEAR[which] - j] = AD_B[NEAR[which]]            # one substitution from adapter_a and one from adapter_b
            put(w, "near")
            put(revcomp(w), "near-rc")
    return b


# ---------------------------------------------------------------------------------------------------------------- classes
def classes_batch(kw):
    b, k = Batch(), 0
    for p in range(5):
        for r0 in range(34, 43):
            for g in range(34, 43):
                for u in range(5):
                    k += 1
                    rep = (REP_AC if k % 2 else REP_AAT)[:30]
                    L = r0 + 30 + g
                    b.add(planted(L, k, rep, r0), quals(L, low_prefix=p, low_suffix=u), "margin")
    ad, ac, px, rf = AD_C[3:27], REP_AC[:28], PHIX[10:40], REFERENCE[5:35]
    for d in range(8):
        k += 1
        s = bytearray(bg(160, k))
        s[40:64], s[72 + d:100 + d] = ad, ac
        b.add(s, quals(160), "adapter-then-repeat")          # the repeat is the last hit: both are forgiven
        s = bytearray(bg(160, k))
        s[72:100], s[108 + d:135 + d] = ac, AD_C[3:30]        # 27 bases: a window on a 4-base border at any d
        b.add(s, quals(160), "repeat-then-adapter")
        s = bytearray(bg(160, k))
        s[20 + d:50 + d], s[100:124] = px, ad
        b.add(s, quals(160), "phix-then-adapter")
        s = bytearray(bg(160, k))
        s[20 + d:50 + d], s[80:108] = px, ac
        b.add(s, quals(160), "phix-then-repeat")
        s = bytearray(bg(160, k))
        s[60:88], s[120 + d:150 + d] = ac, px
        b.add(s, quals(160), "repeat-then-phix")
        b.add(planted(100, k, rf, 32 + d), quals(100), "reference")
        b.add(planted(100, k, REFERENCE[-14:] + REFERENCE[:13], 32 + d), quals(100), "reference-wrap")      # not circularised: no hit
        b.add(planted(100, k, AD_C[-14:] + AD_C[:13], 32 + d), quals(100), "adapter-wrap")
        b.add(bg(100, k), quals(100, low_at=(40 + d,)), "quality-only")                                      # value == nSeq is no reference hit
        b.add(planted(100, k, SHORT_SEQ + SHORT_SEQ + SHORT_SEQ, 32 + d), quals(100), "short-sequence")      # has no window of its own
    return b


# ------------------------------------------------------------------------------------------------------------------ pairs
KINDS = ("clean", "quality", "adapter", "repeat", "phix", "reference")


def kind_read(kind, k):
    L = 100
    if kind == "clean":
        return bg(L, k), quals(L)
    if kind == "quality":
        return bg(L, k), quals(L, low_at=((45 if k % 2 else 60),))
    piece, at = {"adapter": (AD_C[3:27], 72), "repeat": (REP_AC[:26], 36), "phix": (PHIX[10:40], 20), "reference": (REFERENCE[5:35], 32)}[kind]
    return planted(L, k, piece, at), quals(L)


def pairs_batch(kw):
    b, k = Batch(), 0
    combos = [(x, y) for x in KINDS for y in KINDS]
    mate = []
    for x, y in combos[:18]:                                  # mates next to each other, a single of every kind mixed in
        k += 2
        i = b.add(*kind_read(x, k), tag=x + "|" + y)
        b.add(*kind_read(y, k + 1), tag=y + "|" + x)
        mate += [i + 1, i]
        if len(mate) % 6 == 0:
            b.add(*kind_read(KINDS[(len(mate) // 6) % 6], k), tag=KINDS[(len(mate) // 6) % 6] + "|")
            mate.append(-1)
    first = b.n
    rest = combos[18:]
    for x, y in rest:                                         # first reads in one block, second reads in the next
        k += 1
        b.add(*kind_read(x, k), tag=x + "|" + y)
        mate.append(first + len(rest) + len(mate) - first)
    for j, (x, y) in enumerate(rest):
        k += 1
        b.add(*kind_read(y, k), tag=y + "|" + x)
        mate.append(first + j)
    for x in KINDS:
        k += 1
        b.add(*kind_read(x, k), tag=x + "|")
        mate.append(-1)
    b.mate = np.array(mate, dtype=np.int64)
    assert b.mate.size == b.n and all(m < 0 or b.mate[m] == i for i, m in enumerate(mate))
    return b


# ------------------------------------------------------------------------------------------------------------------ short
def short_batch(kw):
    """reads of 0..24 bases with a low prefix of 0..5: the hop clamp, windows that reach past the read's bytes (zeros decide:
    the table has an all-A sequence), and short reads between reads that begin and end with artifact bases"""
    b, k = Batch(), 0
    for L in range(25):
        for p in range(min(5, L) + 1):
            k += 1
            a = bytearray(b"A" * L)
            b.add(a, quals(L, low_prefix=p), "poly-a")
            if L >= 1:
                a1 = bytearray(a)
                a1[L // 2] = ord("C")
                b.add(a1, quals(L, low_prefix=p), "poly-a-1")
            if L >= 2:
                a2 = bytearray(a)
                a2[0], a2[L - 1] = ord("G"), ord("T")
                b.add(a2, quals(L, low_prefix=p), "poly-a-2")
            b.add(bg(L, k), quals(L, low_prefix=p), "random")
    x = AD_C[5:29]
    for n in range(1, 21):
        k += 1
        b.add(bg(30, k) + x[:12], quals(42), "before")
        b.add(x[:n], quals(n), "between")                     # with the next read's first bases behind it this would be a window of adapter_c
        b.add(x[n:] + bg(30, k + 1), quals(24 - n + 30), "after")
    return b


# ------------------------------------------------------------------------------------------------------------- characters
def characters_batch(kw):
    b, k = Batch(), 0
    x = AD_A[5:29]
    for piece, tag in ((x.lower(), "lower-piece"), (x[:12] + x[12:].lower(), "half-lower")):
        k += 1
        b.add(planted(60, k, piece, 20), quals(60), tag)
        b.add(planted(60, k, piece, 20).lower(), quals(60), tag + "-read")
    for i in range(24):
        for ch in b"N.Rn":
            k += 1
            w = bytearray(x)
            w[i] = ch
            b.add(planted(60, k, w, 20), quals(60), "in-A" if x[i] == ord("A") else "in-other")      # markup packs as A
    for at, ch in ((0, b"N"), (59, b"."), (19, b"Y"), (44, b"K"), (10, b"M"), (50, b"S"), (3, b"W"), (57, b"n"), (18, b"B"), (45, b"V")):
        k += 1
        s = bytearray(planted(60, k, x, 20))
        s[at] = ch[0]
        b.add(s, quals(60), "outside")
        b.add(s, quals(60, low_at=(at,)), "outside-low")
    b.add(b"N" * 40, quals(40), "all-N")                      # packs as all A: the all-A sequence
    b.add(b"." * 33, quals(33, low_prefix=2), "all-dot")
    return b


# ----------------------------------------------------------------------------------------------------------------- layout
def gather_reads(b):
    """kept lengths of 63, 64, 65, 127, 128, 129 as a trim behind a low prefix of 0..7 and as a remnant behind it"""
    k = 0
    for K2 in (63, 64, 65, 127, 128, 129):
        for p in range(8):
            k += 1
            L = p + (K2 + 1) + 1 + K2
            b.add(bg(L, k), quals(L, low_prefix=p, low_at=(p + K2 + 1,)), "gather")      # best run K2 + 1, remnant K2
            if p % 4 == 0:                                    # the adapter in the first window, booked at p: the K2 bases right of it stay
                L = p + 24 + K2
                b.add(planted(L, k, AD_C[3:27], 0), quals(L, low_prefix=p), "gather-right")


@functools.lru_cache(maxsize=None)
def _pool():
    w = windows_batch({})
    s = sides_batch({})
    b = Batch()
    for i in range(0, w.n, 17):                              # 19 variants of quality per start: 17 walks through all of them
        b.add(w.seqs[i], w.quals[i], w.tags[i])
    for i in range(s.n):
        if s.tags[i].startswith("tie") or s.tags[i] == "whole":
            b.add(s.seqs[i], s.quals[i], s.tags[i])
    return b


LAYOUTS = [("filler", f) for f in range(8)] + [("count", 255), ("count", 256), ("count", 257), ("gather", 0), ("names", 0)]


def layout_batch(kw, what, arg):
    pool = _pool()
    b = Batch()
    if what == "filler":                                      # every read start of the subset meets every address residue mod 8
        b.add(bg(arg, arg), quals(arg), "filler")
        for i in range(0, pool.n, 3):
            b.add(pool.seqs[i], pool.quals[i], pool.tags[i])
        gather_reads(b)
    elif what == "count":
        for i in range(arg):
            b.add(pool.seqs[i], pool.quals[i], pool.tags[i])
        if arg == 257:                                        # empty reads at the first, a middle and the last place
            for i in (0, 128, 256):
                b.seqs[i], b.quals[i], b.tags[i] = b"", b"", "filler"
    elif what == "gather":
        gather_reads(b)
    else:
        k = 0
        for x in KINDS:
            for _ in range(3):
                k += 1
                b.add(*kind_read(x, k), tag=x)
        gather_reads(b)
        b.names = [b"read_%d/%d kind=%s" % (i // 2, 1 + i % 2, b.tags[i].encode()) for i in range(b.n)]
    return b


# ------------------------------------------------------------------------------------------------------------- all of them
class Case:
    def __init__(self, family, label, kw, fasta, make):
        self.family, self.label, self.kw, self.fasta, self._make = family, label, kw, fasta, make

    @property
    def id(self):
        return self.family + "-" + self.label

    def batch(self):
        return _batch(self.id)


def _cases():
    out = []
    for m in RUN_MIN_LENGTHS:
        kw = dict(edit_distance=0, min_read_length=m)
        out.append(Case("runs", "mrl%g" % m, kw, b"", runs_batch))
    for kw in QUALITY_CONFIGS:
        kw = dict(kw, edit_distance=0)
        out.append(Case("quality", "q%d+%d" % (kw["fastq_start_char"], kw["min_quality"]), kw, FASTA, quality_batch))
    for label, kw in (("m24", dict(edit_distance=0)), ("m24-built1", dict(edit_distance=1)), ("m12", dict(edit_distance=0, match_length=12)),
                      ("m20", dict(edit_distance=0, match_length=20)), ("m28", dict(edit_distance=0, match_length=28))):
        out.append(Case("windows", label, kw, FASTA, windows_batch))
    out.append(Case("sides", "exact", dict(edit_distance=0, min_read_length=0.25), FASTA, sides_batch))
    out.append(Case("edits", "query1", dict(edit_distance=1, build_edits=0, min_read_length=0.2), FASTA, edits_batch))
    out.append(Case("edits", "query2", dict(edit_distance=2, build_edits=0, min_read_length=0.2), FASTA, edits_batch))
    out.append(Case("classes", "exact", dict(edit_distance=0, **CLASSES), FASTA, classes_batch))
    out.append(Case("pairs", "mrl0.4", dict(edit_distance=0, **CLASSES), FASTA, pairs_batch))
    out.append(Case("pairs", "mrl0.85", dict(edit_distance=0, min_read_length=0.85, **CLASSES), FASTA, pairs_batch))
    for ed in (0, 1, 2):
        out.append(Case("short", "query%d" % ed, dict(edit_distance=ed, build_edits=0, min_read_length=0.0), FASTA, short_batch))
    out.append(Case("characters", "exact", dict(edit_distance=0), FASTA, characters_batch))
    out.append(Case("characters", "built1", dict(edit_distance=1), FASTA, characters_batch))
    for what, arg in LAYOUTS:
        out.append(Case("layout", "%s%d" % (what, arg), dict(edit_distance=0), FASTA, functools.partial(layout_batch, what=what, arg=arg)))
    return out


CASES = {c.id: c for c in _cases()}
FAMILIES = ("runs", "quality", "windows", "sides", "edits", "classes", "pairs", "short", "characters", "layout")
# the family that has to notice each deliberate deviation of refartifact, and the case it is run on
SENSITIVE = {"no_odd_hop": "windows-m24", "book_at_window": "windows-m24", "pointer_at_min_pass": "windows-m24",
             "keep_left_gt": "sides-exact", "signed_sides": "sides-exact", "best_swap_ge": "runs-mrl0.4", "len_lt_1": "runs-mrl0",
             "f64_product": "runs-mrl0.4", "past_nonzero": "short-query0", "recanonicalise": "edits-query1", "first_hit": "edits-query1",
             "repeat_margin_le": "classes-exact", "unsigned_qual": "quality-q33+3", "min_qual_plus1": "quality-q33+3"}


@functools.lru_cache(maxsize=None)
def _batch(case_id):
    c = CASES[case_id]
    return c._make(c.kw)


def ids(family=None):
    return [i for i, c in CASES.items() if family is None or c.family == family]


# ------------------------------------------------------------------------------------------------- the reference's answers
def built_in(kw):
    return kw.get("edit_distance", 2) > 0 and kw.get("build_edits", 2) != 0


@functools.lru_cache(maxsize=None)
def reference_filter(case_id):
    """refartifact's filter for a case.  With nothing built in the set is refartifact's own; with substitutions built in it is
    the oracle's (held to the device by test_filter_set_matches_oracle: the map-order rule needs lookup3 and is not restated)"""
    c = CASES[case_id]
    if not built_in(c.kw):
        return ra.Filter(ra.Config(**c.kw), c.fasta)
    from helpers import OracleArtifactFilter, artifact_config
    o = OracleArtifactFilter(artifact_config(**c.kw), c.fasta)
    return ra.Filter(ra.Config(**c.kw), c.fasta, o.entries(), o.info()[2])


@functools.lru_cache(maxsize=None)
def reference(case_id, variant=None):
    """(results, (seqs, quals, names) afterwards) of refartifact; computed once, never changed"""
    b = CASES[case_id].batch()
    return reference_filter(case_id).apply(b.seqs, b.quals, b.mate, b.names, variant)
