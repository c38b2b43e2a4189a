"""Reads and per-position counts for the scoreAndTrimReads tests (plain Python, no GPU).  kmr_score_counts_dev takes any u32 count
per base position, so every count pattern the scoring kernel can meet is written down here directly instead of being engineered
out of k-mers: each read declares the class it is meant to hit (CLASSES), tests/test_score_cases.py checks with the reference's
semantics alone (tests/refsemantics.score_and_trim) that it does, and tests/test_gpu_score_trim.py holds the kernel to the same
function on exactly these arrays.

The kernel (score_reads_kernel, kmr_kernels.hpp) gives 64 consecutive reads to a wavefront and copies their counts into LDS as
u16 when the group's count range is at most SC_CAP entries, else it walks them in global memory; the count range is the group's
base span where counts are indexed by base position ("base" layout: kmr_score_counts_dev, streaming lookups) and its number of
k-mers where they are an exclusive scan ("scan" layout: table probes).  The batch builders put groups on either side of that."""
import numpy as np

from refsemantics import score_and_trim

SC_CAP, GROUP, SC_WAVES = 10240, 64, 3          # kmr_kernels.hpp
PAD = 64                                        # bytes behind the last read, as every device read batch has
MIN_SCORES = (0, 2, 2.5, 70000)
SCORINGS = ("SUM", "MEDIAN", "MIN", "MAX", "AVG")
GEOMETRY = (1, 63, 64, 65, 193)
MAX_COUNT = 65535                               # what a lookup answers at most (the count saturates there)

CLASSES = ("tie", "run_start", "run_end", "none_pass", "all_pass", "zeros_pass", "fraction",
           "median_even", "median_odd", "median_one", "median_equal", "median_extremes",
           "markup_at_k", "markup_at_k1", "markup_several", "markup_x", "markup_dot", "markup_noncut",
           "short", "empty", "empty_before_n", "n_first", "long")


class Read:
    """one read: its bases, a count for each of its max(0, L - k + 1) k-mer positions (also behind a markup, where a real lookup
    leaves zeros: the kernel must not look there), the class it is meant to hit and the minimum scores at which it is in it"""

    def __init__(self, cls, seq, kcounts, at=(2, 2.5)):
        self.cls, self.seq, self.at = cls, bytes(seq), tuple(at)
        self.kcounts = np.asarray(kcounts, dtype=np.uint32)

    def __repr__(self):
        return "Read(%s, L=%d)" % (self.cls, len(self.seq))


def _bases(L, salt):
    """L bases of ACGT (no markup); what they are does not matter to the scoring"""
    return bytes(b"ACGT"[(i * 7 + salt + (i >> 2)) & 3] for i in range(L))


def _read(cls, k, kcounts, marks=(), at=(2, 2.5), salt=0):
    kcounts = list(kcounts)
    s = bytearray(_bases(len(kcounts) + k - 1, salt))
    for pos, ch in marks:
        s[pos] = ord(ch)
    return Read(cls, s, kcounts, at)


def long_read(k):
    """more k-mers than SC_CAP: alone it takes its group out of LDS in both layouts.  Passing runs of 300 with counts up to 65535
    between single failing positions -- every run ties with the first -- and an N that cuts the last 700 k-mers off."""
    n = SC_CAP + 900
    kc = [3 + ((i * 2654435761) >> 7) % 65533 for i in range(n)]
    kc[5], kc[6] = MAX_COUNT, 3
    for i in range(300, n, 301):
        kc[i] = i % 2
    return _read("long", k, kc, marks=[(n - 700 + k - 1, "N")], salt=3)


def cases(k):
    """the reads of every class but "long", in an order that matters only where reads are empty: an empty read shares its
    offset with the read behind it"""
    H = [11, 7, 30, 5, 19, 3, 23, 13, 4, 17, 29, 9]          # all >= 3: pass at 2 and at 2.5
    hi = lambda n, s=0: [H[(i + s) % len(H)] for i in range(n)]
    r = [
        _read("tie", k, [9, 8, 7, 0, 5, 6, 4, 1, 3, 3, 3]),
        _read("tie", k, [0, 5, 5, 1, 6, 7, 0], salt=1),
        _read("run_start", k, [7, 8, 9, 10, 0, 5, 1, 6, 6], salt=2),
        _read("run_end", k, [5, 0, 6, 1, 7, 8, 9, 10], salt=3),
        _read("none_pass", k, [0, 1, 1, 0, 1]),
        _read("none_pass", k, hi(9), at=(70000,), salt=1),
        _read("all_pass", k, hi(7), salt=2),
        _read("all_pass", k, [0, 1, 0, 2, 65535, 1], at=(0,)),
        _read("zeros_pass", k, [0, 0, 5, 0], at=(0,), salt=1),
        _read("fraction", k, [2, 2, 2, 0, 3, 3], at=(2,), salt=2),
        _read("median_even", k, [0, 10, 30, 20, 40, 0]),
        _read("median_even", k, [1, 7, 9, 0], salt=1),
        _read("median_odd", k, [1, 50, 10, 40, 20, 30, 1], salt=2),
        _read("median_one", k, [0, 0, 17, 0, 1], salt=3),
        _read("median_one", k, [4]),
        _read("median_equal", k, [0, 12, 12, 12, 12, 1], salt=1),
        _read("median_extremes", k, [65535, 0, 65535, 0, 0], at=(0,), salt=2),
        _read("median_extremes", k, [0, 65535, 1, 65535], at=(0,), salt=3),
        _read("markup_at_k", k, hi(7), marks=[(k - 1, "N")], at=MIN_SCORES[:3]),
        _read("markup_at_k1", k, hi(7, 2), marks=[(k, "N")], at=MIN_SCORES[:3], salt=1),
        _read("markup_several", k, hi(12, 1), marks=[(k + 5, "X"), (k + 2, "N"), (k + 9, ".")], salt=2),
        _read("markup_x", k, hi(9, 3), marks=[(k + 3, "X")], salt=3),
        _read("markup_dot", k, hi(9, 4), marks=[(k + 1, ".")]),
        _read("markup_noncut", k, hi(9, 5), marks=[(2, "Y"), (k + 1, "n"), (k + 3, "R")], salt=1),
        Read("short", _bases(k - 1, 2), []),
        Read("short", b"N" if k > 1 else b"", []),
        Read("empty", b"", []),
        _read("all_pass", k, hi(5, 6), salt=3),          # the read an empty one shares its offset with
        Read("empty_before_n", b"", []),
        Read("empty_before_n", b"", []),
        _read("n_first", k, hi(6, 7), marks=[(0, "N")], at=MIN_SCORES[:3]),
        Read("empty", b"", []),
    ]
    return r


def passing_runs(values, min_score):
    """[(offset, length)] of the maximal runs of values >= min_score, by a plain scan of its own"""
    runs, start = [], None
    for i, v in enumerate(list(values) + [None]):
        ok = v is not None and float(v) >= min_score
        if ok and start is None:
            start = i
        elif not ok and start is not None:
            runs.append((start, i - start))
            start = None
    return runs


def _cut(read, k):
    """number of k-mers in front of the first N / X / . (all of them if there is none)"""
    n = len(read.kcounts)
    marks = [i for i, c in enumerate(read.seq) if c in b"NX."]
    if marks:
        m = marks[0] + 1
        n = max(0, min(n, m - k))
    return n


def in_class(reads, i, k, min_score, scoring="MEDIAN"):
    """does the reference put reads[i] in its declared class at this minimum score?  Returns a string saying why not, or None."""
    rd = reads[i]
    L, kc = len(rd.seq), rd.kcounts
    ref = score_and_trim(kc, rd.seq, k, min_score, scoring)
    toff, tlen, sc, trimmed = ref
    n = _cut(rd, k)
    runs = passing_runs(kc[:n], min_score)
    longest = max([ln for _, ln in runs], default=0)
    first = next(((o, ln) for o, ln in runs if ln == longest), (0, 0))
    if longest:
        if (toff, tlen, trimmed) != (first[0], longest + k - 1, longest < n):
            return "the reference's run %r is not the first longest %r" % (ref, first)
    elif (toff, tlen, sc, trimmed) != (0, 0, -1.0, n > 0):
        return "nothing passes, yet the reference says %r" % (ref,)
    run = sorted(int(v) for v in kc[first[0]:first[0] + longest])
    med = score_and_trim(kc, rd.seq, k, min_score, "MEDIAN")[2]
    unmarked = bytes(c if c in b"ACGT" else ord("A") for c in rd.seq)
    c = rd.cls
    ok = True
    if c == "tie":
        ties = [o for o, ln in runs if ln == longest]
        ok = len(ties) >= 2 and toff == ties[0] != ties[-1]
    elif c == "run_start":
        ok = longest > 0 and toff == 0 and trimmed and len(runs) >= 2
    elif c == "run_end":
        ok = longest > 0 and toff > 0 and toff + longest == n == len(kc) and len(runs) >= 2
    elif c == "none_pass":
        ok = n > 0 and not runs and ref == (0, 0, -1.0, True)
    elif c == "all_pass":
        ok = n == len(kc) > 0 and (toff, tlen, trimmed) == (0, L, False)
    elif c == "zeros_pass":
        ok = min_score <= 0 and 0 in kc[:n] and (toff, tlen, trimmed) == (0, L, False)
    elif c == "fraction":
        ok = min_score == int(min_score) and score_and_trim(kc, rd.seq, k, min_score + 0.5, scoring)[:2] != (toff, tlen)
    elif c == "median_even":
        ok = longest >= 2 and longest % 2 == 0 and med == run[longest // 2] != run[longest // 2 - 1]
    elif c == "median_odd":
        ok = longest >= 3 and longest % 2 == 1 and run[longest // 2 - 1] != run[longest // 2] != run[longest // 2 + 1] and med == run[longest // 2]
    elif c == "median_one":
        ok = longest == 1 and med == run[0]
    elif c == "median_equal":
        ok = longest >= 2 and run[0] == run[-1] == med
    elif c == "median_extremes":
        ok = longest >= 3 and run[0] == 0 and run[-1] == MAX_COUNT and med == run[longest // 2]
    elif c == "markup_at_k":
        ok = rd.seq[k - 1:k] == b"N" and len(kc) > 1 and all(float(v) >= min_score for v in kc) and ref == (0, 0, -1.0, False)
    elif c == "markup_at_k1":
        ok = rd.seq[k:k + 1] == b"N" and len(kc) > 2 and all(float(v) >= min_score for v in kc) and (toff, tlen, trimmed) == (0, k, False)
    elif c == "markup_several":
        marks = [j for j, ch in enumerate(rd.seq) if ch in b"NX."]
        ok = len(marks) >= 3 and n == marks[0] + 1 - k > 0 and tlen == n + k - 1
    elif c in ("markup_x", "markup_dot"):
        ch = b"X" if c == "markup_x" else b"."
        ok = rd.seq.count(ch) == 1 and ref == score_and_trim(kc, rd.seq.replace(ch, b"N"), k, min_score, scoring) \
            and ref != score_and_trim(kc, unmarked, k, min_score, scoring)
    elif c == "markup_noncut":
        other = [j for j, ch in enumerate(rd.seq) if ch not in b"ACGT"]
        as_n = bytes(ord("N") if j in other[1:] else ch for j, ch in enumerate(rd.seq))
        ok = len(other) >= 3 and b"n" in rd.seq and b"R" in rd.seq and n == len(kc) and ref == score_and_trim(kc, unmarked, k, min_score, scoring) \
            and ref != score_and_trim(kc, as_n, k, min_score, scoring)
    elif c == "short":
        ok = 0 < L < k and ref == (0, 0, -1.0, False)
    elif c == "empty":
        ok = L == 0 and ref == (0, 0, -1.0, False)
    elif c == "empty_before_n":
        nxt = next((x for x in reads[i + 1:] if len(x.seq)), None)
        ok = L == 0 and ref == (0, 0, -1.0, False) and nxt is not None and nxt.cls == "n_first"
    elif c == "n_first":
        ok = rd.seq[:1] == b"N" and len(kc) > 0 and all(float(v) >= min_score for v in kc) and ref == (0, 0, -1.0, False) and i > 0 and reads[i - 1].cls == "empty_before_n"
    elif c == "long":
        ties = [o for o, ln in runs if ln == longest]
        ok = len(kc) > SC_CAP and n < len(kc) and len(ties) >= 2 and toff == ties[0] and max(kc[:n]) == MAX_COUNT
    else:
        return "unknown class %s" % c
    return None if ok else "%r is not in class %s at minimum score %s: reference %r, runs %r" % (rd, c, min_score, ref, runs[:6])


# ---- batches ----------------------------------------------------------------------------------------------------------------
class Batch:
    """what the device is given: bases (PAD bytes behind the last read, `first` bytes in front of the first), offsets[n + 1] and
    one count per base position of bases[:offsets[n]]"""

    def __init__(self, reads, k, first=0):
        self.k, self.n, self.reads = k, len(reads), reads
        lens = np.array([len(r.seq) for r in reads], dtype=np.uint64)
        self.offsets = np.full(self.n + 1, first, dtype=np.uint64)
        np.cumsum(lens, out=self.offsets[1:])
        self.offsets[1:] += np.uint64(first)
        total = int(self.offsets[-1])
        # N, X and . where no read is: right in front of the first read and in the padding, inside the first 16-byte load behind the
        # last base and beyond it.  They show that the scan gives such bytes to no read; they cannot tell whether the kernel's
        # `pp >= b0 && pp < b1` is there: without it a byte in front wraps to a position >= 0xfffffff0 of the first read and one
        # behind lands on position L of the last read, and neither shortens numKmers
        gap = (b"N.XAN" * (first // 5 + 1))[-first:] if first else b""
        pad = bytearray(PAD)
        for j in (0, 1, 2, 15, 16, PAD - 1):
            pad[j] = ord("N")
        pad[3], pad[17] = ord("X"), ord(".")
        self.bases = np.frombuffer(gap + b"".join(r.seq for r in reads) + bytes(pad), dtype=np.uint8).copy()
        assert self.bases.size == total + PAD
        # positions that are no k-mer's (the last k - 1 of a read, the gap) hold counts that pass every minimum score but 70000:
        # a kernel that reads one too many sees a longer run
        self.counts = (60000 + np.arange(total, dtype=np.uint32) % 5).astype(np.uint32)
        for i, r in enumerate(reads):
            o = int(self.offsets[i])
            self.counts[o:o + len(r.kcounts)] = r.kcounts
        assert self.counts.max(initial=0) <= MAX_COUNT

    def seq(self, i):
        return self.bases[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()

    def kcounts(self, i):
        o, L = int(self.offsets[i]), int(self.offsets[i + 1] - self.offsets[i])
        return self.counts[o:o + max(0, L - self.k + 1)]

    def reference(self, min_score, scoring):
        """(trim_offset u32, trim_length u32, score f32, was_trimmed bool) of every read, from what the arrays hold"""
        res = [score_and_trim(self.kcounts(i), self.seq(i), self.k, min_score, scoring) for i in range(self.n)]
        return (np.array([x[0] for x in res], np.uint32), np.array([x[1] for x in res], np.uint32),
                np.array([x[2] for x in res], np.float32), np.array([x[3] for x in res], bool))

    def average(self, min_score):
        """np.float32(sum / n) of the reference's run, the sum taken in f64 over the integer counts (exact), -1 without a run"""
        out = np.full(self.n, -1.0, np.float32)
        for i in range(self.n):
            toff, tlen, _, _ = score_and_trim(self.kcounts(i), self.seq(i), self.k, min_score, "MIN")
            if tlen:
                run = self.kcounts(i)[toff:toff + tlen - self.k + 1].astype(np.float64)
                out[i] = np.float32(run.sum() / run.size)
        return out

    def spans(self, layout="base"):
        """count range of every group of 64 reads: bases ("base") or k-mers ("scan"); staged in LDS where <= SC_CAP"""
        o = self.offsets.astype(np.int64)
        if layout == "scan":
            o = np.concatenate([[0], np.cumsum(np.maximum(np.diff(o) - self.k + 1, 0))])
        return [int(o[min(g + GROUP, self.n)] - o[g]) for g in range(0, self.n, GROUP)]


def staged_batch(k, first=0):
    """every case, no long read: every group in LDS"""
    return Batch(cases(k), k, first)


def unstaged_batch(k, first=0):
    """every case with the long read inside each group of 64: no group in LDS"""
    reads = cases(k)
    out = []
    for r in reads:
        if len(out) % GROUP == 7:
            out.append(long_read(k))
        out.append(r)
    return Batch(out, k, first)


def geometry_batch(k, n_reads):
    """the cases over and over up to n_reads reads.  A group's last read ends in N, right in front of the next group's range, and the third group's first read
    begins with one, right behind the second group's range (a hit must go to the group that holds it; as in Batch, the kernel's
    range comparison itself cannot be told from these); with 65 reads the tail
    group is the long read alone, with 193 the long read takes the second group out of LDS between groups that stay in it"""
    cs = cases(k)
    reads = [cs[i % len(cs)] for i in range(n_reads)]
    reads = [Read(r.cls, r.seq, r.kcounts, r.at) for r in reads]
    if n_reads == 65:
        reads[64] = long_read(k)
    if n_reads == 193:
        reads[70] = long_read(k)
    for g in range(GROUP, n_reads, GROUP):
        reads[g - 1] = _read("boundary", k, [5, 6, 0, 7, 8, 9], marks=[(k + 4, "N")], at=())          # its last base
        if g == 2 * GROUP:
            reads[g] = _read("boundary", k, [9, 8, 7, 0, 5, 6, 4], marks=[(0, "N")], at=(), salt=1)
    return Batch(reads, k)


def _mixed_counts(rng, n):
    """counts with runs, ties and the values around the minimum scores"""
    v = rng.choice(np.array([0, 1, 2, 3, 5, 9, 300, MAX_COUNT], np.uint32), size=n, p=[.12, .12, .06, .2, .2, .15, .1, .05])
    return v.astype(np.uint32)


def threshold_batch(k, layout, over):
    """a first group of 64 reads whose count range is exactly SC_CAP (over = 0) or SC_CAP + 1 (over = 1) in `layout`, and a second
    group of five reads; the twins differ in one base and one count of read 10"""
    assert over in (0, 1) and 160 >= k
    rng = np.random.default_rng(1000 * k + (7 if layout == "scan" else 0))
    per = SC_CAP // GROUP + (k - 1 if layout == "scan" else 0)
    reads = []
    for i in range(GROUP + 5):
        L = per + (1 if (i == 10 and over) else 0)
        kc = _mixed_counts(rng, per - k + 1)
        extra = rng.choice(np.array([3, 1], np.uint32), size=1)          # drawn for both twins: the rest of the batch stays the same
        if L > per:
            kc = np.concatenate([kc, extra])
        s = bytearray(_bases(L, i))
        if i % 9 == 4:
            s[int(rng.integers(0, per))] = ord("N")
        reads.append(Read("threshold", s, kc, ()))
    return Batch(reads, k)


# ---- reads for the end-to-end comparison with the oracle -------------------------------------------------------------------
E2E_KS = (21, 32, 33, 64, 65, 127)
E2E_SEEDS = {21: 121, 32: 132, 33: 133, 64: 164, 65: 165, 127: 227}          # chosen so that test_score_cases' counts hold
E2E_SHORT, E2E_LONG, E2E_LONG_AT = 600, 70, 2 * GROUP


def end_to_end_reads(k, seed=None, others=True):
    """600 ragged noisy reads (helpers.noisy_ragged_reads: some shorter than k, some empty, N at rate 0.003) and, from the same
    genome, 70 reads of 200 to 400 bases in a row from read 128 on -- the third group of 64 is out of LDS in both layouts -- with
    an X, a '.', an n and an R in four reads each (others=False: X and '.' in eight reads each and no markup that does not cut, which
    is what the streaming lookups are kept for)"""
    from helpers import ReadBatch, noisy_ragged_reads, synth_reads
    seed = E2E_SEEDS[k] if seed is None else seed
    rb = noisy_ragged_reads(k, E2E_SHORT, seed)
    rl = max(100, k + 40)
    lg = synth_reads(E2E_LONG, read_len=400, genome_len=max(rl * 2, E2E_SHORT * rl // 30), seed=seed, quality="noisy", n_rate=0.003)
    rng = np.random.default_rng(seed + 1)
    seqs = [bytearray(rb.seq(i)) for i in range(rb.n)]
    quals = [rb.qual(i) for i in range(rb.n)]
    for j in range(E2E_LONG):
        L = int(rng.integers(200, 401))
        seqs.insert(E2E_LONG_AT + j, bytearray(lg.seq(j)[:L]))
        quals.insert(E2E_LONG_AT + j, lg.qual(j)[:L])
    for i in (5, GROUP, 2 * GROUP - 1, E2E_LONG_AT + E2E_LONG + 1):          # empty reads: inside a group, its first, its last
        seqs[i], quals[i] = bytearray(), b""
    roomy = [i for i, s in enumerate(seqs) if len(s) >= k + 12]
    for n_, i in enumerate(rng.choice(roomy, size=16, replace=False)):
        seqs[i][int(rng.integers(k, len(seqs[i])))] = (b"X.nR" if others else b"X.X.")[n_ % 4]
    return ReadBatch([bytes(s) for s in seqs], quals)


def read_spans(offsets, k, layout):
    """Batch.spans for plain offsets"""
    o = np.asarray(offsets).astype(np.int64)
    n = o.size - 1
    if layout == "scan":
        o = np.concatenate([[0], np.cumsum(np.maximum(np.diff(o) - k + 1, 0))])
    return [int(o[min(g + GROUP, n)] - o[g]) for g in range(0, n, GROUP)]


def oracle_counts(cfg, rb, min_depth=2):
    """per read, the oracle's lookups of the oracle's own k-mers in an oracle spectrum built from rb: nothing of the device's"""
    from helpers import OracleSpectrum, oracle_weighted_kmers
    o = OracleSpectrum(cfg)
    o.add_reads(rb)
    o.finalize(min_depth)
    out = []
    for i in range(rb.n):
        keys, _, _ = oracle_weighted_kmers(cfg, rb.seq(i), rb.qual(i))
        out.append(o.lookup(keys) if len(keys) else np.zeros(0, np.uint32))
    o.close()
    return out


def reference_of_counts(counts, rb, k, min_score, scoring):
    """score_and_trim over a read batch and its per-read counts, as the four arrays scoreAndTrimReads returns"""
    res = [score_and_trim(counts[i], rb.seq(i), k, min_score, scoring) for i in range(rb.n)]
    return (np.array([x[0] for x in res], np.uint32), np.array([x[1] for x in res], np.uint32),
            np.array([x[2] for x in res], np.float32), np.array([x[3] for x in res], bool))


def threshold_reads(k, layout, over, seed=77):
    """real reads of threshold_batch's lengths for the end-to-end form of the threshold: reads 0..68 drawn from a 3000-base
    genome, then a copy of each with one base changed in its second half (and an N in every seventh), so that counts of 1 and
    trims appear; the first group of 64 is the one on the threshold"""
    from helpers import ReadBatch
    lens = np.diff(threshold_batch(k, layout, over).offsets.astype(np.int64))
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=3000)]
    starts = rng.integers(0, genome.size - int(lens.max()) - 1, size=lens.size)          # the twins start where each other do
    seqs = [bytearray(genome[s:s + L].tobytes()) for s, L in zip(starts, lens)]
    copies = []
    for i, s in enumerate(seqs):
        c = bytearray(s)
        p = len(c) // 2 + int(rng.integers(0, len(c) // 2 - 1))
        c[p] = ord("N") if i % 7 == 3 else b"ACGT"[(b"ACGT".index(c[p]) + 1) & 3]
        copies.append(c)
    seqs = [bytes(s) for s in seqs + copies]
    return ReadBatch(seqs, [b"I" * len(s) for s in seqs])
