"""Directed batches for coverage normalization (tests/refnormalize.py is what they are judged by).  Every maker returns a Batch that
says in .purpose what it is for and in .witness the reads that make it so; the CPU tests check each family against a restatement
with one rule changed, the GPU tests run the same batches on the device."""
import numpy as np

from refnormalize import Normalizer, draw, pair_list

LABEL = b"MedianScore"
T = 9                     # target depth of the directed batches
SUM_SCORE = 5.0e6         # a SUM score above 2^32 / 1000
SCORES = [3, T, T + 1, 65535, SUM_SCORE, 0.7, -1, 40, T + 0.6, 250]


def labels_of(n, action, lo, hi, to, tl, sc, wt):
    """FilterKnownOddities' AFTrim and setTrimHeaders' labels (src/ReadSelector.h:1015-1036); a discarded read has none"""
    out = []
    for i in range(n):
        if action[i] == 2:
            out.append(b"")
            continue
        parts = []
        if action[i] == 1:
            parts.append(b"AFTrim:%d+%d" % (lo[i], hi[i] - lo[i]))
        if wt[i]:
            parts.append(b"Trim:%d+%d" % (to[i], tl[i]))
        s = float(sc[i]) + 0.5
        parts.append(LABEL + b":%d" % int(max(-2147483648.0, min(2147483647.0, s))))
        out.append(b" ".join(parts))
    return out


class Batch:
    """reads with the results of the earlier stages made up, a pair list, and the parameters of one normalization"""

    def __init__(self, purpose, n, seed=1, read1=None, read2=None, input_starts=None, target=T, min_score=0.5, min_read_length=0.40, by_pair=True,
                 both_pass=False, draw_seed=7, first=0, max_len=100):
        rng = np.random.default_rng(seed)
        self.purpose, self.witness, self.n = purpose, {}, n
        L = [1 + (i * 37 + 11) % max_len for i in range(n)]
        self.raw_names = [b"r%d/%d" % (i * 3, 1 + i % 2) + (b" c" if i % 4 == 0 else b"") for i in range(n)]
        self.names = [nm.split(b" ")[0] for nm in self.raw_names]
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        self.seqs = [bytes(acgt[rng.integers(0, 4, l)]) for l in L]
        self.quals = [bytes(rng.integers(35, 74, l, dtype=np.uint8)) for l in L]
        self.action = np.zeros(n, dtype=np.uint8)
        self.tl = np.array(L, dtype=np.uint32)
        self.to = np.zeros(n, dtype=np.uint32)
        self.sc = np.array([SCORES[(i * 7 + i // 10) % len(SCORES)] for i in range(n)], dtype=np.float32)
        self.read1 = None if read1 is None else np.asarray(read1, dtype=np.int64)
        self.read2 = None if read2 is None else np.asarray(read2, dtype=np.int64)
        self.input_starts = input_starts
        self.cfg = dict(target_depth=target, min_score=min_score, min_read_length=min_read_length, by_pair=by_pair, both_pass=both_pass, seed=draw_seed, first_read_idx=first)

    def trim(self, i, to, tl):
        self.to[i], self.tl[i] = to, tl

    @property
    def lo(self):
        return np.where(self.action == 1, 2, 0).astype(np.uint32)

    @property
    def hi(self):
        return np.array([len(s) for s in self.seqs], dtype=np.uint32) + self.lo

    @property
    def wt(self):
        return np.array([self.tl[i] < len(self.seqs[i]) for i in range(self.n)], dtype=np.uint8)

    @property
    def disc(self):
        return [bool(a == 2) for a in self.action]

    def fastq(self):
        return b"".join(b"@" + self.raw_names[i] + b"\n" + self.seqs[i] + b"\n+\n" + self.quals[i] + b"\n" for i in range(self.n))

    def pairs(self):
        return pair_list(self.n, self.read1, self.read2)

    def expect(self, cls=Normalizer, out_base=33, fasta=False, **override):
        cfg = dict(self.cfg, **override)
        labels = labels_of(self.n, self.action, self.lo, self.hi, self.to, self.tl, self.sc, self.wt)
        return cls(**cfg).run(self.names, self.seqs, self.quals, labels, self.disc, self.to, self.tl, self.sc, self.pairs(), self.input_starts, out_base - 33, out_base, fasta)

    def half(self, lo, hi):
        """the reads [lo, hi) as a batch of their own with first_read_idx moved along; the cut must not part a pair"""
        b = Batch.__new__(Batch)
        b.purpose, b.witness, b.n = self.purpose, {}, hi - lo
        for k in ("raw_names", "names", "seqs", "quals"):
            setattr(b, k, getattr(self, k)[lo:hi])
        for k in ("action", "tl", "to", "sc"):
            setattr(b, k, getattr(self, k)[lo:hi].copy())
        b.read1 = b.read2 = None
        if self.read1 is not None:
            keep = [p for p in range(self.read1.size) if lo <= max(self.read1[p], self.read2[p]) < hi]
            for p in keep:
                assert all(x < 0 or lo <= x < hi for x in (self.read1[p], self.read2[p])), "the cut parts a pair"
            b.read1 = np.array([self.read1[p] - lo if self.read1[p] >= 0 else -1 for p in keep], dtype=np.int64)
            b.read2 = np.array([self.read2[p] - lo if self.read2[p] >= 0 else -1 for p in keep], dtype=np.int64)
        b.input_starts = None
        b.cfg = dict(self.cfg, first_read_idx=self.cfg["first_read_idx"] + lo)
        return b


def interleaved(n, **kw):
    """pairs (0, 1), (2, 3), ...; an odd last read is listed by no pair.  Scores below T, T, T + 1, 65 535, a SUM score above
    2^32 / 1000, 0.7 over a minimum of 0.5, -1; every 11th read discarded, every 13th fails the length, every 7th has an AFTrim label"""
    m = n // 2
    b = Batch("interleaved pairs over every score class", n, read1=np.arange(m) * 2, read2=np.arange(m) * 2 + 1, **kw)
    b.action[5::7] = 1
    b.action[3::11] = 2
    for i in range(6, n, 13):
        b.trim(i, 1, 1)
    for i in range(2, n, 5):
        b.trim(i, i % 3, max(2, int(b.tl[i]) - 4))
    return b


def blocks(m, extra=5, **kw):
    """An R1 block [0, m) and an R2 block [m, 2m) from two inputs, then `extra` reads no pair names in a third: mates lie in
    different units and different files.  Every third pair is listed as (R2 read, R1 read): read1 > read2.  Pairs 1 mod 10 lose
    their R2 side and pairs 4 mod 10 their R1 side (half pairs of either side; the dropped reads are then unlisted).  A discarded
    and a failed mate stand beside passing ones."""
    n = 2 * m + extra
    r1, r2 = [], []
    for i in range(m):
        a, c = i, m + i
        if i % 3 == 2:
            a, c = c, a
        if i % 10 == 1:
            c = -1
        elif i % 10 == 4:
            a = -1
        r1.append(a)
        r2.append(c)
    b = Batch("R1 block then R2 block: pick order, read1 > read2, half pairs of either side, unlisted reads, discarded and failed mates", n, seed=2,
              read1=r1, read2=r2, input_starts=[0, m, 2 * m, n], **kw)
    b.sc[:] = [[40, 250, 65535, T + 1, 3, 100][(i * 5 + i // 6) % 6] for i in range(n)]
    w = b.witness
    w["reversed"] = [i for i in range(m) if r1[i] > r2[i] >= 0]
    w["half1"] = [i for i in range(m) if r2[i] < 0]
    w["half2"] = [i for i in range(m) if r1[i] < 0]
    for i in range(m):
        if i % 10 == 6:
            b.action[m + i] = 2          # a discarded mate
        if i % 10 == 8:
            b.sc[i] = 0.1                # a failed mate
    w["discarded_mate"] = [i for i in range(m) if i % 10 == 6]
    w["failed_mate"] = [i for i in range(m) if i % 10 == 8]
    return b


def both_pass_halves(m=40, **kw):
    """both_pass with half pairs present: their one read passes with a score at or below T, so only the s <= 0 test of :698
    keeps them out"""
    n = 2 * m
    r1 = [2 * i for i in range(m)]
    r2 = [2 * i + 1 if i % 4 else -1 for i in range(m)]
    b = Batch("both_pass drops every half pair", n, seed=3, read1=r1, read2=r2, both_pass=True, **kw)
    b.sc[:] = [[3, T, 40, 5][i % 4] for i in range(n)]
    b.witness["halves"] = [2 * i for i in range(m) if i % 4 == 0]
    return b


def single_reads_over(n, s=100, target=T, **kw):
    """n single reads of score s > T with no pair list: every read draws.  The witness holds the reads whose draw % s is exactly
    T (kept by the inclusive compare) and exactly T + 1 (the first residue that is not)"""
    b = Batch("draw boundaries: draw %% %d == T and == T + 1" % s, n, seed=4, target=target, by_pair=False, **kw)
    b.sc[:] = s
    res = [draw(b.cfg["seed"], b.cfg["first_read_idx"] + i) % s for i in range(n)]
    long_enough = [len(b.seqs[i]) > 1 for i in range(n)]      # a read of one base fails passesLength and never draws
    b.witness["drawing"] = sum(long_enough)
    b.witness["at_T"] = [i for i in range(n) if res[i] == target and long_enough[i]]
    b.witness["at_T_plus_1"] = [i for i in range(n) if res[i] == target + 1 and long_enough[i]]
    assert b.witness["at_T"] and b.witness["at_T_plus_1"], "no read sits on the boundary: take more reads"
    return b


def truncation(n=60, **kw):
    """scores between whole numbers: 0.7 (passes a minimum of 0.5, truncates to 0: never chosen), T + 0.6 (truncates to T:
    kept for certain; rounded it would draw among T + 1), 1.5"""
    b = Batch("(long) truncates the score", n, seed=5, by_pair=False, **kw)
    b.sc[:] = [[0.7, T + 0.6, 1.5, 0.99][i % 4] for i in range(n)]
    b.witness["zero"] = [i for i in range(n) if i % 4 in (0, 3)]
    return b


def reversed_pairs(m=200, **kw):
    """full pairs listed with read1 > read2, all far above T: g of read1 instead of the lower index decides other pairs"""
    b = Batch("g is that of the pair's lower read index", 2 * m, seed=6, read1=[2 * i + 1 for i in range(m)], read2=[2 * i for i in range(m)], **kw)
    b.sc[:] = 30
    return b


def by_read_full_pairs(m=150, **kw):
    """by_pair off over full pairs, some with read1 > read2: a pick may hold read2 alone and is then ordered by it"""
    r1 = [2 * i + (i % 2) for i in range(m)]
    r2 = [2 * i + 1 - (i % 2) for i in range(m)]
    b = Batch("by_pair 0 over full pairs", 2 * m, seed=8, read1=r1, read2=r2, by_pair=False, **kw)
    b.sc[:] = [[30, 12, 3, 0.7][(i // 2 + i) % 4] for i in range(2 * m)]
    return b
