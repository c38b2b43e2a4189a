"""Directed runs for the bimodal cut (ReadSelector --bimodal-sigmas; plain Python, no GPU).  As in tests/scorecases.py the counts of
every k-mer position are written down directly and reach the device through kmr_score_counts_dev; each read is the smallest
shape at which one thing can go wrong, and names the family it belongs to.  tests/test_bimodal_cases.py checks with the
restatement alone (tests/refbimodal.py) that the families do what they are for; tests/test_gpu_bimodal.py holds
bimodal_trim_kernel to the restatement on exactly these arrays.

The kernel deals a read to a wavefront: lane l takes the splits p = l + 1, l + 65, ..., so runs of 63 / 64 / 65 / 128 / 129 k-mers
sit on either side of a chunk of 64 splits; a run of at most BM_CAP k-mers is staged in LDS, a longer one is walked in global
memory; reads 4g .. 4g + 3 share a block of four wavefronts."""
import math

import numpy as np

import refbimodal as rb
from scorecases import Batch, _read

BM_CAP, BM_WAVES = 4096, 4                       # kmr_kernels.hpp
MIN_SCORE = 2
SIGMAS = (0.0, 0.5, 2.0, 2.5, 3.0)
LENGTHS = (2, 3, 4, 63, 64, 65, 128, 129)
FAMILIES = ("length", "single_side", "plateau", "point_nine", "variance", "floor", "offset", "markup", "max_count", "window", "noisy")
# the family written for each deviant of refbimodal.DEVIANTS ("edge": edge_batch -- in f64 the closed form of the variance differs from the
# pass over the deviations in its last bits only, which decide nothing but a comparison on the edge)
WRITTEN_FOR = {"float_abs": "point_nine", "last_tie": "plateau", "no_floor": "floor", "rooted": "variance", "closed_form": "edge"}


def two_level(n, p, hi, lo, head=True):
    """n counts: p of one level, then n - p of the other; head: the higher level first"""
    a, b = (hi, lo) if head else (lo, hi)
    return [a] * p + [b] * (n - p)


def _jitter(vals, salt, amp):
    """the values moved by a fixed pattern of -amp .. +amp, never below MIN_SCORE"""
    return [max(MIN_SCORE, min(65535, v + ((i * 2654435761 + salt * 40503) >> 5) % (2 * amp + 1) - amp)) for i, v in enumerate(vals)]


def cases(k):
    r = []
    add = lambda fam, kc, **kw: r.append(_read(fam, k, kc, **kw))
    # run lengths: 2 is not searched; 3 and 4 are; the others sit around one and two chunks of 64 splits, cut at either end and in the middle
    add("length", [40, 4])
    add("length", [40, 40, 4])
    add("length", [4, 40, 40], salt=1)
    add("length", [40, 4, 4, 4], salt=2)
    for n in LENGTHS[3:]:
        for j, p in enumerate((1, n // 2, 63, 64, n - 1)):
            if 0 < p < n:
                add("length", _jitter(two_level(n, p, 40, 4, head=(j + n) % 2 == 0), n + j, 1), salt=j)
    # a side of one value: its mean is the value undivided, its variance 0, its "stdDev" the floor alone; the reduced run has length 1
    add("single_side", [60] + [5, 6] * 6)
    add("single_side", [5, 6] * 6 + [60], salt=1)
    add("single_side", [3, 30, 31, 29, 30], salt=2)
    add("single_side", [30, 31, 29, 30, 3], salt=3)
    # plateaus: neighbouring splits whose truncated diffs are equal -- the first of them wins
    for j, x in enumerate((12, 11, 13, 9, 16)):
        add("plateau", [20] * 5 + [x] + [4] * 5, salt=j)
        add("plateau", [4] * 5 + [x] + [20] * 5, salt=j + 1)
    add("plateau", [30, 30, 30, 30, 18, 17, 16, 6, 6, 6, 6], salt=2)
    add("plateau", [6, 6, 6, 6, 16, 17, 18, 30, 30, 30, 30], salt=3)
    # mean gaps of x.9 where sigmas * floor lies between x and x.9: nine times hi and once hi - 1 against a flat low side
    for hi, lo, reps in ((11, 2, 10), (8, 2, 10), (15, 3, 10), (9, 2, 10), (4, 2, 10), (12, 2, 10), (15, 2, 10), (7, 2, 10), (21, 5, 10)):
        side = [hi] * (reps - 1) + [hi - 1]
        add("point_nine", side + [lo] * reps, at=(0,))
        add("point_nine", [lo] * reps + side[::-1], at=(0,), salt=1)
    # sides whose variance is far above the floor (it decides), against flat sides where the floor decides
    add("variance", [70, 10, 75, 5, 80, 12, 66, 9] + [4] * 8)
    add("variance", [4] * 8 + [70, 10, 75, 5, 80, 12, 66, 9], salt=1)
    add("variance", [40, 30, 50, 20, 45, 35] + [3, 4, 3, 5, 3, 4], salt=2)
    add("variance", [30, 34, 27, 33, 29, 36, 25, 31] + [12, 9, 14, 8, 11, 13, 7, 10], salt=3)
    add("variance", [12, 9, 14, 8, 11, 13, 7, 10] + [30, 34, 27, 33, 29, 36, 25, 31])
    add("variance", [100, 140, 90, 130, 80, 150, 95, 125] + [60, 75, 50, 70, 55, 65, 58, 72], salt=1)
    add("floor", [16] * 8 + [4] * 8)
    add("floor", [4] * 8 + [16] * 8, salt=1)
    add("floor", [25] * 6 + [9] * 6, salt=2)
    add("floor", [9] * 6 + [25] * 6, salt=3)
    add("floor", [36, 36, 37, 36, 36, 35] + [20] * 6)
    add("floor", [14] * 7 + [7] * 7, salt=1)
    add("floor", [7] * 7 + [15] * 7, salt=2)
    # the run does not start at k-mer 0; an N cuts the k-mers behind it off (the low level beyond the cut is never seen)
    add("offset", [0, 1, 0] + two_level(12, 5, 30, 3) + [1], salt=2)
    add("offset", [5, 6, 1] + two_level(12, 7, 30, 3, head=False), salt=3)
    add("markup", two_level(14, 6, 30, 3) + [3] * 4, marks=[(k + 13, "N")])
    add("markup", two_level(14, 6, 30, 3, head=False) + [30] * 4, marks=[(k + 8, "X")], salt=1)
    # the largest count: means, prefix sums and tags at 16 bits
    add("max_count", [65535] * 5 + [3] * 5)
    add("max_count", [3] * 5 + [65535] * 5, salt=1)
    add("max_count", [65535, 65534, 65535, 65533, 65535, 65530] + [65500, 65498, 65501, 65499, 65502, 65497], salt=2)
    add("max_count", [60000, 60007, 60001, 60006, 60002, 60005, 60003] + [60012, 60018, 60013, 60017, 60014, 60016, 60015], salt=3)
    add("max_count", [50000 + (i * 37) % 11 for i in range(20)] + [50009 + (i * 29) % 13 for i in range(20)])
    return r


def noisy_runs(seed, n_runs, lo_len=3, hi_len=140):
    """two-level runs with Poisson noise on both levels, at depths where every one of the sigmas decides some of them"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_runs):
        n = int(rng.integers(lo_len, hi_len + 1))
        p = int(rng.integers(1, n))
        a, b = float(rng.choice([4, 6, 9, 14, 20, 30, 45])), float(rng.choice([4, 6, 9, 14, 20, 30, 45]))
        v = np.concatenate([rng.poisson(a, p), rng.poisson(b, n - p)])
        out.append([int(x) for x in np.clip(v, MIN_SCORE, 65535)])
    return out


def window_reads(k):
    """the longest run that is staged in LDS and the first that is not, each cut far from its ends"""
    a = _jitter(two_level(BM_CAP, 1500, 40, 6), 5, 2)
    b = _jitter(two_level(BM_CAP + 1, 2700, 40, 6, head=False), 9, 2)
    return [_read("window", k, a), _read("window", k, b, salt=1)]


def directed_batch(k):
    """every directed read and 49 noisy ones; read 63 and read 64 are cut runs (the last of a group of 64 and the first of the next), the
    number of reads is no multiple of 64 nor of a block's four"""
    reads = cases(k) + [_read("noisy", k, kc, salt=i) for i, kc in enumerate(noisy_runs(17, 49))] + window_reads(k)
    reads[63], reads[1] = reads[1], reads[63]
    reads[64], reads[2] = reads[2], reads[64]
    assert len(reads) % 64 and len(reads) % BM_WAVES and len(reads) > 128
    return Batch(reads, k)


def reference(batch, min_score, scoring, sigmas, deviant=None):
    return rb.reference_of_counts([batch.kcounts(i) for i in range(batch.n)], [batch.seq(i) for i in range(batch.n)], batch.k, min_score, scoring, sigmas, deviant)


# ---- the edge family ----------------------------------------------------------------------------------------------------------------
def flip_point(vals):
    """For the split that wins at sigmas = 0 -- the first of the largest diff --: the adjacent doubles s_lo < s_hi with
    diff > s_lo * stdDev and not diff > s_hi * stdDev, found by bisection over the doubles; and whether the floor decides.  None if
    the run has no split."""
    found = rb.find_partition_plain(vals, 0.0)
    if found is None:
        return None
    p = found[0]
    diff, sd, _, floored = rb.threshold(vals, p)
    lo, hi = 0.0, 2.0 * diff / sd + 1.0
    assert diff > lo * sd and not diff > hi * sd
    while math.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2
        if diff > mid * sd:
            lo = mid
        else:
            hi = mid
    return p, lo, hi, floored


def edge_runs(per_kind=16):
    """per_kind runs whose flip point is decided by a variance and per_kind where it is decided by a floor: [(values, s_lo, s_hi,
    floored)].  At s_lo the winning split of sigmas = 0 still qualifies, at s_hi it does not."""
    out, have = [], {True: 0, False: 0}
    for seed in range(400):
        rng = np.random.default_rng(1000 + seed)
        n, flat = int(rng.integers(6, 40)), bool(seed % 2)
        p = int(rng.integers(2, n - 1))
        a, b = (float(x) for x in rng.choice([5, 8, 13, 21, 34, 55], size=2, replace=False))
        if flat:      # little noise: the floors are above the variances
            v = np.concatenate([a + rng.integers(0, 2, p), b + rng.integers(0, 2, n - p)])
        else:
            v = np.concatenate([rng.poisson(a, p) + rng.integers(0, 9, p), rng.poisson(b, n - p) + rng.integers(0, 9, n - p)])
        vals = [int(x) for x in np.clip(v, MIN_SCORE, 65535)]
        fp = flip_point([float(x) for x in vals])
        if fp is None or have[fp[3]] >= per_kind:
            continue
        have[fp[3]] += 1
        out.append((vals, fp[1], fp[2], fp[3]))
        if have[True] >= per_kind and have[False] >= per_kind:
            break
    assert have[True] == per_kind and have[False] == per_kind, have
    return out


def edge_batch(k):
    runs = edge_runs()
    return Batch([_read("edge", k, vals, salt=i) for i, (vals, _, _, _) in enumerate(runs)], k), runs


# ---- reads that cross between a deep and a shallow region of a genome ------------------------------------------------------------------
def boundary_reads(k, n_reads=400, read_len=100, seed=5, copies=10, unique=200, repeat=150):
    """A genome of `copies` units, each `unique` bases of its own followed by the same `repeat` bases: evenly drawn reads see the
    repeat `copies` times as deep as the rest, and a read that crosses a repeat's end switches between the two depths inside one
    run of passing k-mers, in either direction.  Every 37th read holds an N.  Returns a helpers.ReadBatch."""
    from helpers import ReadBatch
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rep = acgt[rng.integers(0, 4, size=repeat)]
    genome = np.concatenate([np.concatenate([acgt[rng.integers(0, 4, size=unique)], rep]) for _ in range(copies)])
    seqs = []
    for i in range(n_reads):
        st = int(rng.integers(0, genome.size - read_len))
        s = bytearray(genome[st:st + read_len].tobytes())
        if i % 37 == 5:
            s[int(rng.integers(k, read_len))] = ord("N")
        seqs.append(bytes(s))
    return ReadBatch(seqs, [b"I" * len(s) for s in seqs])
