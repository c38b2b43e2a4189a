"""Directed reads for CompareSpectrums (tests/refcompare.py restates it, kmernator_amd/csrc/kmr_compare.hpp computes it): set 2 and
the families of set 1, each written for one rule of the comparison.  Reads are (name, bases, qualities) of bytes."""
import numpy as np

from helpers import synth_reads

GENOME_LEN, SET2_READS, SET2_LEN, SET2_SEED = 2000, 200, 100, 7
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def random_bases(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def genome():
    """the genome synth_reads draws set 2 from (its generator's first draw)"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(SET2_SEED).integers(0, 4, size=GENOME_LEN, dtype=np.uint8)].tobytes()


def singleton_read():
    """a sequence foreign to the genome that set 2 holds once: its k-mers sit in set 2's singleton map only"""
    return random_bases(130, 991)


def set2():
    """about 200 reads of 100 bp from a 2 kb genome, noisy qualities and some N, and one read seen once: [(bases, quals)]"""
    rb = synth_reads(SET2_READS, read_len=SET2_LEN, genome_len=GENOME_LEN, seed=SET2_SEED, quality="noisy", n_rate=0.003)
    reads = [(rb.seq(i), rb.qual(i)) for i in range(rb.n)]
    s = singleton_read()
    reads.append((s, b"I" * len(s)))
    return reads


def _hq(s):
    return b"I" * len(s)


def palindrome(k):
    """a k-mer that is its own reverse complement (even k)"""
    assert k % 2 == 0
    half = random_bases(k // 2, 17)
    return half + revcomp(half)


def low_quality(k):
    """a genome read with two stretches of Q5 (P = 0.68 a base): the k-mers over eight of them weigh 0.68^8 = 0.047, which fails
    the weight test at min_weight 0.10 and passes at 0; the others pass both"""
    g = genome()
    s = g[300:300 + 3 * k + 30]
    q = bytearray(_hq(s))
    for a in (5, 2 * k + 9):
        q[a:a + 8] = b"&" * 8
    return s, bytes(q)


def families(k):
    """[(family, name, bases, quals)]"""
    g = genome()
    out = []

    def add(family, s, q=None):
        out.append((family, ("%s_%d" % (family, len(out))).encode(), bytes(s), _hq(s) if q is None else bytes(q)))

    add("short", g[10:10 + k - 1])
    add("exact", g[50:50 + k])
    add("kplus1", g[90:90 + k + 1])
    add("homopolymer", b"A" * (k + 40))
    add("tandem", (b"ACG" * (k + 20))[:2 * k + 31])
    if k % 2 == 0:
        p = palindrome(k)
        add("palindrome", g[400:420] + p + g[420:440] + p + g[440:450])
    fwd = g[700:700 + 2 * k + 17]
    add("strand", fwd)
    add("strand", revcomp(fwd))
    withn = bytearray(g[900:900 + 2 * k + 40])
    withn[k + 3] = ord("N"); withn[0] = ord("N")
    add("with_n", withn)
    s, q = low_quality(k)
    add("low_quality", s, q)
    add("fasta", g[1200:1200 + 2 * k + 25], b"\x7f" * (2 * k + 25))
    add("genome", g[1500:1500 + 3 * k])
    add("genome", revcomp(g[100:100 + 140]))
    add("foreign", random_bases(2 * k + 50, 5))
    add("singleton_only", singleton_read())
    add("empty", b"")
    return out


def circular(k):
    """circular references: longer than k, exactly k, shorter than k, empty"""
    g = genome()
    return [("circular", b"circ_%d" % i, s, _hq(s)) for i, s in enumerate((g[1000:1000 + 2 * k + 5], g[20:20 + k], g[33:33 + k // 2], b""))]


def batch_of(n, k, seed=3):
    """n reads for the batch-size cases: genome reads of ragged lengths around k, every fourth foreign"""
    g = genome()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(max(1, k - 3), k + 60))
        if i % 4 == 3:
            s = random_bases(L, 1000 + i)
        else:
            a = int(rng.integers(0, GENOME_LEN - L))
            s = g[a:a + L]
        out.append(("batch", b"b%d" % i, s, _hq(s)))
    return out


def cap_mix(k, cap, tile_span):
    """reads of cap - 1, cap and cap + 1 k-mers and one of several tile spans, between short ones: the boundary between the LDS kernel
    and the sorted path, and a read that is cut into work units"""
    g = genome()
    out = []
    for j, nk in enumerate((cap - 1, cap, cap + 1)):
        L = nk + k - 1
        s = (g * (L // GENOME_LEN + 2))[37 * j:37 * j + L]
        out.append(("cap", b"cap%d" % nk, s, _hq(s)))
        out.append(("cap", b"gap%d" % j, g[60 * j:60 * j + k + 7], _hq(g[60 * j:60 * j + k + 7])))
    L = 2 * tile_span + 1234
    long_read = (g * (L // GENOME_LEN + 2))[11:11 + L // 2] + random_bases(L - L // 2, 77)
    out.append(("cap", b"long", long_read, _hq(long_read)))
    out.append(("cap", b"tail", g[5:5 + k + 2], _hq(g[5:5 + k + 2])))
    return out
