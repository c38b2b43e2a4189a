"""Directed contigs and reads for KmerMatch (tests/refmatch.py restates it, kmernator_amd/csrc/kmr_match.hpp computes it): families,
each written for one rule of the match.  A case is a dict: contigs [bases], reads [(bases, quals)] laid out as consecutive pairs (read
2 i and 2 i + 1 are mates where the case is paired), discarded [flags], and the settings of the match (k, min_depth, edge,
max_read_matches, include_mate, seed, paired, first = global index of the first read)."""
import numpy as np

TILE_SPAN = 9856 - 32              # kmr_kernels.hpp: the bases of one extraction tile
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def R(n, seed):
    """n random bases"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def hq(s):
    return b"I" * len(s)


def case(name, k, contigs, reads, discarded=None, min_depth=1, edge=None, max_read_matches=450, include_mate=True, seed=0, paired=True, first=0):
    reads = [(bytes(s), hq(s) if q is None else bytes(q)) for s, q in reads]
    if paired and len(reads) % 2:
        reads.append((R(k + 4, 9999), hq(R(k + 4, 9999))))
    disc = [0] * len(reads) if discarded is None else list(discarded) + [0] * (len(reads) - len(discarded))
    return dict(name=name, k=k, contigs=[bytes(c) for c in contigs], reads=reads, discarded=disc, min_depth=min_depth, edge=k + 3 if edge is None else edge,
                max_read_matches=max_read_matches, include_mate=include_mate, seed=seed, paired=paired, first=first)


def _suffix(kw):
    return "".join("-%s%s" % (a, b) for a, b in sorted(kw.items()))


def with_settings(c, **kw):
    d = dict(c)
    d.update(kw)
    d["name"] = c["name"] + _suffix(kw)
    return d


def batches_of(c, cuts=()):
    """the case's reads as batches cut at `cuts` (even places where the case is paired, so that no pair is cut)"""
    edges = [0] + list(cuts) + [len(c["reads"])]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert not c["paired"] or lo % 2 == 0
        n = hi - lo
        mate = [i ^ 1 for i in range(n)] if c["paired"] else None
        out.append(dict(first=c["first"] + lo, reads=c["reads"][lo:hi], mate=mate, discarded=c["discarded"][lo:hi], lo=lo, hi=hi))
    return out


# ----------------------------------------------------------------------------------------------------------------------- contig shapes
def shapes(k, M=4):
    """contigs of n = 0, 1, M, M + 1, 2 M, 2 M + 1, 2 M + 2 k-mers (the last skips exactly one in the middle) under the edge setting
    k - 1 + M, and for every k-mer of every contig one read that holds that k-mer alone: the reads of k-mer j = M match (the left
    side's extra k-mer), those of j = n - M - 1 of the longest contig do not, nor does the read of the skipped middle"""
    contigs, reads = [], []
    for i, n in enumerate((0, 1, M, M + 1, 2 * M, 2 * M + 1, 2 * M + 2)):
        s = R(n + k - 1, 300 + i)
        contigs.append(s)
        reads += [(s[j:j + k], None) for j in range(n)]
    return case("shapes", k, contigs, reads, edge=k - 1 + M, paired=False)


def edge_settings(k):
    """one contig of 12 k-mers and a read per k-mer under the edge settings 0 and k - 2 (M < 0: every k-mer), k - 1 (M = 0: the first
    k-mer only) and 500 (all)"""
    s = R(k + 11, 320)
    base = case("edges", k, [s], [(s[j:j + k], None) for j in range(12)], paired=False)
    return [with_settings(base, edge=e) for e in (0, k - 2, k - 1, 500)]


def palindrome(k):
    half = R(k // 2, 17)
    return half + revcomp(half)


def mixed(k, dup=False, **kw):
    """M = 4, contigs of 12 k-mers and more (the middle is skipped): see the comment of every read"""
    c0 = R(k + 11, 100)
    c1 = R(3, 101) + c0[:k] + R(8, 102)                      # one key (c0's first k-mer) at the edges of two contigs
    X = R(k, 103)
    c2 = X + R(11, 104) + X                                  # one key at both ends of one contig
    c3 = bytearray(R(k + 11, 105)); c3[2] = ord("N")         # an N inside the left edge window
    contigs = [c0, c1, c2, bytes(c3), R(k - 1, 107)]         # ... and a contig shorter than k
    wseq = c1[8:8 + k]                                       # a k-mer of c1's right edge
    reads = [
        (c0[:k + 2], None),                                  # 0 matches c0, and c1 through the shared key: one read, two contigs
        (R(k + 5, 200), None),                               # 1 its mate, foreign: joins both sets
        (revcomp(c0[8:8 + k + 1]), None),                    # 2 matches c0 through the reverse complement
        (R(k + 5, 201), None),                               # 3 its mate, discarded: a discarded mate of a hit
        (c0[5:5 + k + 2], None),                             # 4 holds only the skipped middle of c0: no match
        (R(k + 5, 202), None),                               # 5
        (X + b"C" + X, None),                                # 6 the same k-mer twice in one read, at both ends of c2: once in c2's set
        (R(k + 5, 203), None),                               # 7
        (bytes(c3).replace(b"N", b"A")[:k + 2], None),       # 8 matches c3's windows over the N, which pack as A
        (bytes(c3)[:k + 2], None),                           # 9 the same with the N: its k-mers weigh 0, no match
        (c0[9:9 + k], None),                                 # 10 discarded: would hit c0
        (R(k + 5, 204), None),                               # 11 its mate: comes into no set
        (wseq, b"&" * k),                                    # 12 Q5 throughout: the occurrence fails the weight test ...
        (wseq, None),                                        # 13 ... while this read's passes: only 13 and 14 match c1
        (wseq, None),                                        # 14
        (R(k + 5, 205), None),                               # 15
    ]
    disc = [0] * len(reads)
    disc[3] = disc[10] = 1
    if k % 2 == 0:
        p = palindrome(k)
        contigs.append(p + R(11, 106))                       # a palindromic k-mer at the left edge
        reads += [(p + b"G", None), (R(k + 5, 206), None)]
        disc += [0, 0]
    if dup:                                                  # every read twice: every passing k-mer is seen twice at least
        reads, disc = reads + reads, disc + disc
    return case("mixed%s%s" % ("_dup" if dup else "", _suffix(kw)), k, contigs, reads, disc, **kw)


def many(k, n_hit, **kw):
    """n_hit reads that hold the first two k-mers of one contig, each followed by a foreign mate: sets that span tiles (> 64 reads) and
    wavefronts' worth of records (> 256), and the sampling's threshold"""
    c = R(k + 11, 400)
    reads = []
    for i in range(n_hit):
        reads += [(c[:k + 1], None), (R(k + 2, 5000 + i), None)]
    return case("many%d%s" % (n_hit, _suffix(kw)), k, [c, R(k + 11, 401)], reads, **kw)


def long_read(k):
    """a target read longer than an extraction tile, cut into work units: the contig's edges lie in its second and third unit"""
    c = R(k + 11, 500)
    s = R(TILE_SPAN + 300, 501) + c[:k + 1] + R(TILE_SPAN, 502) + revcomp(c[-(k + 1):]) + R(100, 503)
    return case("long_read", k, [c], [(s, None), (R(k + 5, 504), None), (c[4:4 + k], None), (R(k + 5, 505), None)])


def ref_quality(k):
    """reads without qualities (FASTA: every quality is Read::REF_QUAL): their k-mers weigh 1 and pass the weight test"""
    c = R(k + 11, 700)
    seqs = [c[:k + 3], revcomp(c[-(k + 2):]), R(k + 5, 701), c[5:5 + k + 2], c[:k + 3]]
    d = case("ref_quality", k, [c], [(s, b"\x7f" * len(s)) for s in seqs], paired=False, min_depth=2)
    d["fasta"] = True
    return d


# a global read index whose sampling draw in contig 0 under seed 0 is exactly the f32 bound of 6.0f / 7.0f (0.857142866..., above the
# quotient in double): u <= fraction holds in f32 and fails in double.  Found by a search over Philox once; test_match_cases checks it.
F32_EDGE_READ = 8601937104


def f32_edge():
    """seven reads on one contig under max_read_matches 3 (7 > 6: sampled), the fourth of them the read above"""
    k = 21
    c = R(k + 11, 600)
    reads = []
    for i in range(7):
        reads += [(c[:k], None), (R(k + 2, 6000 + i), None)]
    return case("f32_edge", k, [c], reads, max_read_matches=3, first=F32_EDGE_READ - 6, include_mate=False)


KS = (21, 22, 33, 65, 97)          # one, one (even), two, three and four key words


def all_cases():
    out = []
    for k in KS:
        out += [mixed(k), mixed(k, min_depth=2), mixed(k, dup=True, min_depth=2), mixed(k, dup=True, min_depth=3), mixed(k, include_mate=False), shapes(k)]
    out += edge_settings(21) + edge_settings(33)
    out += [many(21, 70, max_read_matches=35), many(21, 71, max_read_matches=35), many(21, 300, max_read_matches=100), many(21, 300, max_read_matches=100, seed=12345),
            many(21, 300, max_read_matches=0), many(33, 300, max_read_matches=100, include_mate=False), many(21, 300, max_read_matches=100, first=(1 << 32) + 12345)]
    out += [long_read(21), long_read(65), f32_edge(), ref_quality(21), ref_quality(65)]
    names = [c["name"] + "-k%d" % c["k"] for c in out]
    assert len(set(names)) == len(names), names
    return out


def cut_layouts(c):
    """two and three batches at different places (even where the case is paired)"""
    n = len(c["reads"])
    if n < 6:
        return []
    if c["paired"]:
        return [(2,), (n // 2 // 2 * 2, n - 2)] + ([(4, 6)] if n > 6 else [])
    return [(1,), (n // 2, n - 1), (3, 4)]
