"""Directed inputs for TnfDistance (tests/reftnf.py restates it, kmernator_amd/csrc/kmr_tnf.hpp computes it).  Sequences are
(bases, qualities) of bytes; a FASTA sequence carries quality 127 throughout."""
import numpy as np

REF = b"\x7f"


def random_bases(n, seed, gc=0.5):
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).choice(4, size=n, p=p)].tobytes()


def fasta(s):
    return bytes(s), REF * len(s)


def hq(s):
    return bytes(s), b"I" * len(s)


def vector_families(k):
    """[(name, bases, quals)]: the lengths around k, N at every kind of place, lower case, palindromes, homopolymers"""
    g = random_bases(400, 11)
    out = [("empty",) + fasta(b""), ("km1",) + fasta(g[:k - 1]), ("exact",) + fasta(g[5:5 + k]), ("kp1",) + fasta(g[9:9 + k + 1])]
    body = bytearray(g[20:20 + 6 * k + 7])
    for name, where in (("n_first", [0]), ("n_last", [len(body) - 1]), ("n_run", list(range(k + 1, 2 * k + 3)) + [3 * k + 1, 3 * k + 2])):
        s = bytearray(body)
        for i in where:
            s[i] = ord("N")
        out.append((name,) + fasta(s))
    for r in range(k):
        s = bytearray(body)
        for i in range(r, len(s), k):
            s[i] = ord("N")
        out.append(("n_mod_%d" % r,) + fasta(s))
    out.append(("lower",) + fasta(g[100:100 + 5 * k + 3].lower()))
    out.append(("mixed_case",) + fasta(g[100:130].lower() + g[130:170]))
    out.append(("palindromes",) + fasta(b"ACGT" * 20))
    out.append(("homopolymer_a",) + fasta(b"A" * 200))
    out.append(("homopolymer_t",) + fasta(b"T" * 71))
    out.append(("dinucleotide",) + fasta(b"AT" * 45))
    out.append(("hq_fastq",) + hq(g[200:330]))
    return out


def short_batch(n, seed=5):
    """n sequences of ragged lengths from 0 to 90 bases, FASTA and FASTQ mixed"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = random_bases(int(rng.integers(0, 91)), 1000 * seed + i, gc=float(rng.uniform(0.2, 0.8)))
        out.append(fasta(s) if i % 3 else hq(s))
    return out


def long_sequence(n=20000, seed=21):
    """one contig with an N here and there, longer than two extraction tiles"""
    s = bytearray(random_bases(n, seed, gc=0.6))
    for i in (0, 63, 64, 65, 4095, 4096, 9215, 9216, 9217, n - 1):
        s[i] = ord("N")
    return fasta(s)


def low_middle(n=300, seed=31):
    """a FASTQ sequence whose middle third has quality 2 (below min_quality_score 3: probability 0): its own vector loses the k-mers
    over it, a window's vector, which carries reference quality, does not"""
    s = random_bases(n, seed)
    return s, b"I" * (n // 3) + b"#" * (n // 3) + b"I" * (n - 2 * (n // 3))


def window_lengths(window, step):
    """sequences of window - 1, window, window + 1 and window + step + 1 bases, and one whose length the step does not divide"""
    return [fasta(random_bases(L, 40 + i)) for i, L in enumerate((window - 1, window, window + 1, window + step + 1, window + 3 * step + step // 2 + 1))]


def with_gaps(window, n_windows, seed=50):
    """a sequence that a step of `window` cuts into exactly n_windows windows, the first and the last of them mostly N"""
    s = bytearray(random_bases(window * n_windows + 1, seed))
    s[2:window - 2] = b"N" * (window - 4)
    last = window * (n_windows - 1)
    s[last + 2:last + window - 2] = b"N" * (window - 4)
    return fasta(s)


def three_inputs(window, step):
    """(reads, names, input_starts): input 0 two sequences of different composition, input 1 one sequence just long enough for exactly
    one window, input 2 a sequence too short for any and a longer one"""
    reads = [fasta(random_bases(window + 9 * step + 3, 61, gc=0.35)), fasta(random_bases(window + 4 * step + 1, 62, gc=0.65)),
             fasta(random_bases(window + 1, 63, gc=0.5)),
             fasta(random_bases(window - 2, 64)), fasta(random_bases(window + 7 * step + 2, 65, gc=0.75))]
    names = [b"in0_a", b"in0_b", b"in1_a", b"in2_short", b"in2_b"]
    return reads, names, np.array([0, 2, 3, 5], dtype=np.uint64)


def no_window_inputs(window, step):
    """three inputs of which the first yields no window and the second exactly one"""
    reads = [fasta(random_bases(window, 71)), fasta(random_bases(window + 1, 72)), fasta(random_bases(window + 5 * step + 1, 73, gc=0.3)), fasta(random_bases(window + 2 * step + 1, 74, gc=0.7))]
    return reads, np.array([0, 1, 2, 4], dtype=np.uint64)


def distance_set(n, k, seed=80):
    """n sequences for the distance matrices: 40 - 400 bases of varying GC, so that at k = 6 most columns are zero (heavy ties); the second
    is too short for a k-mer (a zero vector, length 1), the fourth repeats the third (distance +0)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i == 1:
            s = b"ACGTA"[:k - 1]
        elif i == 3:
            s = out[2][0]
        else:
            s = random_bases(int(rng.integers(40, 401)), seed * 1000 + i, gc=float(rng.uniform(0.25, 0.75)))
        out.append(fasta(s))
    return out


def fasta_text(reads, names):
    """FASTA text of the sequences, lines of 70 bases"""
    out = []
    for (s, _), name in zip(reads, names):
        out.append(b">" + name + b"\n")
        out += [s[i:i + 70] + b"\n" for i in range(0, len(s), 70)]
    return b"".join(out)
