"""Directed batches for the artifact filter's report (kmr_artifact_filter_report; tests/refartifact_report.py restates it): every
rule of the Recorder as a family of a handful of reads, a filter with more sequences than the counters' LDS cap, and a pseudo-random
batch in an R1 and an R2 block.  tests/test_artifact_report_cases.py proves on the CPU that each family holds what it is meant to
hold and notices the deviation written for it; tests/test_gpu_artifact_report.py runs them on the device.

The reads and the small FASTA table are those of tests/artifactcases.py (three adapters, two simple repeats, a stand-in PhiX and a
reference-class sequence).  Every filter has edit distance 0, so refartifact computes its set itself."""
import functools

import numpy as np

import artifactcases as ac
import refartifact as ra
import refartifact_report as rr

KW = dict(edit_distance=0, **ac.CLASSES)
L = 100


def low_every(n, step):
    return ac.quals(n, low_at=tuple(range(step - 1, n, step)))


def make_read(kind, k):
    """(bases, qualities) of one read that meets the rule named `kind`"""
    if kind in ac.KINDS:
        return ac.kind_read(kind, k)           # clean; quality: kept; adapter: trimmed to 72; repeat; phix; reference (38 kept of 100, discarded)
    if kind == "adapter_short":                # a hit in the middle of a short read: 20 of 60 bases are left, below 0.40
        return ac.planted(60, k, ac.AD_C[3:27], 20), ac.quals(60)
    if kind == "quality_discard":              # no run of 40 good bases
        return ac.bg(L, k), low_every(L, 20)
    if kind == "reference_long":               # 72 bases would be kept, but a reference hit discards
        return ac.planted(L, k, ac.REFERENCE[5:29], 72), ac.quals(L)
    if kind == "one_bad":
        return ac.bg(1, k), ac.LOW
    if kind == "empty":
        return b"", b""
    if kind.startswith("all_low"):             # all_low<n>: n bases, none good
        n = int(kind[7:])
        return ac.bg(n, k), ac.LOW * n
    raise KeyError(kind)


# what each kind comes to on its own under KW: (action, value) with value "q" = n_sequences
ALONE = {"clean": (0, 0), "quality": (1, "q"), "adapter": (1, ac.IDX[b"adapter_c"]), "phix": (2, ac.IDX[b"phix"]), "reference": (2, ac.IDX[b"reference"]),
         "adapter_short": (2, ac.IDX[b"adapter_c"]), "quality_discard": (2, "q"), "reference_long": (2, ac.IDX[b"reference"]), "one_bad": (2, "q"), "empty": (0, 0)}


# the table without its all-A sequence, for the reads of no or one base: the zeros past a read's bytes look like A's to the windows
FASTA_NO_POLY_A = b"".join(b">" + n + b" made for the tests\n" + (ac.lcg_bases(24, 29) if n == b"poly_a" else s) + b"\n" for n, s in ac.TABLE)


class Case:
    """names None: the batch goes in through ReadSet.from_arrays and every name is empty; else through FASTQ text"""

    def __init__(self, cid, kinds, pairs=None, input_starts=None, names="plain", kw=KW, fasta=ac.FASTA, in_base=33, out_base=33, reads=None):
        self.id, self.kinds, self.pairs, self.kw, self.fasta, self.in_base, self.out_base = cid, kinds, pairs, dict(kw, fastq_start_char=in_base), fasta, in_base, out_base
        self.input_starts = None if input_starts is None else [int(x) for x in input_starts]
        rd = reads if reads is not None else [make_read(kind, 3 * i + 1) for i, kind in enumerate(kinds)]
        self.seqs = [s for s, _ in rd]
        self.quals = [bytes((c - 33 + in_base) & 0xff for c in q) for _, q in rd]
        if names is None:
            self.names = None
        elif names == "plain":
            self.names = [b"read%d/%d" % (i, 1 + i % 2) for i in range(len(rd))]
        else:
            self.names = list(names)
        assert self.names is None or len(self.names) == len(rd)

    @property
    def n(self):
        return len(self.seqs)

    def shown_names(self):
        return self.names if self.names is not None else [b""] * self.n

    def fastq(self):
        return b"".join(b"@" + nm + b"\n" + s + b"\n+\n" + q + b"\n" for nm, s, q in zip(self.names, self.seqs, self.quals))

    def arrays(self):
        off = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        return np.frombuffer(b"".join(self.seqs), dtype=np.uint8).copy(), np.frombuffer(b"".join(self.quals), dtype=np.uint8).copy(), off

    def mate(self):
        if self.pairs is None:
            return None
        m = np.full(self.n, -1, dtype=np.int64)
        for a, b in self.pairs:
            if a >= 0 and b >= 0:
                m[a], m[b] = b, a
        return m

    def pair_arrays(self):
        if self.pairs is None:
            return None
        p = np.array(self.pairs, dtype=np.int64).reshape(-1, 2)
        return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])

    def prefixes(self):
        return ["in%d" % j for j in range(1 if self.input_starts is None else len(self.input_starts) - 1)]


def name_of_length(i, n):
    head = b"r%d_" % i
    return head + b"x" * (n - len(head))


def _label_case():
    """a filter whose sequences are named with 1 and with 100 characters, hit by one discarded read each"""
    s1, s2 = ac.lcg_bases(40, 31), ac.lcg_bases(40, 37)
    fasta = b">x one character\n" + s1 + b"\n>" + b"L" * 100 + b"\thundred\n" + s2 + b"\n"
    reads = [(ac.planted(60, 1, s1[2:26], 20), ac.quals(60)), (ac.planted(60, 2, s2[4:28], 20), ac.quals(60)), (ac.bg(60, 3), ac.quals(60))]
    return Case("labels-1-100", ["hit_x", "hit_L", "clean"], kw=dict(edit_distance=0), fasta=fasta, reads=reads)


MANY_SEQ = 300      # 24 x 301 = 7224 bytes of counters: above the 6 KiB a unit sums in LDS by default


def _many_sequences_case():
    """300 sequences of match_length bases; reads that hit the first, one in the middle, the last two and a read with a quality trim"""
    seqs = [ac.lcg_bases(24, 1000 + i) for i in range(MANY_SEQ)]
    fasta = b"".join(b">s%d\n" % (i + 1) + s + b"\n" for i, s in enumerate(seqs))
    reads, kinds = [], []
    for k, i in enumerate((0, 0, 149, 298, 299, 299, 299)):
        at = 20 if k % 2 else 72       # discarded (20 of 60 left) or trimmed (72 of 100 left)
        n = 60 if k % 2 else L
        reads.append((ac.planted(n, k, seqs[i], at), ac.quals(n)))
        kinds.append("s%d" % (i + 1))
    reads += [make_read("quality_discard", 50), make_read("quality", 51), make_read("clean", 52)]
    kinds += ["quality_discard", "quality", "clean"]
    return Case("many-sequences", kinds, kw=dict(edit_distance=0), fasta=fasta, reads=reads)


RANDOM_HALF = 1100
RANDOM_KINDS = ("clean",) * 12 + ("quality", "adapter", "phix", "reference", "adapter_short", "quality_discard", "reference_long", "quality")


def _random_case():
    """2200 reads in an R1 and an R2 block (two inputs): pair p is (p, 1100 + p), every 7th the other way round, every 11th split into two half pairs"""
    x, kinds = 12345, []
    for _ in range(2 * RANDOM_HALF):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        kinds.append(RANDOM_KINDS[(x >> 33) % len(RANDOM_KINDS)])
    pairs = []
    for p in range(RANDOM_HALF):
        a, b = p, RANDOM_HALF + p
        if p % 11 == 5:
            pairs += [(a, -1), (-1, b)]
        else:
            pairs.append((b, a) if p % 7 == 3 else (a, b))
    return Case("random-r1r2", kinds, pairs=pairs, input_starts=[0, RANDOM_HALF, 2 * RANDOM_HALF])


def _cases():
    out = []
    out.append(Case("singles", ["clean", "adapter", "adapter_short", "quality", "quality_discard", "phix", "reference_long", "clean", "phix", "adapter_short"]))
    out.append(Case("short-only", ["one_bad", "empty", "one_bad", "clean"], names=None, fasta=FASTA_NO_POLY_A))
    out.append(Case("singles-nameless", ["clean", "one_bad", "empty", "quality_discard", "phix", "empty", "one_bad"], names=None, fasta=FASTA_NO_POLY_A))
    # pairs: every read is named once; (read1, read2)
    kinds = ["phix", "clean",                    # 0 1   PhiX on one side only
             "quality_discard", "clean",         # 2 3   (filler for the half pairs below)
             "adapter_short", "quality_discard", # 4 5   both discarded, read1 = 5 the higher index
             "quality_discard", "clean",         # 6 7   one discarded, the other clean
             "adapter", "adapter_short",         # 8 9   one trimmed, the other discarded
             "reference_long", "adapter",        # 10 11 a reference hit, the other affected (its trim becomes a discard)
             "reference_long", "clean",          # 12 13 a reference hit, the other clean
             "clean", "phix",                    # 14 15 PhiX on read2 only
             "quality", "quality"]               # 16 17 both trimmed: counted, not written
    pairs = [(0, 1), (2, -1), (-1, 3), (5, 4), (6, 7), (8, 9), (10, 11), (12, 13), (14, 15), (16, 17)]
    out.append(Case("pairs", kinds, pairs=pairs))
    out.append(Case("pairs-half", ["quality_discard", "adapter_short", "phix", "clean", "phix"], pairs=[(-1, 0), (1, -1), (-1, 2), (3, -1), (4, -1)], input_starts=[0, 2, 5]))
    # a pair across two inputs: read1 in the second input, read2 in the first
    out.append(Case("pairs-two-inputs", ["adapter_short", "clean", "quality_discard", "phix", "quality_discard", "clean"], pairs=[(4, 0), (1, 3), (2, 5)], input_starts=[0, 3, 6]))
    out.append(Case("pairs-nameless", ["phix", "empty", "one_bad", "phix", "one_bad", "empty"], pairs=[(0, 1), (2, 3), (4, 5)], names=None, fasta=FASTA_NO_POLY_A))
    out.append(Case("three-inputs", ["quality_discard", "phix", "clean", "clean", "quality", "adapter_short", "phix"], input_starts=[0, 2, 5, 7]))
    # names: comments behind a blank and behind a tab; records of 63 .. 129 bytes = name + bases + 23 with the label MinQualityTrim3 and the base line N
    names = [b"blank some comment", b"tab\tcomment"] + [name_of_length(i, n) for i, n in ((2, 10), (3, 11), (4, 12), (5, 14), (6, 15), (7, 16))]
    out.append(Case("names", ["quality_discard", "phix", "all_low30", "all_low30", "all_low30", "all_low90", "all_low90", "all_low90"], names=names))
    out.append(_label_case())
    out.append(Case("shift-64-to-33", ["quality_discard", "phix", "adapter", "clean"], in_base=64, out_base=33))
    out.append(Case("shift-33-to-64", ["quality_discard", "phix", "adapter", "clean"], in_base=33, out_base=64))
    out.append(_many_sequences_case())
    out.append(_random_case())
    return out


CASES = {c.id: c for c in _cases()}
RECORD_SIZES = (63, 64, 65, 127, 128, 129)

# the case that has to notice each deliberate deviation of refartifact_report, and cases it must leave alone
SENSITIVE = {"bases_printed": "singles", "quals_masked": "singles", "phix_affected_only": "pairs", "phix_labelled": "singles", "file_of_own_read": "pairs-two-inputs",
             "read_index_order": "pairs", "trim_counts_len": "singles", "mate_labelled": "pairs"}
UNTOUCHED = {"bases_printed": ("short-only",), "quals_masked": ("short-only",), "phix_affected_only": ("singles", "three-inputs"),
             "phix_labelled": ("many-sequences", "labels-1-100"), "file_of_own_read": ("singles", "three-inputs", "pairs"), "read_index_order": ("singles", "three-inputs", "pairs-half"),
             "trim_counts_len": ("names", "pairs-half"), "mate_labelled": ("singles", "pairs-half", "three-inputs")}


def ids():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def reference_filter(case_id):
    c = CASES[case_id]
    return ra.Filter(ra.Config(**dict(c.kw, build_edits=0)), c.fasta)


@functools.lru_cache(maxsize=None)
def decisions(case_id):
    """(results, reads afterwards) of refartifact for the case; computed once, never changed"""
    c = CASES[case_id]
    return reference_filter(case_id).apply(c.seqs, c.quals, c.mate(), c.shown_names())


@functools.lru_cache(maxsize=None)
def expected(case_id, print_bases=False, artifact_output=True, phix_output=True, variant=None):
    c = CASES[case_id]
    return rr.report(reference_filter(case_id), decisions(case_id)[0], c.shown_names(), c.seqs, c.quals, c.pairs, c.input_starts, artifact_output, phix_output,
                     c.in_base, c.out_base, print_bases, variant)
