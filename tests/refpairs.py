"""A plain sequential restatement of ReadSet::identifyPairs (src/ReadSet.cpp:446-570, with _isSequentialPair :94-118) and of the
name helpers it uses (src/Utils.h: trimName :561-598, commonName :669-676, isCommentCasava18 :678-685, readNum :689-713, isPair
:719-733), for one call on a fresh ReadSet: strings, a dict and a list of pairs, as the reference has them.  The oracle of the
pair-identification tests, with the cases worked by hand and the seeded generator both the CPU and the GPU tests use."""
import numpy as np

NONE = -1          # MAX_READ_IDX


def is_comment_casava18(comment):
    if len(comment) < 6:
        return False
    return comment[1] == ":" and comment[3] == ":" and comment[5] == ":" and comment[0] in "12" and comment[2] in "YN"


def trim_name(line, store_comment):
    """(name, comment as Read keeps it, passes the Casava filter) of a name line without its marker"""
    good = True
    comment = ""
    pos = -1
    for i, ch in enumerate(line):
        if ch in " \t\r\n":
            pos = i
            break
    if pos < 0:
        return line, "", True
    chars = list(line)
    if len(line) >= pos + 2:
        comment = line[pos + 1:]
        if is_comment_casava18(comment) and (pos <= 2 or chars[pos - 2] != "/"):
            if not store_comment:
                chars[pos] = "/"
                pos += 2
            if pos + 3 < len(chars) and chars[pos + 3] == "Y":
                good = False
    name = "".join(chars[:pos])
    return name, (comment if store_comment else ""), good          # a Read keeps its comment only if comments are stored


def common_name(name):
    if len(name) <= 2:
        return name
    if name[-2] == "/":
        return name[:-1]
    return name


def read_num(name, comment):
    if is_comment_casava18(comment):
        return 2 if comment[0] == "2" else 1
    if len(name) < 2 or name[-2] != "/":
        return 0
    if name[-1] in "1AF":
        return 1
    if name[-1] in "2BR":
        return 2
    return 0


def is_pair(name_a, comment_a, name_b, comment_b):
    if common_name(name_a) != common_name(name_b):
        return False
    a, b = read_num(name_a, comment_a), read_num(name_b, comment_b)
    return a != 0 and b != 0 and a != b


class Result:
    """mate[i]; pairs = list of (read1, read2); the counts; and how often each branch was taken (the generator's test asks)"""

    def __init__(self, n):
        self.n_reads = n
        self.mate = [NONE] * n
        self.pairs = []
        self.n_sequential = 0
        self.n_full = 0
        self.conflict_read1 = 0
        self.conflict_read2 = 0
        self.name_matched = 0
        self.zero_matches = 0          # a readNum == 0 read that met an entry
        self.chain_reads = 0           # reads at distance >= 2 from the start of a run of consecutive links

    @property
    def n_pairs(self):
        return len(self.pairs)

    @property
    def n_conflicts(self):
        return self.conflict_read1 + self.conflict_read2

    def has_pairs(self):
        return 0 < len(self.pairs) < self.n_reads

    def mate_array(self):
        return np.array(self.mate, dtype=np.int64).reshape(-1)

    def pair_array(self):
        return np.array(self.pairs, dtype=np.int64).reshape(-1, 2)


def identify_pairs(name_lines, store_comment):
    """name_lines: each read's name line without '@' and without the line end, in batch order"""
    reads = [trim_name(l, store_comment)[:2] for l in name_lines]
    n = len(reads)
    res = Result(n)
    paired = [False] * n
    # :467-478 over _isSequentialPair (:94-118)
    prev_name, prev_comment = "", ""
    for i, (name, comment) in enumerate(reads):
        seq = False
        if read_num(name, comment) == 0:
            prev_name, prev_comment = "", ""
        elif prev_name != "" and is_pair(prev_name, prev_comment, name, comment):
            prev_name, prev_comment = "", ""
            seq = True
        else:
            prev_name, prev_comment = name, comment
        if seq:
            paired[i] = paired[i - 1] = True
            res.mate[i], res.mate[i - 1] = i - 1, i
            res.pairs.append((i - 1, i))
            res.n_sequential += 1
    # (for the generator's test only: reads that would pair with their predecessor, which would pair with its own)
    link = [i > 0 and is_pair(reads[i - 1][0], reads[i - 1][1], reads[i][0], reads[i][1]) for i in range(n)]
    res.chain_reads = sum(1 for i in range(1, n) if link[i] and link[i - 1])
    res.n_full = res.n_sequential
    # :500-565
    unmatched = {}
    for i, (name, comment) in enumerate(reads):
        if paired[i]:
            continue
        num = read_num(name, comment)
        common = common_name(name)
        if common in unmatched:
            at = unmatched[common]
            r1, r2 = res.pairs[at]
            if num == 2:
                if r2 != NONE:
                    res.conflict_read2 += 1
                    del unmatched[common]
                    res.pairs.append((NONE, i))
                    continue
                r2 = i
            else:
                if r1 != NONE:
                    res.conflict_read1 += 1
                    del unmatched[common]
                    res.pairs.append((i, NONE))
                    continue
                r1 = i
            res.pairs[at] = (r1, r2)
            del unmatched[common]
            paired[r1] = paired[r2] = True
            res.mate[r1], res.mate[r2] = r2, r1
            res.n_full += 1
            res.name_matched += 1
            if num == 0:
                res.zero_matches += 1
        else:
            if num > 0:
                unmatched[common] = len(res.pairs)
            res.pairs.append((NONE, i) if num == 2 else (i, NONE))
    return res


def casava_rewrites(name_lines, store_comment):
    """how many names trimName rewrites"""
    return sum(1 for l in name_lines if trim_name(l, store_comment)[0] != trim_name(l, True)[0])


# ---- cases worked by hand from the reference's code: (label, name lines, store_comment, mate, pairs) ----------------------
X = NONE
HAND_CASES = [
    ("interleaved /1 /2", ["a/1", "a/2", "b/1", "b/2"], 1, [1, 0, 3, 2], [(0, 1), (2, 3)]),
    ("R1 block then R2 block", ["a/1", "b/1", "c/1", "a/2", "b/2", "c/2"], 1, [3, 4, 5, 0, 1, 2], [(0, 3), (1, 4), (2, 5)]),
    ("/A /B and /F /R", ["a/A", "a/B", "b/F", "b/R", "c/R", "c/F"], 1, [1, 0, 3, 2, 5, 4], [(0, 1), (2, 3), (4, 5)]),
    # the single clears the pending read; it has readNum 0, so it pushes (2, -) and never enters the map
    ("a single without suffix between pairs", ["a/1", "a/2", "solo", "b/1", "b/2"], 1, [1, 0, X, 4, 3], [(0, 1), (3, 4), (2, X)]),
    # "/1" and "/2" have length 2: commonName keeps them whole, so they differ; "x" and "1" have readNum 0
    ("names of length <= 2", ["/1", "/2", "x", "1", "/1"], 1, [X, X, X, X, X],
     # phase 2: "/1" pushes (0,-) and enters; "/2" pushes (-,1) and enters; "x", "1" push; the second "/1" meets the entry of read 0
     # whose read1 is taken: conflict, entry erased, pushes (4,-)
     [(0, X), (X, 1), (2, X), (3, X), (4, X)]),
    # x/1 x/2 pair; the third read finds no pending read and stays pending; phase 2 pushes it
    ("adjacent chain x/1 x/2 x/1", ["x/1", "x/2", "x/1"], 1, [1, 0, X], [(0, 1), (2, X)]),
    # x/1 pending, second x/1 is no pair and becomes pending; x/2 later: phase 2: read 0 pushes and enters, read 1 conflicts (erased),
    # read 3 finds no entry and starts afresh
    ("x/1 x/1 adjacent, then x/2 later", ["x/1", "x/1", "y", "x/2"], 1, [X, X, X, X], [(0, X), (1, X), (2, X), (X, 3)]),
    # the later x/2 starts a fresh entry, which the last x/1 then fills
    ("a non-adjacent second x/1", ["x/1", "y", "x/1", "z", "x/2", "w", "x/1"], 1, [X, X, X, X, 6, X, 4],
     [(0, X), (1, X), (2, X), (3, X), (6, 4), (5, X)]),
    # "ab/" has readNum 0 and is its own common name, which is also that of ab/1 and ab/2.  A readNum 0 read asks for read1: against
    # the entry left by ab/2 it fills read1; against the one left by ab/1 read1 is taken: conflict
    ("readNum 0 read named like the common name", ["ab/2", "q", "ab/", "ab/1", "r", "ab/"], 1, [2, X, 0, X, X, X],
     [(2, 0), (1, X), (3, X), (4, X), (5, X)]),
    # store_comment 1: names stay, readNum from the comment, common names equal -> sequential pairs
    ("Casava comments kept", ["m 1:N:0:ACGT", "m 2:N:0:ACGT", "k 2:N:0:ACGT", "j 1:N:0:A", "k 1:N:0:ACGT"], 1, [1, 0, 4, X, 2],
     [(0, 1), (4, 2), (3, X)]),
    # store_comment 0: m -> m/1, m/2; p/1 already ends in /x: not rewritten, its comment is dropped, readNum from the suffix (1), so
    # "p/1 2:N:0:A" is read 1 of p and conflicts with the entry of "p/1"
    ("Casava comments rewritten", ["m 1:N:0:ACGT", "m 2:N:0:ACGT", "p/1 1:N:0:A", "s", "p/1 2:N:0:A", "m/1", "t 2:N:0:A", "t/1"], 0,
     [1, 0, X, X, X, X, 7, 6], [(0, 1), (6, 7), (2, X), (3, X), (4, X), (5, X)]),
    # the same lines with the comments kept: "p/1 2:N:0:A" is read 2 of p/ and fills the entry of "p/1 1:N:0:A"; "t" and "t/1" share
    # no common name ("t" against "t/")
    ("Casava comment on a name that ends in /1, kept", ["p/1 1:N:0:A", "s", "p/1 2:N:0:A", "t 2:N:0:A", "t/1"], 1,
     [2, X, 0, X, X], [(0, 2), (1, X), (X, 3), (4, X)]),
    ("read 2 first", ["x/2", "y", "x/1"], 1, [2, X, 0], [(2, 0), (1, X)]),
    # chains: a/1 a/2 a/1 a/2 a/1 -> (0,1) (2,3), 4 left; phase 2 pushes it
    ("a longer chain", ["a/1", "a/2", "a/1", "a/2", "a/1"], 1, [1, 0, 3, 2, X], [(0, 1), (2, 3), (4, X)]),
    # a/2 a/1 a/2: pending a/2, a/1 pairs with it (earlier index is read1), a/2 pending
    ("earlier index is read1", ["a/2", "a/1", "a/2"], 1, [1, 0, X], [(0, 1), (X, 2)]),
    # comment separated by a tab, and too short to be Casava
    ("tab and short comment", ["a/1\tfoo", "a/2 1:N:0", "b/1 x"], 0, [1, 0, X], [(0, 1), (2, X)]),
]


# ---- the seeded generator ------------------------------------------------------------------------------------------------
def generate(seed, n_fragments=300):
    """name lines that take every branch of identifyPairs: interleaved pairs in all three suffix styles and with Casava comments,
    an R1 block with its R2 block later, read-2-first pairs, singles, chains, duplicated names (both conflict branches), readNum 0
    reads named like a common name, names of length <= 2"""
    rng = np.random.RandomState(seed)
    styles = [("/1", "/2"), ("/A", "/B"), ("/F", "/R"), (" 1:N:0:ACGT", " 2:N:0:ACGT")]
    lines, later = [], []
    for f in range(n_fragments):
        base = "frag%d_%d" % (seed, f)
        s1, s2 = styles[rng.randint(len(styles))]
        kind = rng.randint(12)
        if kind < 3:
            lines += [base + s1, base + s2]
        elif kind == 3:
            lines.append(base + s1); later.append(base + s2)
        elif kind == 4:
            lines.append(base + s2); later.append(base + s1)
        elif kind == 5:
            lines.append(base if rng.randint(2) else base + " some comment")
        elif kind == 6:
            lines += [base + s1, base + s2, base + s1] + ([base + s2, base + s1] if rng.randint(2) else [])
        elif kind == 7:          # duplicated read 1 / read 2, not adjacent to its twin
            dup = s1 if rng.randint(2) else s2
            lines.append(base + dup); later.append(base + dup); later.append(base + (s2 if dup == s1 else s1))
        elif kind == 8:          # a readNum 0 read named as the common name of a /x read
            lines.append(base + ("/2" if rng.randint(2) else "/1")); later.append(base + "/")
        elif kind == 9:
            lines.append(["/1", "/2", "x", "a/", "/"][rng.randint(5)])
        elif kind == 10:         # a rewritten Casava name against an old-style one
            lines.append(base + " 1:N:0:A"); later.append(base + "/2")
        else:
            lines += [base + s1, base + s1]; later.append(base + s2)
    rng.shuffle(later)
    return lines + later


def fastq_text(name_lines, read_len=8):
    """FASTQ text with these name lines (short fixed bases: the names are what matters)"""
    seq = ("ACGTTGCA" * (read_len // 8 + 1))[:read_len]
    qual = "I" * read_len
    return "".join("@%s\n%s\n+\n%s\n" % (l, seq, qual) for l in name_lines).encode()
