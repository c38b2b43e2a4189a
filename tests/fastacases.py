"""FASTA and FASTA+QUAL texts for the FASTA ingest tests (plain Python, no GPU), in the manner of ingestcases.py: every line width
around the parser's 16-byte chunk and 4 KB block, records of one, two and many lines, a long record on one line and in 60-column
lines, a header at every position of a chunk and astride a block border, every kind of end, the characters a sequence line may hold,
the Casava comments, one refused text per rule, and for the QUAL side the clamp, the separators, the joined lines and the limits of
the quality-base detection.  tests/test_fasta_cases.py holds every text to tests/reffasta.py on the CPU; tests/test_gpu_fasta_ingest.py
feeds them to kmr_ingest_fasta and kmr_ingest_fasta_dev.

A case: label, text, qual (None: plain FASTA), start (the handle's fastq_start_char), store_comment, and for a refused text
refused = (the cause as the library's message names it, what the reference does: "differ" = its stream and mmap forms give different
results, "throws" = both throw, "mangles" = both go on with something that is not the file's content)."""
import numpy as np

CHUNK, BLOCK = 16, 4096          # ING_BYTES, ING_THREADS * ING_BYTES of kmr_ingest.hpp
WINDOW = 20000                   # validateFastqStart looks at a read while getSize() < 20000: the first 19 999 kept reads
WIDTHS = (1, 15, 16, 17, 60, 4095, 4096, 4097)

_rng = np.random.default_rng(44)


def seq(n, alphabet=b"ACGT"):
    return _rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tobytes()


def wrap(s, width):
    return b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width))


def case(label, text, qual=None, start=33, store_comment=True, refused=None):
    return {"label": label, "text": text, "qual": qual, "start": start, "store_comment": store_comment, "refused": refused}


def qual_lines(values, width=None, sep=b" ", tail=b" "):
    """the numbers in lines of `width` numbers (None: one line), each line ending in `tail`"""
    width = width or max(1, len(values))
    return b"".join(sep.join(b"%d" % v for v in values[i:i + width]) + tail + b"\n" for i in range(0, len(values), width))


def _mixed():
    """a text of a little over two blocks: short and long records, every name form, blank lines here and there"""
    names = [b"m0 1:N:0:ACGT", b"m1/1 1:Y:0:ACGT", b"m2 2:Y:0:ACGT", b"m3\tsome comment", b"m4", b"m5/2", b"m6 1:Y:0:A", b"m7 x", b"m8 2:N:0:TT"]
    lens = [1, 61, 120, 7, 300, 59, 60, 1000, 33, 2, 517, 64, 4, 181, 250, 2400, 3, 900, 16, 15, 17, 1200]
    out = b""
    for i, n in enumerate(lens):
        s = seq(n, b"ACGTacgtN")
        out += b">" + names[i % len(names)] + b"%d" % i + b"\n" + wrap(s, (60, 70, 1000, 13)[i % 4]) + (b"\n" * (i % 5 == 3)) + (b"\n\n" * (i % 7 == 6))
    return out


def fasta_cases():
    out = [case("empty", b"")]
    for w in WIDTHS:
        for nlines, tag in ((1, "one"), (2, "two"), (5, "many")):
            n = w * nlines - (w // 2 if nlines == 5 and w > 1 else 0)          # the last of many lines is shorter
            out.append(case("width/%d/%s" % (w, tag), b">a\n" + wrap(seq(7), w) + b">w%d some comment\n" % w + wrap(seq(n), w) + b">z\n" + wrap(seq(w + 3), w)))
    long_seq = seq(20000, b"ACGTN")
    out.append(case("long/one-line", b">chr1 a genome\n" + long_seq + b"\n"))
    out.append(case("long/60-columns", b">chr1 a genome\n" + wrap(long_seq, 60)))
    out.append(case("long/one-line-no-newline", b">s\nAC\n>chr1\n" + long_seq))
    for off in range(CHUNK):                             # the second header starts at BLOCK - 8 + off: every position of a chunk, astride the border
        lead = BLOCK - 8 + off - len(b">p\n") - 1
        out.append(case("header-at/%d" % off, b">p\n" + seq(lead) + b"\n>header_%02d with a comment\n" % off + wrap(seq(200), 60)))
        assert out[-1]["text"].index(b">header") == BLOCK - 8 + off
    body = b">a\nACGT\nAC\n>b\nGG\n"
    out.append(case("end/newline", body))
    out.append(case("end/none", body[:-1]))
    out.append(case("end/three-newlines", body + b"\n\n"))
    out.append(case("end/one-base-no-newline", b">a\nA"))
    out.append(case("blank/between-records", b">a\nACGT\nAC\n\n>b\nGG\n\n\n\n>c\nT\n"))
    out.append(case("cr/before-newline", body.replace(b"\n", b"\r\n")))
    out.append(case("cr/alone-on-a-line", b">a\nAC\n\r\nGT\n"))          # a line of one '\r' is not empty
    out.append(case("letters/lower-N-iupac-dot", b">a\nacgtnACGTN\nRYKMSWBDHVrykmswbdhv\n..N..x*-\n>b\n>inside is no header\n".replace(b">inside", b"A>inside")))
    casava = b">r1 1:N:0:ACGT\nAAAA\n>r2 1:Y:0:ACGT\nCCCC\n>r3/1 1:Y:0:ACGT\nGGGG\n>r4 2:N:0:A\nTTTT\n>r5 2:Y:0:A\nACAC\n>r6/2 2:N:0:A\nGTGT\n>r7 1:Y:0\nAA\n>r8\t1:Y:0:A\nCC\n"
    for sc in (True, False):
        out.append(case("casava/%s" % ("stored" if sc else "not-stored"), casava, store_comment=sc))
        out.append(case("mixed/%s" % ("stored" if sc else "not-stored"), _mixed(), store_comment=sc))
    out.append(case("casava/all-dropped", b">r2 1:Y:0:ACGT\nCCCC\nAA\n>r5 2:Y:0:A\nACAC\n"))
    # one refused text per rule
    out += [
        case("refused/text-before-header", b"ACGT\n>a\nAC\n", refused=("text or an empty line before the first header", "differ")),
        case("refused/empty-line-first", b"\n>a\nAC\n", refused=("text or an empty line before the first header", "differ")),
        case("refused/only-newlines", b"\n\n", refused=("text or an empty line before the first header", "differ")),
        case("refused/header-header", b">a\n>b\nAC\n", refused=("a header followed by a header", "differ")),
        case("refused/header-at-end", b">a\nAC\n>b\n", refused=("a header at the end of the text", "mangles")),
        case("refused/header-at-end-no-newline", b">a\nAC\n>b", refused=("a header at the end of the text", "mangles")),
        case("refused/empty-line-before-sequence", b">a\n\nAC\n>b\nGG\n", refused=("an empty line before or between the lines of a record", "differ")),
        case("refused/empty-line-between-sequence", b">a\nAC\n\nGT\n>b\nGG\n", refused=("an empty line before or between the lines of a record", "differ")),
        case("refused/empty-name", b">a\nAC\n>\nGT\n>c\nGG\n", refused=("an empty name", "mangles")),
        case("refused/empty-name-with-comment", b">a\nAC\n> x\nGT\n>c\nGG\n", refused=("an empty name", "mangles")),
    ]
    return out


def _window(bad, start):
    """WINDOW + 1 one-base reads of quality 30, the one at index `bad` of quality 41 (above start + 40)"""
    f = b">r\nA\n" * (WINDOW + 1)
    q = [b">r\n30 \n"] * (WINDOW + 1)
    q[bad] = b">r\n41 \n"
    return case("window/%d/%d" % (start, bad), f, b"".join(q), start=start)


def qual_cases():
    out = [case("qual/empty", b"", b"")]
    vals = [0, 40, 41, 93, 94, 999, 7, 100, 62, 63, 5, 39]
    f1 = b">a\n" + seq(len(vals)) + b"\n"
    for start in (33, 64):
        out.append(case("values/%d" % start, f1 + b">b\nAC\n", b">a\n" + qual_lines(vals) + b">b\n1 2\n", start=start))
    out.append(case("separators/tabs-and-runs", f1, b">a\n \t 0\t40  41 \t\t93 94   999\t\n7\t100 \n  62 63\t\n\t5 39\n"))
    out.append(case("separators/leading-and-trailing-blanks", f1, b">a\n   " + qual_lines(vals, tail=b"   ")))
    out.append(case("separators/no-trailing-blank-last-line", f1, b">a\n" + qual_lines(vals, 5)[:-2]))
    out.append(case("separators/digit-then-blank-start", b">a\nACGT\n", b">a\n1 2\n 3 4\n"))          # a line may end in a digit where the next starts with a blank
    n = 333
    big = list(_rng.integers(0, 61, size=n))
    fbig = b">big x\n" + wrap(seq(n), 60) + b">small\nACG\n\n>third 1:N:0:A\n" + wrap(seq(100), 17)
    small = [3, 2, 1]
    third = list(_rng.integers(0, 130, size=100))
    out.append(case("lines/one-line-records", fbig, b">big\n" + qual_lines(big) + b">small\n" + qual_lines(small) + b">third 1:N:0:A\n" + qual_lines(third)))
    for sc in (True, False):
        out.append(case("lines/many-line-records/%s" % ("stored" if sc else "not-stored"), fbig,
                        b">big y\n" + qual_lines(big, 25) + b"\n>small other comment\n" + qual_lines(small, 1) + b">third 1:N:0:A\n" + qual_lines(third, 60) + b"\n\n", store_comment=sc))
    # records across the 4 KB blocks of the QUAL text, numbers astride their borders
    recs = [(b"q%d" % i, seq(int(L))) for i, L in enumerate(_rng.integers(1, 400, size=40))]
    ftxt = b"".join(b">" + nm + b"\n" + wrap(s, 70) for nm, s in recs)
    for width, tag in ((None, "one-line"), (20, "20-per-line")):
        qtxt = b"".join(b">" + nm + b"\n" + qual_lines(list(_rng.integers(0, 130, size=len(s))), width) for nm, s in recs)
        assert len(qtxt) > 4 * BLOCK
        out.append(case("blocks/%s" % tag, ftxt, qtxt))
    # the Casava filter is the FASTA header's; a dropped record's numbers are never counted
    out.append(case("dropped/by-fasta-header", b">a 1:Y:0:A\nACGT\n>b\nGG\n", b">a 1:Y:0:A\n1 2 3\n>b\n4 5\n"))
    out.append(case("dropped/qual-comment-differs", b">a 1:N:0:A\nACGT\n>b\nGG\n", b">a 1:Y:0:A\n1 2 3 4\n>b\n4 5\n"))
    for start in (33, 64):
        for bad in (0, WINDOW - 2, WINDOW - 1):
            out.append(_window(bad, start))
    out.append(case("flip/long-read-one-low", b">a\n" + seq(500) + b"\n>b\nAC\n", b">a\n" + qual_lines([50] * 300 + [40] + [50] * 199, 30) + b">b\n1 2 \n"))
    out.append(case("flip/second-read-all-high", b">a\nAC\n>b\n" + seq(500) + b"\n", b">a\n1 2 \n>b\n" + qual_lines([50] * 500, 30)))
    out += [
        case("refused/qual-glued", f1, b">a\n" + qual_lines(vals, 4, tail=b""), refused=("a quality line ends in a digit and the next one starts with a digit", "throws")),
        case("refused/qual-glued-count-fits", b">a\n" + seq(len(vals) - 2) + b"\n", b">a\n" + qual_lines(vals, 4, tail=b""), refused=("a quality line ends in a digit and the next one starts with a digit", "mangles")),
        case("refused/qual-count", f1, b">a\n" + qual_lines(vals[:-1]), refused=("number of bases and quals not equal", "throws")),
        case("refused/qual-count-more", f1 + b">b\nAC\n", b">a\n" + qual_lines(vals + [1]) + b">b\n1 \n", refused=("number of bases and quals not equal", "throws")),
        case("refused/qual-record-count", f1 + b">b\nAC\n", b">a\n" + qual_lines(vals), refused=("records for the", "throws")),
        case("refused/qual-record-count-more", f1, b">a\n" + qual_lines(vals) + b">b\n1 2 \n", refused=("records for the", "differ")),
        case("refused/qual-name", f1 + b">b\nAC\n", b">a\n" + qual_lines(vals) + b">c\n1 2 \n", refused=("fasta and quals have different names", "throws")),
        case("refused/qual-name-pair-digit", b">a 1:N:0:A\nAC\n", b">a 2:N:0:A\n1 2 \n", store_comment=False, refused=("fasta and quals have different names", "throws")),
        case("refused/qual-byte", b">a\nACGT\n", b">a\n1 2 x 4\n", refused=("a byte that is no digit, blank or tab in a quality line", "throws")),
        case("refused/qual-empty-line", b">a\nACGT\n", b">a\n1 2 \n\n3 4 \n", refused=("an empty line before or between the lines of a record", "differ")),
        case("refused/qual-header-header", f1 + b">b\nAC\n", b">a\n>b\n1 2 \n", refused=("a header followed by a header", "throws")),
    ]
    return out


def all_cases():
    return fasta_cases() + qual_cases()
