"""FASTQ texts for the ingest tests (plain Python, no GPU): one text of a little over two of the parser's 4 KB blocks with every
name form and reads of 1 to 1000 bases, the same text behind 0..15 blank lines and in front of three kinds of end, texts cut at the
borders of a 16-byte chunk and of a block, and the limits of validateFastqStart's quality-base detection.  tests/test_ingest_cases.py
holds every text to the oracle's parser on the CPU; tests/test_gpu_ingest_device_text.py feeds them to the device parser from
device memory at every alignment.

Left out on purpose (kmr_ingest.hpp's header declares the device parser stricter than the reference there): a quality line that
is the single byte 127, and junk lines between records."""
import numpy as np

CHUNK, BLOCK = 16, 4096          # ING_BYTES, ING_THREADS * ING_BYTES of kmr_ingest.hpp
WINDOW = 20000                   # validateFastqStart looks at a read while getSize() < 20000: the first 19 999 kept reads

# (length, name form) in text order.  Every read of 255 bases or more (several rounds of ingest_copy's lane loop) is kept
# whatever store_comment is; the failed-filter reads between them shift the offsets of what follows, so the long reads' base
# offsets differ between the two settings and cover all four values of o & 3 in each (the CPU test asserts it).
_PASS, _FAIL, _SLASH, _TAB, _PLAIN = range(5)
_SUFFIX = {_PASS: b" 1:N:0:ACGT", _FAIL: b" 2:Y:0:ACGT", _SLASH: b"/1 1:Y:0:ACGT", _TAB: b"\tsome comment", _PLAIN: b""}
_BASE_READS = [(1, _PASS), (260, _SLASH), (2, _FAIL), (263, _TAB), (3, _PLAIN), (259, _PASS), (1000, _PLAIN), (150, _SLASH), (7, _PASS),
               (6, _PLAIN), (400, _SLASH), (4, _FAIL), (257, _TAB), (13, _FAIL), (256, _PASS), (5, _SLASH), (516, _TAB), (64, _PLAIN),
               (255, _PASS), (100, _FAIL), (10, _TAB), (9, _FAIL), (300, _PLAIN), (31, _PASS), (11, _SLASH), (8, _TAB), (12, _PLAIN)]
# these records start six bytes in front of a block border (the name line of the record before them is padded), so the blank lines
# of framed() carry their line starts up to, onto and over the border
_ANCHORS = {(7, _PASS): BLOCK - 6, (10, _TAB): 2 * BLOCK - 6}


def record(name_line, seq, qual, plus=b""):
    return b"@" + name_line + b"\n" + seq + b"\n+" + plus + b"\n" + qual + b"\n"


def base_records():
    """[(record bytes, failed the Casava filter)]: Casava pass and fail, /1 with a comment, tab comments, '+name' lines, lower
    case, N, quality lines that begin with '@' and with '+'.  Quality characters lie in [35, 73]: no read is out of range."""
    rng = np.random.default_rng(20)
    parts = []
    for i, (L, kind) in enumerate(_BASE_READS):
        seq = rng.choice(list(b"ACGTN"), size=L, p=[.24, .24, .24, .24, .04]).astype(np.uint8).tobytes()
        if i % 7 == 0:
            seq = seq.lower()
        elif i % 7 == 3:
            seq = seq[:L // 2].lower() + seq[L // 2:]
        q = bytearray((rng.integers(2, 41, size=L) + 33).astype(np.uint8).tobytes())
        if i % 4 == 1:
            q[0] = ord("@")
        elif i % 4 == 3:
            q[0] = ord("+")
        name = b"b%d" % i + _SUFFIX[kind]
        parts.append([name, seq, bytes(q), name if i % 3 == 0 else b""])
    out, pos = [], 0
    for i, (name, seq, q, plus) in enumerate(parts):
        nxt = _ANCHORS.get(_BASE_READS[i + 1]) if i + 1 < len(parts) else None
        if nxt is not None:
            pad = nxt - pos - len(record(name, seq, q, plus))
            assert 0 <= pad < 256, pad
            name += b"x" * pad
        out.append((record(name, seq, q, plus), _BASE_READS[i][1] == _FAIL))
        pos += len(out[-1][0])
    return out


def base_text():
    return b"".join(r for r, _ in base_records())


def base_reads(store_comment=True):
    """how many reads base_text() holds: the failed-filter records are dropped only where comments are stored (without them the
    reference looks two characters further on and finds no 'Y')"""
    recs = base_records()
    return sum(1 for _, failed in recs if not (failed and store_comment))


TAILS = {"one": b"\n", "none": b"", "three": b"\n\n\n"}


def framed(text, lead, tail):
    """`lead` blank lines (0..15 newline bytes) in front -- every line start moves through all 16 positions of a chunk and across the
    block borders -- and the end given by `tail`: one newline, none, or three"""
    assert 0 <= lead < CHUNK
    return b"\n" * lead + text.rstrip(b"\n") + TAILS[tail]


TAIL_LENGTHS = (4095, 4096, 4097, 4104, 8192)          # len % 16 = 15, 0, 1, 8, 0; a block border, one short of it, one past it


def tail_cases():
    """[(label, text, reads with comments stored)]: texts of exactly TAIL_LENGTHS bytes that end in a newline ("nl") or in the last
    quality character ("cut"), the last record a 100-base read whose comment is padded to reach the length; and one text shorter
    than a chunk"""
    recs = base_records()
    seq, qual = b"ACGTNacgtn" * 10, b"I5+@#IIII?" * 10
    out = []
    for target in TAIL_LENGTHS:
        for end in ("nl", "cut"):
            least = len(record(b"last c", seq, qual)) - (end == "cut")
            body, kept = b"", 0
            for r, failed in recs:
                if len(body) + len(r) + least > target:
                    break
                body += r
                kept += 0 if failed else 1
            last = record(b"last c" + b"x" * (target - len(body) - least), seq, qual)
            text = body + (last[:-1] if end == "cut" else last)
            assert len(text) == target
            out.append(("%d/%s" % (target, end), text, kept + 1))
    out.append(("short", b"@a\nA\n+\nI", 1))
    return out


# ---- quality-base detection -------------------------------------------------------------------------------------------------
_ONE = b"@r\nA\n+\nI\n"


def _window_text(bad_kept_index, skipped_before=()):
    """WINDOW + 1 kept 1-base reads of quality 'I', the one at `bad_kept_index` of quality 'J' (74 > 33 + 40); in front of the kept
    reads listed in `skipped_before`, a record that fails the Casava filter and whose quality is out of range as well"""
    kept = [_ONE] * (WINDOW + 1)
    kept[bad_kept_index] = b"@r\nA\n+\nJ\n"
    failed = b"@f 1:Y:0:A\nA\n+\nJ\n"
    out = []
    at = sorted(skipped_before)
    for i, r in enumerate(kept):
        out += [failed] * at.count(i)
        out.append(r)
    return b"".join(out)


def _reads(*quals, seq=None):
    """a text of one read per quality string"""
    return b"".join(record(b"q%d" % i, (b"ACGT" * (len(q) // 4 + 1))[:len(q)] if seq is None else seq, q) for i, q in enumerate(quals))


def quality_cases():
    """[(label, text, start_char, input_base, expected_final_base)]; the label's first part is the group.  Comments are stored in
    every case.  quality_case_reads() gives the number of reads of each."""
    last, skip_flip, skip_keep = WINDOW - 2, (0, 0, 5000, 19990, 19997, 19998), (0, 0, 5000, 19990, 19998, 19999)
    long_q = bytearray(b"h" * 400)
    long_q[300] = ord("?")                                # the only character below 64: dword 75 of its read, lane 11's second round
    cases = [
        # the only out-of-range read is kept read number 19 999 / 20 000
        ("window/flip", _window_text(last), 33, 33, 64),
        ("window/no-flip", _window_text(last + 1), 33, 33, 33),
        ("window/skipped-flip", _window_text(last, skip_flip), 33, 33, 64),
        ("window/skipped-no-flip", _window_text(last + 1, skip_keep), 33, 33, 33),
        # both bounds are taken on the read's MINIMUM: a read whose minimum is 73 may hold 75
        ("bounds/33-min-33", _reads(b"II", b"I!IK", b"III"), 33, 33, 33),
        ("bounds/33-min-73", _reads(b"II", b"KIJ", b"III"), 33, 33, 33),
        ("bounds/33-min-74", _reads(b"II", b"KJL", b"III"), 33, 33, 64),
        ("bounds/64-min-64", _reads(b"hh", b"h@h", b"hhh"), 64, 64, 64),
        ("bounds/64-min-63", _reads(b"hh", b"h?h", b"hhh"), 64, 64, 33),
        ("bounds/64-min-104", _reads(b"hh", b"jhi", b"hhh"), 64, 64, 64),
        ("bounds/64-min-105", _reads(b"hh", b"jik", b"hhh"), 64, 64, 33),
        # start 33 wants to flip to 64, which the input already is: '5' rescales to 22 < 33 and nothing happens
        ("same-base/33-from-64", _reads(b"hh", b"h5h", b"hhh"), 33, 64, 64),
        # a read whose first rescaled quality is 127 is exempt although its minimum (74) is out of range; not so in second place
        ("exempt/127-first", _reads(b"II", b"\x7fJK", b"III"), 33, 33, 33),
        ("exempt/127-second", _reads(b"II", b"J\x7fK", b"III"), 33, 33, 64),
        # where the offending character sits: beyond the first round of the 64 lanes; the first / last byte of a read whose output
        # offset is 1, in a partial head / tail dword of ingest_copy (offsets 1..6 of the output: dwords 0 and 1, both partial)
        ("position/300-of-400", _reads(b"hhh", bytes(long_q), b"hh"), 64, 64, 33),
        ("position/first-byte", _reads(b"h", b"?hhhhh", b"hh"), 64, 64, 33),
        ("position/last-byte", _reads(b"h", b"hhhhh?", b"hh"), 64, 64, 33),
        # CR is data to the reference's getline and to the device: it ends up in bases and quals, and as quality 13 it flips the base
        ("crlf/text", _reads(b"IIII", b"I5I", b"II").replace(b"\n", b"\r\n"), 33, 33, 64),
    ]
    return cases


def quality_case_reads(label):
    return WINDOW + 1 if label.startswith("window/") else 3


def device_quality_cases():
    """the cases the device form repeats: every window case and the first of each other group"""
    seen, out = set(), []
    for c in quality_cases():
        group = c[0].split("/")[0]
        if group == "window" or group not in seen:
            out.append(c)
        seen.add(group)
    return out


# ---- reads for the two-bit round trip ---------------------------------------------------------------------------------------
TWOBIT_LENGTHS = (0, 1, 3, 259, 260, 261, 262, 263, 516, 1000, 1027)


def twobit_reads():
    """sequences for the two-bit round trip: each of TWOBIT_LENGTHS four times, behind a short read chosen so that the long read's
    base offset takes each value mod 4; N, '.', other codes and lower-case acgt here and there, and in fixed places beyond position 256"""
    rng = np.random.default_rng(29)
    alphabet = np.frombuffer(b"ACGTacgtN.XRY", dtype=np.uint8)
    p = [.225] * 4 + [.02] * 4 + [.004] * 5          # few enough markups that most 31-mers of a read are clean
    seqs, o = [], 0
    for L in TWOBIT_LENGTHS:
        for want in range(4):
            short = (want - o) % 4 + (4 if (L + want) % 3 else 0)          # 0..7 bases, so that (o + short) % 4 == want
            s = bytearray(rng.choice(alphabet, size=short, p=p).tobytes())
            seqs.append(bytes(s)); o += short
            assert o % 4 == want
            s = bytearray(rng.choice(alphabet, size=L, p=p).tobytes())
            for pos, c in ((257, b"N"), (258, b"c"), (300, b"."), (515, b"X"), (L - 1, b"N"), (L - 2, b"g")):
                if 256 < pos < L:
                    s[pos] = c[0]
            seqs.append(bytes(s)); o += L
    return seqs
