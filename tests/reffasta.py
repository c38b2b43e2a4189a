"""The reference's FASTA and FASTA+QUAL readers restated in plain Python, line by line from its source: the independent reference of
the FASTA ingest tests (the oracle has no FASTA reader).

  parse_stream   ReadFileReader::nextRead(name, bases, quals, comment) (src/ReadFileReader.h:299-332) over FastaStreamParser /
                 FastaQualStreamParser::readRecord() (:844-1006), SequenceStreamParser::readName / nextLine (:449-458,584-617),
                 with std::getline, peek and eof as an istream over the text behaves
  parse_mmap     the mapped-file form: FastaStreamParser::readRecord(RecordPtr) (:868-896) and, for the qualities, the FASTA
                 branch of SequenceRecordParser::parse (src/Utils.h:617-645) with nextLine(buffer, RecordPtr) (:548-558), under
                 ReadFileReader::nextRead(RecordPtr &) (:262-287)
  trim_name, is_comment_casava18, convert_qual_ints_to_chars   src/Utils.h:561-598, 678-685, 652-667
  add_reads      ReadSet::appendFasta + addRead + validateFastqStart + __setFastqStart (src/ReadSet.cpp:136-141,310-345,
                 src/ReadSet.h:171-209, src/Sequence.h:456-479) with inputReadQualityBase == Read::FASTQ_START_CHAR at the start
  accepted       the language kmr_ingest_fasta accepts (include/kmernator_amd.h)

The mapped form finds a line's end with strchr; a last line without '\\n' is modelled as ending at the end of the text."""
import re

REF_QUAL = 127
VALIDATE_READS = 20000


class RefThrow(Exception):
    """LOG_THROW of the reference"""


# ---- src/Utils.h ------------------------------------------------------------------------------------------------------------
def is_comment_casava18(c):
    return len(c) >= 6 and c[1:2] == b":" and c[3:4] == b":" and c[5:6] == b":" and c[0:1] in (b"1", b"2") and c[2:3] in (b"Y", b"N")


def trim_name(name_line, store_comment):
    """(name, comment, isGood); name_line with its marker"""
    if len(name_line) == 0:
        return b"", b"", False
    good = True
    if name_line[0:1] not in (b">", b"@"):
        raise RefThrow("Can not parse name without a marker")
    n = bytearray(name_line[1:])
    comment = b""
    m = re.search(rb"[ \t\r\n]", bytes(n))
    if m:
        pos = m.start()
        if len(n) >= pos + 2:
            comment = bytes(n[pos + 1:])
            if is_comment_casava18(comment) and (pos <= 2 or n[pos - 2:pos - 1] != b"/"):
                if not store_comment:
                    n[pos] = ord("/")
                    pos += 2
                if n[pos + 3:pos + 4] == b"Y":
                    good = False
        del n[pos:]
    return bytes(n), comment, good


def convert_qual_ints_to_chars(qual_ints, start):
    """istringstream >> int until it fails: (characters, everything was consumed)"""
    out = bytearray()
    top = REF_QUAL - start - 1
    pos, n = 0, len(qual_ints)
    ws = b" \t\n\v\f\r"
    while True:
        while pos < n and qual_ints[pos] in ws:
            pos += 1
        m = re.match(rb"[+-]?[0-9]+", qual_ints[pos:])
        if not m:
            break
        v = int(m.group())
        if not -2 ** 31 <= v < 2 ** 31:
            break
        pos += m.end()
        out.append((min(v, top) + start) & 0xff)
    return bytes(out), pos == n


# ---- an istream over the text -----------------------------------------------------------------------------------------------
class _IStream:
    def __init__(self, text):
        self.t, self.pos, self.eof = bytes(text), 0, False

    def getline(self):
        if self.eof or self.pos >= len(self.t):
            self.eof = True
            return b""
        nl = self.t.find(b"\n", self.pos)
        if nl < 0:
            line, self.pos, self.eof = self.t[self.pos:], len(self.t), True
        else:
            line, self.pos = self.t[self.pos:nl], nl + 1
        return line

    def peek(self):
        if self.eof or self.pos >= len(self.t):
            self.eof = True
            return -1
        return self.t[self.pos]


class _FastaStreamParser:
    def __init__(self, text, store_comment):
        self.s, self.sc = _IStream(text), store_comment
        self.name = self.comment = self.bases = b""
        self.good = False
        self.lines = []

    def read_name(self):
        name = self.s.getline()
        self.comment = b""
        count = 0
        while len(name) == 0 or name[0:1] != b">":
            if self.s.eof:
                self.name, self.good = b"", False
                return self.name
            name = self.s.getline()
            count += 1
            if count > 100000:
                break
        if len(name) == 0:
            self.name, self.good = b"", False
            return self.name
        if name[0:1] != b">":
            raise RefThrow("Missing name marker")
        self.raw = name[1:]
        self.name, self.comment, self.good = trim_name(name, self.sc)
        return self.name

    def get_bases_or_quals(self):
        self.bases, self.lines = b"", []
        while not self.s.eof:
            line = self.s.getline()
            if len(line) == 0:
                break
            self.bases += line
            self.lines.append(line)
            if self.s.peek() == ord(">"):
                break
        return self.bases


def _next_read(read_record, state):
    """nextRead(name, bases, quals, comment): one kept read or None; counts the skipped failed-filter reads"""
    rec = read_record()
    while rec["name"] and not rec["good"]:
        state["filtered"] += 1
        rec = read_record()
    if not rec["name"]:
        return None
    rec["bases"] = bytes(c - 32 if 97 <= c <= 122 else c for c in rec["bases"])
    if len(rec["quals"]) != len(rec["bases"]) and not (len(rec["quals"]) == 1 and rec["quals"][0] == REF_QUAL):
        raise RefThrow("Number of bases and quals not equal")
    return rec


def parse_stream(text, qual_text=None, start=33, store_comment=True):
    """{"reads": [{name, raw, comment, bases, quals}], "filtered", "mangled"} or raises RefThrow.  mangled: the reference went on
    with something no reader of the file would call its content -- a read without bases, or quality lines whose numbers came out
    differently from what each line says (lines joined without a separator, conversion stopped at a byte it could not read), or
    an end of input in mid-file at an empty name"""
    f = _FastaStreamParser(text, store_comment)
    q = None if qual_text is None else _FastaStreamParser(qual_text, store_comment)
    state = {"filtered": 0, "mangled": False}

    def read_record():
        if q is not None:
            qn = q.read_name()
            if f.read_name() != qn:
                raise RefThrow("fasta and quals have different names")
        else:
            f.read_name()
        if not f.name:
            if f.s.pos < len(f.s.t):
                state["mangled"] = True                  # an empty name in mid-file ends the input without a word
            return {"name": b"", "good": False}
        bases = f.get_bases_or_quals()
        if q is None:
            quals = bytes([REF_QUAL]) * len(bases)
        else:
            ints = q.get_bases_or_quals()
            quals, whole = convert_qual_ints_to_chars(ints, start)
            per_line = [convert_qual_ints_to_chars(l, start) for l in q.lines]
            if not whole or quals != b"".join(c for c, _ in per_line) or not all(w for _, w in per_line):
                state["mangled"] = True
        if len(bases) == 0:
            state["mangled"] = True
        return {"name": f.name, "raw": f.raw, "comment": f.comment, "good": f.good, "bases": bases, "quals": quals}

    reads = []
    while True:
        rec = _next_read(read_record, state)
        if rec is None:
            break
        reads.append(rec)
    return {"reads": reads, "filtered": state["filtered"], "mangled": state["mangled"]}


# ---- the mapped-file form ---------------------------------------------------------------------------------------------------
def _next_line(t, p):
    """SequenceRecordParser::nextLine(buffer, recordPtr): (line, pointer behind its newline)"""
    nl = t.find(b"\n", p)
    if nl < 0:
        nl = len(t)
    return t[p:nl], nl + 1


def parse_mmap(text, qual_text=None, start=33, store_comment=True):
    t = bytes(text)
    qt = None if qual_text is None else bytes(qual_text)
    pos = {"f": 0, "q": 0}
    state = {"filtered": 0, "mangled": False}

    def read_record():
        p = pos["f"]
        if p >= len(t):                                   # isPastPartition
            return {"name": b"", "good": False}
        if t[p:p + 1] != b">":
            raise RefThrow("FastaStreamParser::readRecord(): Could not FastaStreamParser::readRecord()")
        line, p = _next_line(t, p)
        name, comment, good = trim_name(line, store_comment)
        bases = b""
        while p < len(t) and t[p:p + 1] != b">":
            l, p = _next_line(t, p)
            bases += l
        pos["f"] = p
        if qt is None:
            quals = bytes([REF_QUAL]) * len(bases)
        else:
            qp = pos["q"]
            buf, qp = _next_line(qt, qp)
            qname = trim_name(buf, store_comment)[0]
            if qname != name:
                raise RefThrow("fasta and qual do not match names!")
            ints = b""
            while qp < len(qt) and qt[qp:qp + 1] != b">":
                l, qp = _next_line(qt, qp)
                ints += l
            pos["q"] = qp
            quals = convert_qual_ints_to_chars(ints, start)[0]
        return {"name": name, "raw": line[1:], "comment": comment, "good": good, "bases": bases, "quals": quals}

    reads = []
    while True:
        rec = _next_read(read_record, state)
        if rec is None:
            break
        reads.append(rec)
    return {"reads": reads, "filtered": state["filtered"], "mangled": False}


def outcome(fn, *a, **kw):
    """("ok", result without the mangled flag) or ("throws", None)"""
    try:
        r = fn(*a, **kw)
    except RefThrow:
        return "throws", None
    return "ok", ([(x["name"], x["comment"], x["bases"], x["quals"]) for x in r["reads"]], r["filtered"])


# ---- ReadSet ----------------------------------------------------------------------------------------------------------------
def add_reads(reads, start=33):
    """(quality strings as the ReadSet ends up holding them, final inputReadQualityBase)"""
    input_base = start
    held = []
    for r in reads:
        q = r["quals"]
        if input_base != start:
            q = bytes((c + start - input_base) & 0xff for c in q)
        held.append(q)
        if len(held) < VALIDATE_READS and len(q) and q[0] != REF_QUAL:
            mn = min(q)
            if mn < start or mn > start + 40:
                other = 64 if start == 33 else 33
                if other != input_base:
                    delta = input_base - other
                    held = [bytes((c + delta) & 0xff for c in x) for x in held]
                    input_base = other
    return held, input_base


def parse(text, qual_text=None, start=33, store_comment=True):
    """what a batch ingested from the text must hold: n, filtered, base, bases, quals, offsets, names (the header behind '>')"""
    r = parse_stream(text, qual_text, start, store_comment)
    quals, base = add_reads(r["reads"], start)
    offsets = [0]
    for x in r["reads"]:
        offsets.append(offsets[-1] + len(x["bases"]))
    return {"n": len(r["reads"]), "filtered": r["filtered"], "base": base, "bases": b"".join(x["bases"] for x in r["reads"]), "quals": b"".join(quals),
            "offsets": offsets, "names": [x["raw"] for x in r["reads"]], "trimmed": [x["name"] for x in r["reads"]]}


# ---- the accepted language --------------------------------------------------------------------------------------------------
def _records(text):
    """[(header line, [lines])] or the rule broken"""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                      # the newline that ends the last line
    recs, blank = [], False
    for i, l in enumerate(lines):
        if l[0:1] == b">":
            if recs and not recs[-1][1]:
                return "a header followed by a header"
            recs.append((l, []))
            blank = False
        elif l == b"":
            if not recs or not recs[-1][1]:
                return "text or an empty line before the first header" if not recs else "an empty line before or between the lines of a record"
            blank = True
        else:
            if not recs:
                return "text or an empty line before the first header"
            if blank:
                return "an empty line before or between the lines of a record"
            recs[-1][1].append(l)
    if recs and not recs[-1][1]:
        return "a header at the end of the text"
    for h, _ in recs:
        if trim_name(h, True)[0] == b"":
            return "an empty name"
    return recs


def refusal(text, qual_text=None, store_comment=True):
    """None if kmr_ingest_fasta accepts the text(s), else the cause as its message names it"""
    f = _records(text)
    if isinstance(f, str):
        return f
    if qual_text is None:
        return None
    q = _records(qual_text)
    if isinstance(q, str):
        return q
    for _, ls in q:
        for a, b in zip(ls, ls[1:] + [b" "]):
            if re.search(rb"[^0-9 \t]", a):
                return "a byte that is no digit, blank or tab in a quality line"
            if re.search(rb"[0-9]{4}", a):
                return "a quality of more than 3 digits"
            if a[-1:].isdigit() and b[:1].isdigit():
                return "a quality line ends in a digit and the next one starts with a digit"
    if len(q) != len(f):
        return "records for the"
    for (fh, fl), (qh, ql) in zip(f, q):
        fn, _, good = trim_name(fh, store_comment)
        if trim_name(qh, store_comment)[0] != fn:
            return "fasta and quals have different names"
        if good and sum(len(l.split()) for l in ql) != sum(len(l) for l in fl):
            return "number of bases and quals not equal"
    return None


def accepted(text, qual_text=None, store_comment=True):
    return refusal(text, qual_text, store_comment) is None


# ---- the way back: testFastaWithQualFile (test/ReadSetTest.cpp:141-166) -----------------------------------------------------
def reprint(parsed, start=33):
    fasta = qual = b""
    o = parsed["offsets"]
    for i in range(parsed["n"]):
        name_line = b">" + parsed["trimmed"][i] + b"\n"
        fasta += name_line + parsed["bases"][o[i]:o[i + 1]] + b"\n"
        qual += name_line + b"".join(b"%d " % (c - start) for c in parsed["quals"][o[i]:o[i + 1]]) + b"\n"
    return fasta, qual
