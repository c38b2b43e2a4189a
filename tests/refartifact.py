"""The artifact filter (FilterKnownOddities) restated in plain Python from the reference's source alone -- applyFilterToPair
(src/FilterKnownOddities.h:355-386), applyFilterToRead (:389-541), recordAffectedRead (:551-640), applyFilter (:663-706),
KmerArrayPair::permuteBases (src/Kmer.h:1389-1427), TwoBitSequence::compressSequence / permuteBase and the tables they use
(src/TwoBitSequence.cpp), ReadSelectorUtil::passesLength (src/ReadSelector.h:219-228) -- with nothing of the product or the
C++ oracle in it.

It keeps the reference's own data shapes, so that a misreading of the rolled-window form the oracle and the kernel share
cannot repeat here: a read is packed into two-bit bytes, a window is twoBitLength bytes at a byte pointer that starts at the
read's first byte whatever minPass is and advances one byte per hop, substitutions go through the 256 x 12 permutations table
byte by byte, and the arithmetic stays in the reference's types (SequenceLengthType = u32 and wraps, passLength = that
difference read as int, qualities are signed chars, passesLength works in f32).

Bytes past a read's two-bit buffer are undefined in the reference; the project reads zeros there, and so does this file.
`past_buffer` marks every read where a window touched such a byte while the filter held a key (with an empty filter no byte
of a window can matter).

`variant` switches one deliberate deviation on; tests/test_artifact_cases.py uses them to prove that the cases of
tests/artifactcases.py would notice it.  "The guard minAffected <= maxAffected dropped" is not among them: without a hit
minAffected = maxPass and maxAffected = minPass, and then value is 0 (or, for a forgiven repeat, set to 0), so the guard never
decides anything."""
import numpy as np

U32 = 0xffffffff

VARIANTS = ("no_odd_hop",          # drop the -1 hop when seqLen % 4 != 0
            "book_at_window",      # book a window at 4 * w, not at the reference's 4 * (minPass / 4 + w)
            "keep_left_gt",        # keep-left decision > instead of >=
            "best_swap_ge",        # best-run swap on >= instead of >
            "past_nonzero",        # bytes past the end of a short read are 0xff, not zero
            "recanonicalise",      # re-canonicalise the permuted query keys
            "first_hit",           # the first hit's value wins instead of the last
            "repeat_margin_le",    # simple-repeat margin <= 36 instead of < 36
            "unsigned_qual",       # quality bytes >= 0x80 compared unsigned
            "len_lt_1",            # passesLength: length < 1 instead of <= 1
            "min_qual_plus1",      # minimum quality char off by one
            "signed_sides",        # keep-left decision with signed differences (no u32 wrap)
            "f64_product",         # readLength * minimumLength in f64 instead of f32
            "pointer_at_min_pass")  # the byte pointer starts at minPass / 4 instead of at the read's first byte


class Config:
    """the fields of kmr_artifact_config with the reference's defaults"""
    FIELDS = (("match_length", 24), ("edit_distance", 2), ("build_edits", 2), ("simple_repeat_begin", 0), ("simple_repeat_end", 0),
              ("phix_idx", 0), ("reference_begin", 0), ("min_quality", 3), ("fastq_start_char", 33), ("min_read_length", 0.40))

    def __init__(self, **kw):
        for name, v in self.FIELDS:
            setattr(self, name, kw.pop(name, v))
        assert not kw, kw


# ------------------------------------------------------------------------------------------ TwoBitSequence.cpp's tables
def _compress_base(ch):                      # compressBase_slower; INVALID_BASE becomes 0 in compressSequence
    return {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(ch, 0)


def compress_sequence(seq):
    """compressSequence: four bases a byte, the first in bits 7..6, markup as A, trailing pad bits zero"""
    out = bytearray((len(seq) + 3) // 4)
    for off, ch in enumerate(seq):
        out[off >> 2] |= _compress_base(ch) << (6 - 2 * (off & 3))
    return bytes(out)


def _init_reverse_complement_table():
    t = []
    for c in range(256):
        comp = ~c & 0xff
        t.append(((comp << 6) & (3 << 6)) | ((comp << 2) & (3 << 4)) | ((comp >> 2) & (3 << 2)) | ((comp >> 6) & 3))
    return bytes(t)


def _init_permutations_table():
    t = []
    for i in range(256):
        row = []
        for base_idx in range(4):
            for k in range(4):
                new_base, mask = k << (6 - base_idx * 2), 3 << (6 - base_idx * 2)
                test = (i & ~mask & 0xff) | new_base
                if test != i:
                    row.append(test)
        assert len(row) == 12
        t.append(row)
    return t


RC_TABLE = _init_reverse_complement_table()
PERMUTATIONS = _init_permutations_table()


def reverse_complement(kmer):
    return bytes(RC_TABLE[b] for b in reversed(kmer))


def least_complement(kmer):
    """buildLeastComplement: the k-mer itself if it is <= its reverse complement (bytes compare as the k-mers do)"""
    rc = reverse_complement(kmer)
    return kmer if kmer <= rc else rc


def permute_bases(kmer, edit_distance, start_idx=0, out=None):
    """__permuteBases: the array order -- v1 v2 v3 of a base, then their subtrees; never re-canonicalised"""
    if out is None:
        out = []
    if edit_distance == 0:
        return out
    n_bases = 4 * len(kmer)
    for base_idx in range(start_idx, n_bases):
        byte_idx = ((base_idx + 1) + 3) // 4 - 1
        j = (base_idx & 3) * 3
        row = PERMUTATIONS[kmer[byte_idx]]
        vs = [kmer[:byte_idx] + bytes((row[j + i],)) + kmer[byte_idx + 1:] for i in range(3)]
        out.extend(vs)
        if edit_distance > 1:
            for v in vs:
                permute_bases(v, edit_distance - 1, base_idx + 1, out)
    return out


def passes_length(length, read_length, minimum_length, variant=None):
    """ReadSelectorUtil::passesLength(float length, SequenceLengthType readLength, float minimumLength)"""
    length, minimum_length = np.float32(length), np.float32(minimum_length)
    if (length < np.float32(1.0)) if variant == "len_lt_1" else (length <= np.float32(1.0)):
        return False
    if minimum_length <= np.float32(1.0):
        if variant == "f64_product":
            return bool(float(read_length) * float(minimum_length) <= float(length))
        return bool(np.float32(read_length) * minimum_length <= length)
    return bool(minimum_length <= length)


def parse_fasta(text):
    names, seqs = [], []
    for line in bytes(text).split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            names.append(line[1:].split()[0] if line[1:].split() else b"")
            seqs.append(b"")
        elif line and seqs:
            seqs[-1] += line.upper()
    return names, seqs


def _schar(b):
    return b - 256 if b >= 128 else b


class Filter:
    """the filter set and what the reference does with it.  entries = None: the set is computed here (nothing built in:
    cfg.build_edits == 0 or cfg.edit_distance == 0) -- canonical windows of the circularised sequences, the lowest sequence
    index keeps a key, reference-class sequences not circularised (they are appended after circularize(), :215-222).
    Otherwise (keys, values) of a set with substitutions built in and the number of edits left for query time."""

    def __init__(self, cfg, fasta, entries=None, remaining_edits=None):
        self.cfg = cfg
        self.length = cfg.match_length
        assert self.length % 4 == 0 and 0 < self.length <= 28
        self.two_bit_length = self.length // 4
        self.names, seqs = parse_fasta(fasta)
        self.names.insert(0, b"")
        seqs.insert(0, b"")                                  # readIdx 0 is the signal for no match
        self.n_seq = len(seqs)
        if entries is None:
            assert cfg.build_edits == 0 or cfg.edit_distance == 0
            self.num_errors = cfg.edit_distance
            self.table = {}
            for i, s in enumerate(seqs):
                if cfg.reference_begin == 0 or i < cfg.reference_begin:
                    s = s + s[:self.length]
                for j in range(len(s) - self.length + 1):
                    self.table.setdefault(least_complement(compress_sequence(s[j:j + self.length])), i)      # getOrSetElement
        else:
            self.num_errors = remaining_edits
            tb = self.two_bit_length
            self.table = {int(k).to_bytes(tb, "big"): int(v) for k, v in zip(entries[0].tolist(), entries[1].tolist())}

    def entries(self):
        items = sorted((int.from_bytes(k, "big"), v) for k, v in self.table.items())
        return np.array([k for k, _ in items], dtype=np.uint64), np.array([v for _, v in items], dtype=np.uint32)

    def is_phix(self, v):
        return self.cfg.phix_idx != 0 and v == self.cfg.phix_idx

    def is_simple_repeat(self, v):
        return self.cfg.simple_repeat_end != 0 and self.cfg.simple_repeat_begin <= v < self.cfg.simple_repeat_end

    def is_reference(self, v):
        return self.cfg.reference_begin != 0 and self.cfg.reference_begin <= v

    # ------------------------------------------------------------------------------------------- applyFilterToRead
    def screen(self, seq, qual, variant=None):
        """dict: value, min_pass, max_pass, second (first, second), remnant, past_buffer, and what the decision saw:
        pass0 (minPass, maxPass after the quality scan), affected (minAffected, maxAffected after the windows), hits"""
        cfg, length, tbl = self.cfg, self.length, self.two_bit_length
        seq_len = len(seq)
        assert len(qual) == seq_len
        nbytes = (seq_len + 3) // 4                          # getTwoBitEncodingSequenceLength
        buf = compress_sequence(seq)

        best, second, test = [0, 0], [0, 0], [0, 0]          # std::pair<long, long>
        min_qual = _schar((cfg.fastq_start_char + cfg.min_quality + (1 if variant == "min_qual_plus1" else 0)) & 0xff)      # char minQual
        if variant == "unsigned_qual":
            min_qual &= 0xff
        for i in range(seq_len):
            test[1] = i
            q = qual[i] if variant == "unsigned_qual" else _schar(qual[i])
            if q < min_qual:
                d = test[1] - test[0]
                if (d >= best[1] - best[0]) if variant == "best_swap_ge" else (d > best[1] - best[0]):
                    best, test = test, best
                if test[1] - test[0] > second[1] - second[0]:
                    second, test = test, second
                test = [i + 1, i + 1]
        test[1] = seq_len
        d = test[1] - test[0]
        if (d >= best[1] - best[0]) if variant == "best_swap_ge" else (d > best[1] - best[0]):
            best, test = test, best
        if test[1] - test[0] > second[1] - second[0]:
            second, test = test, second
        if best[1] > best[0]:
            min_pass, max_pass = best[0] & U32, best[1] & U32
        else:
            min_pass = max_pass = 0
        pass0 = (min_pass, max_pass)

        # long byteHops = ((maxPass+3)/4) - twoBitLength - (...): unsigned int arithmetic (twoBitLength is an unsigned short,
        # promoted to int and then converted), so a negative value arrives in the long as a huge positive one
        odd = 0 if (seq_len & 3) == 0 or variant == "no_odd_hop" else 1
        byte_hops = (((max_pass + 3) & U32) // 4 - tbl - odd) & U32
        if byte_hops < 0 or byte_hops > nbytes:
            byte_hops = 0

        value, was_phix, past, hits = 0, False, False, 0
        min_affected, max_affected = max_pass, min_pass
        ptr = min_pass // 4 if variant == "pointer_at_min_pass" else 0
        first_hop = min_pass // 4
        for byte_hop in range(first_hop, byte_hops + 1):
            fwd = buf[ptr:ptr + tbl]
            if len(fwd) < tbl:
                past = past or bool(self.table)
                fwd = fwd + (b"\xff" if variant == "past_nonzero" else b"\x00") * (tbl - len(fwd))
            least = least_complement(fwd)
            keys = [least]
            if self.num_errors > 0:
                permute_bases(least, self.num_errors, 0, keys)
                if variant == "recanonicalise":
                    keys = [least_complement(k) for k in keys]
            pos = ((byte_hop - first_hop if variant == "book_at_window" else byte_hop) * 4) & U32
            for k in keys:
                v = self.table.get(k)
                if v is not None:
                    if not (variant == "first_hit" and hits):
                        value = v
                    hits += 1
                    was_phix = was_phix or self.is_phix(v)
                    if min_affected > pos:
                        min_affected = pos
                    if max_affected < ((pos + length) & U32):
                        max_affected = (pos + length) & U32
            ptr += 1
        affected = (min_affected, max_affected)

        if was_phix:
            value = cfg.phix_idx
        elif self.is_simple_repeat(value):
            good, margin = True, 3 * length // 2             # (long) 3*length/2; the u32 differences widen to long unchanged
            left, right = (min_affected - min_pass) & U32, (max_pass - max_affected) & U32
            if (left <= margin) if variant == "repeat_margin_le" else (left < margin):
                good = False
            if (right <= margin) if variant == "repeat_margin_le" else (right < margin):
                good = False
            if good:
                value = 0
                min_affected, max_affected = max_pass, min_pass

        if value > 0 and min_affected <= max_affected:
            if variant == "signed_sides":
                left, right = min_affected - min_pass, max_pass - max_affected
            else:
                left, right = (min_affected - min_pass) & U32, (max_pass - max_affected) & U32
            if (left > right) if variant == "keep_left_gt" else (left >= right):
                max_pass = min_affected                      # keep the left side
            else:
                min_pass = max_affected

        remnant = False
        if value == 0 and ((max_pass - min_pass) & U32) != seq_len:
            value = self.n_seq                               # sequences.getSize(): quality trim only
            if passes_length(second[1] - second[0], seq_len, cfg.min_read_length, variant):
                remnant = True
        return dict(value=value, min_pass=min_pass, max_pass=max_pass, second=(second[0], second[1]), remnant=remnant,
                    past_buffer=past, pass0=pass0, affected=affected, hits=hits)

    # ------------------------------------------------------------- recordAffectedRead, for one read of a pair or a single
    def action(self, r1, r2, seq_len, variant=None):
        """0 untouched, 1 trimmed to [min_pass, max_pass), 2 discarded; r2 = the mate's screen or None (FilterResults(): value 0)"""
        v1, v2 = r1["value"], (r2["value"] if r2 is not None else 0)
        if v1 == 0 and v2 == 0:
            return 0
        if self.is_phix(v1) or self.is_phix(v2):
            return 2                                         # both reads of the pair are discarded
        if v1 == 0:
            return 0
        was_reference = (v1 != self.n_seq and self.is_reference(v1)) or (v2 != self.n_seq and self.is_reference(v2))
        pass_length = (r1["max_pass"] - r1["min_pass"]) & U32
        if pass_length >= 1 << 31:
            pass_length -= 1 << 32                           # int passLength
        if was_reference or pass_length <= 0 or not passes_length(pass_length, seq_len, self.cfg.min_read_length, variant):
            return 2
        return 1

    # --------------------------------------------------------------------------------------------------- applyFilter
    def apply(self, seqs, quals, mate=None, names=None, variant=None):
        """(results, reads afterwards): results = dict of arrays value, min_pass, max_pass, action, remnant_off, remnant_len (as the
        device hands them out), past_buffer, and `screens` (the list of screen() dicts); reads afterwards = (seqs, quals, names):
        trimmed reads in place, discarded reads empty, remnants appended in read order, names carried"""
        n = len(seqs)
        scr = [self.screen(seqs[i], quals[i], variant) for i in range(n)]
        res = {k: np.zeros(n, dtype=np.uint32) for k in ("value", "min_pass", "max_pass", "remnant_off", "remnant_len")}
        res["action"] = np.zeros(n, dtype=np.uint8)
        res["past_buffer"] = np.zeros(n, dtype=bool)
        out_s, out_q, out_n = [], [], []
        for i in range(n):
            m = -1 if mate is None else int(mate[i])
            a = self.action(scr[i], scr[m] if m >= 0 else None, len(seqs[i]), variant)
            r = scr[i]
            res["value"][i], res["min_pass"][i], res["max_pass"][i], res["action"][i] = r["value"], r["min_pass"], r["max_pass"], a
            res["past_buffer"][i] = r["past_buffer"]
            if r["remnant"]:
                res["remnant_off"][i], res["remnant_len"][i] = r["second"][0], r["second"][1] - r["second"][0]
            s, q = seqs[i], quals[i]
            if a == 1:
                s, q = s[r["min_pass"]:r["max_pass"]], q[r["min_pass"]:r["max_pass"]]
            elif a == 2:
                s, q = b"", b""
            out_s.append(s)
            out_q.append(q)
            out_n.append(names[i] if names is not None else b"")
        for i in range(n):                                   # the remnant is cut from the read as it was before any trim
            if scr[i]["remnant"]:
                o, l = scr[i]["second"][0], scr[i]["second"][1] - scr[i]["second"][0]
                out_s.append(seqs[i][o:o + l])
                out_q.append(quals[i][o:o + l])
                out_n.append(names[i] if names is not None else b"")
        res["screens"] = scr
        return res, (out_s, out_q, out_n)


def screen(flt, seq, qual, variant=None):
    return flt.screen(seq, qual, variant)


def apply(reads, mate, cfg, fasta=b"", entries=None, remaining_edits=None, variant=None):
    """reads = (seqs, quals) or (seqs, quals, names)"""
    flt = Filter(cfg, fasta, entries, remaining_edits)
    return flt.apply(reads[0], reads[1], mate, reads[2] if len(reads) > 2 else None, variant)
