"""What FilterKnownOddities' Recorder makes of the artifact filter's decisions, restated in plain Python from the reference's source
alone -- Recorder (src/FilterKnownOddities.h:296-353), recordAffectedRead (:551-640), getFilterName (:543-550), the naming and the
table of applyFilter (:663-732), _writeFilterRead (:734-736) with Read::toFastq / getQuals (src/Sequence.cpp:729-770) and
getFastaNoMarkup of a discarded read (:290-296) -- over the dicts tests/refartifact.py's Filter.apply returns.  Nothing of the
product is in it.

The order is that of one thread: unit after unit (an entry of the pair list, read1 then read2; without a list one read), every record
into the file of the input the unit's read1 belongs to (read2's if read1 is absent).

`variant` switches one deliberate deviation on; tests/test_artifact_report_cases.py uses them to prove that the families of
tests/artifactreportcases.py would notice it."""
import numpy as np

import refartifact as ra

VARIANTS = ("bases_printed",          # prints the read's bases instead of N
            "quals_masked",           # collapses the quality line of a discarded read
            "phix_affected_only",     # leaves the clean mate of a PhiX read alone
            "phix_labelled",          # puts a label on PhiX records
            "file_of_own_read",       # files a record under its own read's input, not read1's
            "read_index_order",       # orders records by read index, not by unit
            "trim_counts_len",        # adds len, not the removed bases, for a trim
            "mate_labelled")          # writes a clean mate of a discarded read

ROWS = ("-Artifact.fastq", "-PhiX.fastq")


def filter_name(flt, v):
    """getFilterName: the header name of sequence v, or MinQualityTrim<min quality> for sequences.getSize()"""
    assert v > 0
    return flt.names[v] if v < flt.n_seq else b"MinQualityTrim%d" % flt.cfg.min_quality


def record(name, seq, qual, label, in_base, out_base, print_bases=False, variant=None):
    """Read::toFastq(0, len, label, unmasked = true) of a read that has been discarded"""
    n = len(seq)
    shown = name.split(b" ")[0].split(b"\t")[0]
    if n <= 1 or variant == "quals_masked":
        q = bytes([out_base + 1])
    else:
        q = bytes((c + out_base - in_base) & 0xff for c in qual)
    bases = seq if (print_bases or variant == "bases_printed") and n > 1 else b"N"
    return b"@" + shown + ((b" " + label) if label else b"") + b"\n" + bases + b"\n+\n" + q + b"\n"


def input_of(input_starts, r):
    if input_starts is None:
        return 0
    j = 0
    while j + 1 < len(input_starts) - 1 and input_starts[j + 1] <= r:
        j += 1
    return j


class Report:
    def __init__(self, n_seq, n_inputs):
        self.discarded, self.trimmed, self.bases = (np.zeros(n_seq + 1, dtype=np.uint64) for _ in range(3))
        self.records = [[[] for _ in range(n_inputs)] for _ in ROWS]      # [row][input] -> (read, bytes)

    def counts(self):
        return self.discarded, self.trimmed, self.bases

    def table(self, flt):
        """applyFilter :714-725"""
        s = "Final Filter Matches to reads:%d\nDiscarded Reads:%d\nTrimmed Reads:%d\nDiscarded/Trimmed Bases:%d\n\n\tDiscarded\tAffected\tBasesRemoved\tMatch\n" % (
            int(self.trimmed.sum()), int(self.discarded.sum()), int(self.trimmed.sum()), int(self.bases.sum()))
        for i in range(self.bases.size):
            if self.bases[i] > 0:
                s += "\t%d\t%d\t%d\t%s\n" % (int(self.discarded[i]), int(self.trimmed[i]), int(self.bases[i]), filter_name(flt, i).decode())
        return s

    def file_bytes(self, row, j):
        return b"".join(b for _, b in self.records[row][j])

    def files(self, output="", prefixes=None):
        """OfstreamMap(out, suffix) with key "-" + prefix; a file nothing was written to does not exist"""
        n_inputs = len(self.records[0])
        prefixes = prefixes if prefixes is not None else ["transformed-%d" % (j + 1) for j in range(n_inputs)]
        return [("%s-%s%s" % (output, prefixes[j], ROWS[row]), self.file_bytes(row, j)) for row in range(2) for j in range(n_inputs) if self.records[row][j]]

    def read_segment(self, n):
        seg = np.full(n, -1, dtype=np.int32)
        n_inputs = len(self.records[0])
        for row in range(2):
            for j in range(n_inputs):
                for r, _ in self.records[row][j]:
                    seg[r] = row * n_inputs + j
        return seg


def report(flt, res, names, seqs, quals, pairs=None, input_starts=None, artifact_output=True, phix_output=True, in_base=33, out_base=33, print_bases=False,
           variant=None):
    """flt: the refartifact.Filter; res: what its apply() returned for (seqs, quals) with the mate that follows from `pairs`;
    pairs: list of (read1, read2), -1 for an absent side, or None for every read on its own"""
    n = len(seqs)
    n_inputs = 1 if input_starts is None else len(input_starts) - 1
    rep = Report(flt.n_seq, n_inputs)
    units = [(i, -1) for i in range(n)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    phix = flt.cfg.phix_idx

    def discard(v, r, row, label, first):
        rep.discarded[v] += 1
        rep.bases[v] += len(seqs[r])
        if row is not None:
            j = input_of(input_starts, r if variant == "file_of_own_read" else first)
            rep.records[row][j].append((r, record(names[r], seqs[r], quals[r], label, in_base, out_base, print_bases, variant)))

    for a, b in units:
        present = [r for r in (a, b) if r >= 0]
        v = {r: int(res["value"][r]) for r in present}
        if not any(v.values()):
            continue
        first = a if a >= 0 else b
        if phix != 0 and phix in v.values():
            for r in present:
                if variant == "phix_affected_only" and v[r] == 0:
                    continue
                discard(phix, r, 1 if phix_output else None, filter_name(flt, phix) if variant == "phix_labelled" else b"", first)
            continue
        any_discard = any(v[r] != 0 and res["action"][r] == 2 for r in present)
        for r in present:
            if v[r] == 0:
                if variant == "mate_labelled" and any_discard and artifact_output:
                    other = [x for x in present if x != r][0]
                    j = input_of(input_starts, first)
                    rep.records[0][j].append((r, record(names[r], seqs[r], quals[r], filter_name(flt, v[other]), in_base, out_base, print_bases, variant)))
                continue
            act = int(res["action"][r])
            if act == 2:
                discard(v[r], r, 0 if artifact_output else None, filter_name(flt, v[r]), first)
            elif act == 1:
                rep.trimmed[v[r]] += 1
                kept = int(res["max_pass"][r]) - int(res["min_pass"][r])
                rep.bases[v[r]] += len(seqs[r]) if variant == "trim_counts_len" else len(seqs[r]) - kept
    if variant == "read_index_order":
        for row in rep.records:
            for recs in row:
                recs.sort(key=lambda t: t[0])
    return rep
