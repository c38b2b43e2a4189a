"""The texts of tests/fastacases.py against tests/reffasta.py, on the CPU: every accepted text is one the reference's stream form and
its mmap form read alike and without mangling, every refused text is one they read differently, throw on or mangle (asserted which);
the reference's own FASTA fixtures re-print byte for byte; and the restatement agrees with the oracle's FASTQ parser on 1000.std.fastq
rewritten as FASTA + QUAL."""
import os

import numpy as np
import pytest

import fastacases as fc
import reffasta as rf
from helpers import oracle_parse_fastq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = fc.all_cases()


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def fastq_as_fasta_qual(text, start=33, width=None, qual_width=None):
    """a four-line FASTQ text as a FASTA and a QUAL text (sequence in lines of `width`, numbers in lines of `qual_width`)"""
    lines = bytes(text).split(b"\n")
    fasta, qual = [], []
    for i in range(0, len(lines) - 3, 4):
        head = b">" + lines[i][1:] + b"\n"
        fasta.append(head + (fc.wrap(lines[i + 1], width) if width else lines[i + 1] + b"\n"))
        qual.append(head + fc.qual_lines([c - start for c in lines[i + 3]], qual_width))
    return b"".join(fasta), b"".join(qual)


def outcomes(c):
    kw = {"start": c["start"], "store_comment": c["store_comment"]}
    return rf.outcome(rf.parse_stream, c["text"], c["qual"], **kw), rf.outcome(rf.parse_mmap, c["text"], c["qual"], **kw)


def test_labels_are_unique_and_every_rule_has_a_refused_text():
    labels = [c["label"] for c in CASES]
    assert len(set(labels)) == len(labels)
    causes = {c["refused"][0] for c in CASES if c["refused"]}
    assert len(causes) == 10


@pytest.mark.parametrize("c", [c for c in CASES if not c["refused"]], ids=lambda c: c["label"])
def test_accepted_texts_read_alike_in_both_forms(c):
    assert rf.accepted(c["text"], c["qual"], c["store_comment"])
    s, m = outcomes(c)
    assert s[0] == "ok" and s == m
    assert not rf.parse_stream(c["text"], c["qual"], c["start"], c["store_comment"])["mangled"]


@pytest.mark.parametrize("c", [c for c in CASES if c["refused"]], ids=lambda c: c["label"])
def test_refused_texts_differ_throw_or_mangle(c):
    cause, kind = c["refused"]
    assert rf.refusal(c["text"], c["qual"], c["store_comment"]) == cause
    s, m = outcomes(c)
    if kind == "differ":
        assert s != m
    elif kind == "throws":
        assert s[0] == "throws" and m[0] == "throws"
    else:
        assert kind == "mangles" and s[0] == "ok" and s == m
        assert rf.parse_stream(c["text"], c["qual"], c["start"], c["store_comment"])["mangled"]


def test_what_the_cases_cover():
    by = {c["label"]: c for c in CASES}
    p = rf.parse(by["long/60-columns"]["text"])
    assert p["n"] == 1 and len(p["bases"]) == 20000 and p["bases"] == rf.parse(by["long/one-line"]["text"])["bases"]
    assert set(p["quals"]) == {rf.REF_QUAL} and p["base"] == 33
    # the Casava filter drops with comments stored what it keeps without them ("name 1:Y" -> "name/1": pos moves on)
    assert rf.parse(by["casava/stored"]["text"], store_comment=True)["filtered"] == 3          # r2, r5 and r8 (a tab separates as a blank does)
    assert rf.parse(by["casava/not-stored"]["text"], store_comment=False)["filtered"] == 0
    assert rf.parse(by["casava/all-dropped"]["text"])["n"] == 0
    # the clamp: 93 and everything above it is one below Read::REF_QUAL
    v = rf.parse(by["values/33"]["text"], by["values/33"]["qual"], 33)
    assert list(v["quals"][:6]) == [33, 73, 74, 126, 126, 126] and v["base"] == 33
    v = rf.parse(by["values/64"]["text"], by["values/64"]["qual"], 64)
    assert list(v["quals"][:6]) == [64, 104, 105, 126, 126, 126] and v["base"] == 64
    # the quality-base flip happens for reads 0 and 19 998, not for read 19 999
    for start, other in ((33, 64), (64, 33)):
        for bad, final in ((0, other), (fc.WINDOW - 2, other), (fc.WINDOW - 1, start)):
            c = by["window/%d/%d" % (start, bad)]
            r = rf.parse(c["text"], c["qual"], start)
            assert r["n"] == fc.WINDOW + 1 and r["base"] == final
            assert r["quals"][1] == 30 + start + (start - other if final == other else 0)
    assert rf.parse(by["flip/long-read-one-low"]["text"], by["flip/long-read-one-low"]["qual"])["base"] == 33
    assert rf.parse(by["flip/second-read-all-high"]["text"], by["flip/second-read-all-high"]["qual"])["base"] == 64


def test_the_reference_fixtures_are_accepted_and_reprint():
    """testFastaWithQualFile (test/ReadSetTest.cpp:141-166): names, bases and formatted qualities give the files back"""
    fasta, qual, fa5 = golden("10.fasta"), golden("10.qual"), golden("5.fa")
    assert (len(fasta), len(qual), len(fa5)) == (923, 2044, 500)
    assert rf.accepted(fasta, qual) and rf.accepted(fa5)
    for form in (rf.parse_stream, rf.parse_mmap):
        assert rf.outcome(form, fasta, qual) == rf.outcome(rf.parse_stream, fasta, qual)
    p = rf.parse(fasta, qual)
    assert p["n"] == 10 and p["base"] == 33
    assert rf.reprint(p) == (fasta, qual)
    p5 = rf.parse(fa5)
    assert p5["n"] == 5 and rf.reprint(p5)[0] == fa5 and set(p5["quals"]) == {rf.REF_QUAL}


@pytest.mark.parametrize("width,qual_width", [(None, None), (60, 25)])
def test_restatement_agrees_with_the_oracle_on_a_fastq_rewritten(width, qual_width):
    text = golden("1000.std.fastq")
    want, base = oracle_parse_fastq(text, 33, 33, True)
    fasta, qual = fastq_as_fasta_qual(text, 33, width, qual_width)
    assert rf.accepted(fasta, qual)
    got = rf.parse(fasta, qual, 33, True)
    assert got["n"] == want.n == 1000 and got["base"] == base and got["filtered"] == 0
    assert got["names"] == want.names
    assert np.array_equal(np.array(got["offsets"], dtype=np.uint64), want.offsets)
    assert got["bases"] == want.bases.tobytes() and got["quals"] == want.quals.tobytes()


def test_library_exports_the_fasta_ingest():
    import kmernator_amd as ka
    lib = ka.load()
    assert lib.kmr_ingest_fasta and lib.kmr_ingest_fasta_dev
    assert {"kmr_ingest_fasta", "kmr_ingest_fasta_dev"} <= set(ka._lib.EXPORTS)
