"""FASTA and FASTA+QUAL ingest on the device (kmr_ingest_fasta, kmr_ingest_fasta_dev, ReadSet.from_fasta) against tests/reffasta.py,
byte for byte, on every text of tests/fastacases.py -- from host text and from device text at every alignment of both pointers,
[a x 'A'][text][32 x 'A'] as tests/test_gpu_ingest_device_text.py places it -- and the batch in the stages that take it: spectrum
build, reference subtraction, pairs, scoring and the selector's output."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import fastacases as fc
import reffasta as rf
from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK
from test_fasta_cases import fastq_as_fasta_qual, golden
from test_gpu_ingest_device_text import place, read_back

pytestmark = pytest.mark.gpu
CASES = fc.all_cases()
KMR_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def handles():
    return {s: ka.KmerSpectrum(ka.default_config(21, estimated_raw_kmers=1 << 16, device=0, fastq_start_char=s)) for s in (33, 64)}


@functools.lru_cache(maxsize=None)
def wanted(label):
    c = next(c for c in CASES if c["label"] == label)
    return rf.parse(c["text"], c["qual"], c["start"], c["store_comment"])


def same(got, want, what):
    assert got["n"] == want["n"], what
    assert got["filtered"] == want["filtered"], what
    assert got["base"] == want["base"], what
    assert got["offsets"].tolist() == want["offsets"], what
    assert got["bases"].tobytes() == want["bases"], what
    assert got["quals"].tobytes() == want["quals"], what
    assert got["names"] == want["names"], what


def call_host(sp, c, out):
    q = c["qual"]
    qbuf = None if q is None else C.create_string_buffer(q, len(q) + 1)
    return sp.lib.kmr_ingest_fasta(sp.h, c["text"] if c["text"] else None, len(c["text"]), qbuf, 0 if q is None else len(q), 1 if c["store_comment"] else 0, C.byref(out))


def call_dev(sp, c, a, aq, out):
    buf, ptr = place(c["text"], a)
    qbuf, qptr = (None, None) if c["qual"] is None else place(c["qual"], aq)
    rc = sp.lib.kmr_ingest_fasta_dev(sp.h, C.c_void_p(ptr), len(c["text"]), None if qptr is None else C.c_void_p(qptr), 0 if c["qual"] is None else len(c["qual"]),
                                     1 if c["store_comment"] else 0, C.byref(out))
    del buf, qbuf
    return rc


def alignments(c):
    """(a, aq): every alignment of the text, the qual text at an offset of its own ((5a + 3) mod 16 runs through all 16 as well)"""
    return [(a, (5 * a + 3) % 16) for a in range(16)]


@pytest.mark.parametrize("c", [c for c in CASES if not c["refused"]], ids=lambda c: c["label"])
def test_accepted_texts(handles, c):
    sp = handles[c["start"]]
    want = wanted(c["label"])
    out = C.c_void_p()
    assert call_host(sp, c, out) == 0, sp.lib.kmr_last_error(sp.h)
    same(read_back(sp, out, c["text"]), want, "host text")
    for a, aq in alignments(c):
        out = C.c_void_p()
        assert call_dev(sp, c, a, aq, out) == 0, (a, aq, sp.lib.kmr_last_error(sp.h))
        same(read_back(sp, out, c["text"]), want, ("device text", a, aq))


@pytest.mark.parametrize("c", [c for c in CASES if c["refused"]], ids=lambda c: c["label"])
def test_refused_texts(handles, c):
    sp = handles[c["start"]]
    cause = c["refused"][0]
    out = C.c_void_p(1)
    assert call_host(sp, c, out) == KMR_ERR_INVALID_ARG and not out.value
    message = sp.lib.kmr_last_error(sp.h).decode()
    assert cause in message and message.startswith("malformed "), message
    for a, aq in alignments(c):
        out = C.c_void_p(1)
        assert call_dev(sp, c, a, aq, out) == KMR_ERR_INVALID_ARG and not out.value, (a, aq)
        assert sp.lib.kmr_last_error(sp.h).decode() == message, (a, aq)


def test_argument_checks_and_the_python_mirror(handles):
    sp = handles[33]
    out = C.c_void_p(1)
    assert sp.lib.kmr_ingest_fasta_dev(sp.h, None, 10, None, 0, 1, C.byref(out)) == KMR_ERR_INVALID_ARG and not out.value
    assert sp.lib.kmr_ingest_fasta(sp.h, b">a\nAC\n", 6, None, 5, 1, C.byref(out)) == KMR_ERR_INVALID_ARG and not out.value
    rs = ka.ReadSet.from_fasta(sp, b"")
    assert (rs.n, rs.total_bases, rs.filtered, rs.input_quality_base) == (0, 0, 0, 33)
    rs.close()
    with pytest.raises(ka.KmerSpectrumError, match="records for the"):
        ka.ReadSet.from_fasta(sp, b">a\nAC\n", b"")
    with pytest.raises(ka.KmerSpectrumError, match="a header followed by a header"):
        ka.ReadSet.from_fasta(sp, b">a\n>b\nAC\n")
    fasta, qual = golden("10.fasta"), golden("10.qual")
    rs = ka.ReadSet.from_fasta(sp, fasta, qual)
    b, q, o, names = rs.arrays()
    want = rf.parse(fasta, qual)
    assert rs.text == fasta and names == want["names"] and b.tobytes() == want["bases"] and q.tobytes() == want["quals"] and o.tolist() == want["offsets"]
    pairs = rs.identifyPairs()
    assert pairs.getPairSize() == 5 and rs.n == 10          # testFastaWithQualFile: getSize() / 2 == getPairSize()
    pairs.close()
    rs.close()


def _spectrum(k, fill, reference=None):
    sp = ka.KmerSpectrum(ka.default_config(k, estimated_raw_kmers=1 << 17, device=0))
    if reference is not None:
        sp.subtractReference(reference)
    fill(sp)
    sp.finalize(1)
    return sp


def _phix():
    text = golden("phix.fa")
    seq = b"".join(text.split(b"\n")[1:]).upper()
    assert text.count(b"\n") > 50 and len(seq) == 5386
    return text, np.frombuffer(seq, dtype=np.uint8), np.array([0, len(seq)], dtype=np.uint64)


@pytest.mark.parametrize("k", [21, 51])
def test_spectrum_of_a_genome_from_fasta(k):
    """a multi-line record of 5386 bases, every quality Read::REF_QUAL, against the same sequence handed over with quals=None"""
    text, bases, offsets = _phix()

    def from_fasta(sp):
        rs = ka.ReadSet.from_fasta(sp, text)
        assert (rs.n, rs.total_bases) == (1, 5386)
        sp.buildKmerSpectrumFromReadSet(rs)
        rs.close()
    a = _spectrum(k, from_fasta)
    b = _spectrum(k, lambda sp: sp.buildKmerSpectrum(bases, None, offsets))
    assert a.stats() == b.stats() and a.stats()["raw_kmers"] == 5386 - k + 1
    for which in (KMR_MAP_WEAK, KMR_MAP_SINGLETON):
        assert a.digest(which) == b.digest(which)
        assert np.array_equal(a.image(which), b.image(which))


def test_subtracting_a_reference_from_fasta():
    text, bases, offsets = _phix()
    fastq = golden("1000.std.fastq")

    def from_fasta(sp):
        rs = ka.ReadSet.from_fasta(sp, text)
        sp.buildKmerSpectrumFromReadSet(rs)
        rs.close()
    ref_a = _spectrum(21, from_fasta)
    ref_b = _spectrum(21, lambda sp: sp.buildKmerSpectrum(bases, None, offsets))

    def reads(sp):
        rs = ka.ReadSet(sp, fastq)
        sp.buildKmerSpectrumFromReadSet(rs)
        rs.close()
    a, b = _spectrum(21, reads, ref_a), _spectrum(21, reads, ref_b)
    assert a.getSubtracted() == b.getSubtracted() and a.getSubtracted() > 0
    assert a.stats() == b.stats()
    for which in (KMR_MAP_WEAK, KMR_MAP_SINGLETON):
        assert a.digest(which) == b.digest(which)


@pytest.fixture(scope="module")
def fastq_and_twin():
    """1000.std.fastq ingested as FASTQ and as FASTA + QUAL (sequence in 60-column lines, 25 numbers a line), on one handle"""
    sp = ka.KmerSpectrum(ka.default_config(21, estimated_raw_kmers=1 << 17, device=0))
    fastq = golden("1000.std.fastq")
    fasta, qual = fastq_as_fasta_qual(fastq, 33, 60, 25)
    return sp, ka.ReadSet(sp, fastq), ka.ReadSet.from_fasta(sp, fasta, qual)


def test_fasta_qual_twin_of_a_fastq(fastq_and_twin):
    sp, rq, rf_ = fastq_and_twin
    bq, qq, oq, nq = rq.arrays()
    bf, qf, of, nf = rf_.arrays()
    assert rq.n == rf_.n == 1000 and rq.input_quality_base == rf_.input_quality_base == 33
    assert np.array_equal(bq, bf) and np.array_equal(qq, qf) and np.array_equal(oq, of) and nq == nf
    digests = []
    for rs in (rq, rf_):
        s = _spectrum(21, lambda x: x.buildKmerSpectrumFromReadSet(rs))
        digests.append((s.stats(), s.digest(KMR_MAP_WEAK), s.digest(KMR_MAP_SINGLETON)))
    assert digests[0] == digests[1]
    pq, pf = rq.identifyPairs(), rf_.identifyPairs()
    assert np.array_equal(pq.mate, pf.mate) and pq.getPairSize() == pf.getPairSize() > 0
    pq.close(); pf.close()


def test_selector_output_of_fasta_reads(fastq_and_twin):
    """reads from plain FASTA (every quality 127) scored against the spectrum of the FASTQ and written as FASTA: the text of the
    FASTQ-ingested batch.  Scoring reads bases only, and the FASTA writer prints no qualities."""
    sp, rq, _ = fastq_and_twin
    fasta, _ = fastq_as_fasta_qual(golden("1000.std.fastq"), 33, 60, 25)
    spec = _spectrum(21, lambda x: x.buildKmerSpectrumFromReadSet(rq))
    rq2, rp2 = ka.ReadSet(spec, golden("1000.std.fastq")), ka.ReadSet.from_fasta(spec, fasta)
    want = ka.ReadSelector(spec, rq2).filterReads(format="fasta")
    got = ka.ReadSelector(spec, rp2).filterReads(format="fasta")
    assert len(want) > 10000 and got == want
    rq2.close(); rp2.close()
