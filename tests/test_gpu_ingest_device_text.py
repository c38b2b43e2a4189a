"""FASTQ ingest and pair identification from text the caller holds on the device (kmr_ingest_fastq_dev, kmr_identify_pairs_dev), at
every alignment of the pointer, every position of a line start inside a 16-byte chunk and a 4 KB block and every kind of end, and
the two-bit forms of reads longer than one round of the unpack kernel's lanes -- against the oracle's parser, tests/refpairs.py and
orc_compress_sequence, byte for byte.

The text lies inside a larger device buffer, [a bytes of 'A'][text][32 bytes of 'A'], and the call gets the address of its first
byte and its length: a read of text[-1] or of anything at or behind the end meets a byte that is no newline, which moves a line
start or the last line's end and shows in the result.  kmr_ingest_fastq gives the kernels a fresh 256-byte aligned copy with slack
behind it, so only this file runs the byte-wise side of the alignment switches of kmr_ingest.hpp and kmr_pairs.hpp (DESIGN.md,
"Ingest from device text")."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import ingestcases as ic
import refpairs
from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, OracleSpectrum, ReadBatch, default_config, oracle_lib, oracle_parse_fastq
from test_gpu_identify_pairs import check as check_pairs

pytestmark = pytest.mark.gpu
POISON_BEHIND = 32


@pytest.fixture(scope="module")
def sp33():
    return ka.KmerSpectrum(ka.default_config(21, estimated_raw_kmers=1 << 16, device=0))


@pytest.fixture(scope="module")
def sp64():
    return ka.KmerSpectrum(ka.default_config(21, estimated_raw_kmers=1 << 16, device=0, fastq_start_char=64))


def place(text, a):
    """(tensor that owns the bytes, address of the text's first byte): [a x 'A'][text][32 x 'A'] on the device"""
    import torch
    buf = torch.frombuffer(bytearray(b"A" * a + bytes(text) + b"A" * POISON_BEHIND), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + a


def read_back(sp, r, text):
    """what a kmr_reads holds, as ReadSet.arrays() reads it, and the batch given back"""
    n, tot, qb, nf = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    assert sp.lib.kmr_reads_info(r, C.byref(n), C.byref(tot), C.byref(qb), C.byref(nf)) == 0
    b = np.zeros(tot.value, dtype=np.uint8)
    q = np.zeros(tot.value, dtype=np.uint8)
    o = np.zeros(n.value + 1, dtype=np.uint64)
    no = np.zeros(max(1, n.value), dtype=np.uint64)
    nl = np.zeros(max(1, n.value), dtype=np.uint32)
    u64p = C.POINTER(C.c_uint64)
    rc = sp.lib.kmr_reads_copy(r, b.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), o.ctypes.data_as(u64p), no.ctypes.data_as(u64p),
                               nl.ctypes.data_as(C.POINTER(C.c_uint32)))
    sp.lib.kmr_reads_free(r)
    assert rc == 0
    names = [text[int(no[i]):int(no[i]) + int(nl[i])] for i in range(n.value)]
    return {"n": n.value, "filtered": nf.value, "base": qb.value, "bases": b, "quals": q, "offsets": o, "names": names}


def ingest_dev(sp, text, a, input_base=0, store_comment=True):
    buf, ptr = place(text, a)
    r = C.c_void_p()
    sp._call("ingest_fastq_dev", sp.h, C.c_void_p(ptr), len(text), input_base, 1 if store_comment else 0, C.byref(r))
    del buf
    return read_back(sp, r, text)


def ingest_host(sp, text, input_base=0, store_comment=True):
    rs = ka.ReadSet(sp, text, input_base, store_comment)
    b, q, o, names = rs.arrays()
    return {"n": rs.n, "filtered": rs.filtered, "base": rs.input_quality_base, "bases": b, "quals": q, "offsets": o, "names": names}


def same(got, want, records, what):
    rb, base = want
    assert got["n"] == rb.n, what
    assert got["filtered"] == records - rb.n, what
    assert got["base"] == base, what
    assert np.array_equal(got["offsets"], rb.offsets), what
    assert np.array_equal(got["bases"], rb.bases), what
    assert np.array_equal(got["quals"], rb.quals), what
    assert got["names"] == rb.names, what


@functools.lru_cache(maxsize=None)
def framed_case(lead, tail, store_comment):
    text = ic.framed(ic.base_text(), lead, tail)
    return text, oracle_parse_fastq(text, 33, 33, store_comment)


N_BASE = len(ic.base_records())


@pytest.mark.parametrize("a", range(16))
def test_every_pointer_alignment(sp33, a):
    """a = 0: the 16-byte chunk load, the 8-byte line-end words and the dword pairs of ingest_copy; a = 4, 8, 12: bytes for the first two,
    dwords for the copy; every other a: bytes throughout"""
    for lead in (0, 1, 15):
        for tail in sorted(ic.TAILS):
            text, want = framed_case(lead, tail, True)
            same(ingest_dev(sp33, text, a), want, N_BASE, (a, lead, tail))


@pytest.mark.parametrize("lead", range(16))
def test_every_line_start_position(sp33, lead):
    """every line start at every position of its chunk, and the records at the block borders in front of, on and behind them"""
    for a, store_comment, tail in ((0, True, "one"), (1, False, "none"), (4, False, "three"), (8, True, "none")):
        text, want = framed_case(lead, tail, store_comment)
        same(ingest_dev(sp33, text, a, store_comment=store_comment), want, N_BASE, (a, lead, tail))


@pytest.mark.parametrize("case", ic.tail_cases(), ids=[c[0] for c in ic.tail_cases()])
def test_tails_at_chunk_and_block_borders(sp33, case):
    """texts that end on, one short of and one past a chunk and a block border, in a newline or in the last quality character: the last
    thread's chunk is whole, or partial and read byte by byte, and the last line is read to its end in words or bytes"""
    label, text, reads = case
    want = oracle_parse_fastq(text, 33, 33, True)
    assert want[0].n == reads
    records = text.count(b"\n@b") + 1 + (0 if label == "short" else 1)
    for a in (0, 3, 8):
        same(ingest_dev(sp33, text, a), want, records, (label, a))


QUALITY_ON_DEVICE = {c[0] for c in ic.device_quality_cases()}


@pytest.mark.parametrize("case", ic.quality_cases(), ids=[c[0] for c in ic.quality_cases()])
def test_quality_base_detection_limits(sp33, sp64, case):
    label, text, start, inb, final = case
    sp = sp33 if start == 33 else sp64
    want = oracle_parse_fastq(text, start, inb, True)
    assert want[1] == final and want[0].n == ic.quality_case_reads(label)
    records = text.count(b"\n+")
    same(ingest_host(sp, text, inb), want, records, label)
    if label in QUALITY_ON_DEVICE:
        same(ingest_dev(sp, text, 5, inb), want, records, label + " from device text")


def test_device_form_argument_checks(sp33):
    sp = sp33
    r = C.c_void_p()
    assert sp.lib.kmr_ingest_fastq_dev(sp.h, None, 10, 33, 1, C.byref(r)) == -1 and not r.value          # KMR_ERR_INVALID_ARG
    assert sp.lib.kmr_ingest_fastq_dev(sp.h, None, 0, 33, 1, C.byref(r)) == 0
    got = read_back(sp, r, b"")
    assert (got["n"], got["filtered"], got["base"], got["offsets"].tolist()) == (0, 0, 33, [0])
    buf, ptr = place(b"@r\nACGT\n+\nIIII\n", 3)
    r = C.c_void_p()
    assert sp.lib.kmr_ingest_fastq_dev(sp.h, C.c_void_p(ptr), 0, 33, 1, C.byref(r)) == 0                # a pointer and no bytes
    assert read_back(sp, r, b"")["n"] == 0
    bad = b"@r\nACGT\n+\nIII\n"
    assert oracle_parse_fastq(bad, 33, 33) is None
    buf, ptr = place(bad, 3)
    r = C.c_void_p()
    assert sp.lib.kmr_ingest_fastq_dev(sp.h, C.c_void_p(ptr), len(bad), 33, 1, C.byref(r)) == -1 and not r.value
    dev_error = sp.lib.kmr_last_error(sp.h).decode()
    with pytest.raises(ka.KmerSpectrumError) as host_error:
        ka.ReadSet(sp, bad)
    assert "malformed FASTQ" in dev_error and dev_error in str(host_error.value)


@pytest.mark.parametrize("store_comment", [False, True])
@pytest.mark.parametrize("seed", [1, 4])
def test_pairs_on_unaligned_device_text(sp33, seed, store_comment):
    """pairs_parse_kernel reads the names through PairsBytes: dwords at a = 0, bytes at a = 1, 2, 3"""
    lines = refpairs.generate(seed)
    want = refpairs.identify_pairs(lines, 1 if store_comment else 0)
    rs = ka.ReadSet(sp33, refpairs.fastq_text(lines), store_comment=store_comment)
    assert rs.n == len(lines)
    host = rs.identifyPairs()
    check_pairs(host, want, "host text")
    for a in range(4):
        buf, ptr = place(rs.text, a)
        dev = rs.identifyPairs(device_text=ptr)
        check_pairs(dev, want, a)
        assert np.array_equal(dev.mate, host.mate) and np.array_equal(dev.pairs, host.pairs), a
        dev.close()
        del buf
    host.close()
    rs.close()


def test_twobit_round_trip_of_long_reads():
    """reads of more than 259 bases (more aligned output dwords than the unpack kernel has lanes) at every offset mod 4, with markups
    beyond position 256: packed against orc_compress_sequence, unpacked against the text, and built into a spectrum against the text's"""
    seqs = ic.twobit_reads()
    rb = ReadBatch(seqs, [b"I" * len(s) for s in seqs])
    cfg = default_config(31, estimated_raw_kmers=1 << 16)
    sp = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1 << 16, device=0))
    rs = ka.ReadSet.from_arrays(sp, rb.bases, rb.quals, rb.offsets)
    tw, to, mp, mc, mo = rs.twobit()
    rs.close()
    # 1: the packed form and the markups are compressSequence's
    lib = oracle_lib()
    assert int(to[-1]) == tw.size == sum((len(s) + 3) // 4 for s in seqs)
    unpacked = []
    for i, s in enumerate(seqs):
        nb = (len(s) + 3) // 4
        out = np.zeros(nb + 1, dtype=np.uint8)
        pos = np.zeros(len(s) + 1, dtype=np.uint32)
        ch = C.create_string_buffer(len(s) + 1)
        nm = lib.orc_compress_sequence(s, len(s), out.ctypes.data_as(C.POINTER(C.c_uint8)), pos.ctypes.data_as(C.POINTER(C.c_uint32)), ch, len(s) + 1)
        assert int(to[i + 1] - to[i]) == nb, i
        assert np.array_equal(tw[int(to[i]):int(to[i + 1])], out[:nb]), i
        assert int(mo[i + 1] - mo[i]) == nm, i
        assert np.array_equal(mp[int(mo[i]):int(mo[i + 1])], pos[:nm]), i
        assert mc[int(mo[i]):int(mo[i + 1])].tobytes() == ch.raw[:nm], i
        # the text these say, in plain numpy: two bits per base, first base in bits 7-6, then the markups
        codes = (out[:nb, None] >> np.array([6, 4, 2, 0], dtype=np.uint8)) & 3
        t = np.frombuffer(b"ACGT", dtype=np.uint8)[codes.reshape(-1)[:len(s)]].copy()
        t[pos[:nm]] = np.frombuffer(ch.raw[:nm], dtype=np.uint8)
        assert t.tobytes() == s.upper().replace(b".", b"N"), i          # the alphabet has no lower case but acgt
        unpacked.append(t.tobytes())
    assert int(mo[-1]) > 100 and any(int(p) > 256 for p in mp)
    # 2: and back
    back = ka.ReadSet.from_twobit(sp, tw, to, rb.offsets, quals=rb.quals, markups=(mp, mc, mo))
    b, q, o, _ = back.arrays()
    back.close()
    assert np.array_equal(o, rb.offsets) and np.array_equal(q, rb.quals)
    for i, s in enumerate(unpacked):
        assert b[int(o[i]):int(o[i + 1])].tobytes() == s, (i, len(s), int(o[i]) & 3)
    # 3: the spectrum of the packed reads is the spectrum of the text
    # (every read twice, so that its k-mers are no singletons and the weak map holds them)
    orc = OracleSpectrum(cfg)
    st = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1 << 16, device=0))
    for first in (0, rb.n):
        orc.add_reads(rb, first)
        sp.buildKmerSpectrumTwoBit(tw, to, rb.offsets, quals=rb.quals, markups=(mp, mc, mo), first_read_idx=first)
        st.buildKmerSpectrum(rb.bases, rb.quals, rb.offsets, first_read_idx=first)
    for x in (orc, sp, st):
        x.finalize(1)
    assert sp.stats() == st.stats() == orc.stats()
    for which in (KMR_MAP_WEAK, KMR_MAP_SINGLETON):
        assert np.array_equal(sp.image(which), st.image(which))
    nb = orc.num_buckets(KMR_MAP_WEAK)
    assert np.array_equal(sp.image(KMR_MAP_WEAK)[:16 + 8 * nb], orc.image(KMR_MAP_WEAK)[:16 + 8 * nb])
    keys, cnt, _, _, _ = orc.entries()
    assert keys.shape[0] > 5000 and np.array_equal(sp.getCount(keys), cnt)
