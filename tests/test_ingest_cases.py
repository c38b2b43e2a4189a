"""The generator of the ingest tests (tests/ingestcases.py) held to the oracle's parser on the CPU: the oracle accepts every text
and finds the number of reads the generator states, and every quality-base case ends on the input base its table row states -- so
the device comparison of tests/test_gpu_ingest_device_text.py cannot pass on texts the oracle rejects, and no boundary case sits
on the wrong side of its boundary."""
import numpy as np
import pytest

import ingestcases as ic
from helpers import oracle_parse_fastq


def test_base_text_is_what_the_device_tests_need():
    text = ic.base_text()
    assert 2 * ic.BLOCK + 512 < len(text) < 10 * 1024          # a little over two blocks: line starts in three of them
    for sc in (True, False):
        rb, base = oracle_parse_fastq(text, 33, 33, sc)
        assert rb.n == ic.base_reads(sc) and base == 33
        lens = np.diff(rb.offsets.astype(np.int64))
        assert lens.min() == 1 and lens.max() == 1000
        long_reads = lens >= 255                                # more than 63 output dwords: ingest_copy's lane loop goes round again
        assert {int(o) & 3 for o in rb.offsets[:-1][long_reads]} == {0, 1, 2, 3}
        assert {int(o) & 3 for o in rb.offsets[:-1]} == {0, 1, 2, 3}
    assert ic.base_reads(True) < ic.base_reads(False) == len(ic.base_records())
    names = oracle_parse_fastq(text, 33, 33, False)[0].names
    for form in (b" 1:N:0:ACGT", b" 2:Y:0:ACGT", b"/1 1:Y:0:ACGT", b"\tsome comment"):
        assert any(n.endswith(form) for n in names), form
    assert b"\n+b0 " in text and b"\n+\n" in text             # '+name' and bare '+' lines
    quals = [text.split(b"\n")[4 * i + 3] for i in range(len(names))]
    assert any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
    bases = b"".join(text.split(b"\n")[4 * i + 1] for i in range(len(names)))
    assert b"N" in bases and b"n" in bases and b"a" in bases and b"A" in bases


@pytest.mark.parametrize("tail", sorted(ic.TAILS))
@pytest.mark.parametrize("lead", range(ic.CHUNK))
def test_oracle_accepts_every_framing(lead, tail):
    text = ic.framed(ic.base_text(), lead, tail)
    assert text[:lead] == b"\n" * lead and text[lead:lead + 1] == b"@"
    plain, _ = oracle_parse_fastq(ic.base_text(), 33, 33, True)
    rb, base = oracle_parse_fastq(text, 33, 33, True)
    assert rb.n == ic.base_reads(True) and base == 33
    assert np.array_equal(rb.bases, plain.bases) and np.array_equal(rb.quals, plain.quals) and rb.names == plain.names


def test_framing_moves_line_starts_through_every_chunk_position_and_over_the_block_borders():
    text = ic.base_text()
    starts = [0] + [i + 1 for i, c in enumerate(text[:-1]) if c == 10]
    for s in starts[::7]:
        assert {(s + lead) % ic.CHUNK for lead in range(ic.CHUNK)} == set(range(ic.CHUNK))
    # for each of the two borders some framing puts a line start on the block's first byte (its `prev` is the neighbour block's)
    for border in (ic.BLOCK, 2 * ic.BLOCK):
        assert any((s + lead) == border for s in starts for lead in range(ic.CHUNK)), border


def test_tail_cases():
    cases = ic.tail_cases()
    lengths = sorted({len(t) for _, t, _ in cases})
    assert lengths == [8] + sorted(ic.TAIL_LENGTHS)          # "short" is half a chunk
    assert {n % ic.CHUNK for n in ic.TAIL_LENGTHS} == {0, 1, 8, 15}
    assert {4095, 4096, 4097, 8192} <= set(ic.TAIL_LENGTHS)
    for label, text, reads in cases:
        got = oracle_parse_fastq(text, 33, 33, True)
        assert got is not None, label
        assert got[0].n == reads and got[1] == 33, label
        assert text.endswith(b"\n") == label.endswith("nl"), label
        assert len(got[0].seq(reads - 1)) == (1 if label == "short" else 100), label


@pytest.mark.parametrize("case", ic.quality_cases(), ids=[c[0] for c in ic.quality_cases()])
def test_quality_cases_land_on_their_stated_side(case):
    label, text, start, inb, final = case
    got = oracle_parse_fastq(text, start, inb, True)
    assert got is not None, label
    rb, base = got
    assert rb.n == ic.quality_case_reads(label)
    assert base == final
    if label.startswith("window/"):
        # the out-of-range read is where the label says, counted in kept reads, and the only one
        bad = np.flatnonzero(rb.quals != rb.quals[0])
        assert bad.tolist() == [ic.WINDOW - 2 if label.endswith("/flip") or label.endswith("skipped-flip") else ic.WINDOW - 1]
        assert (text.count(b"@f 1:Y") == 6) == ("skipped" in label)
    if label.startswith("crlf/"):
        assert b"\r" in rb.bases.tobytes() and all(n.endswith(b"\r") for n in rb.names)


def test_device_quality_cases_hold_every_group():
    labels = [c[0] for c in ic.device_quality_cases()]
    assert sum(1 for l in labels if l.startswith("window/")) == 4
    assert {l.split("/")[0] for l in labels} == {c[0].split("/")[0] for c in ic.quality_cases()}


def test_twobit_reads_put_every_long_read_at_every_offset():
    seqs = ic.twobit_reads()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    for L in ic.TWOBIT_LENGTHS:
        assert {int(offs[i]) & 3 for i, s in enumerate(seqs) if len(s) == L and i % 2 == 1} == {0, 1, 2, 3}, L
    long_ones = [s for s in seqs if len(s) > 516]
    assert all(s[257:258] == b"N" and s[300:301] == b"." and s[515:516] == b"X" and s[258:259] == b"c" for s in long_ones) and long_ones
