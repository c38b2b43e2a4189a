"""Pair identification on the device (kmr_identify_pairs*, kmr_pairs.hpp) against the sequential restatement of
ReadSet::identifyPairs in tests/refpairs.py: mate, the pair list in the reference's order and every count, exactly."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import kmernator_amd as ka
from helpers import GOLDEN
import refpairs

pytestmark = pytest.mark.gpu
K = 31


def spectrum():
    return ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 16, device=0))


def check(pairs, want, what=""):
    assert pairs.n_reads == want.n_reads, what
    assert np.array_equal(pairs.mate, want.mate_array()), what
    assert np.array_equal(pairs.pairs, want.pair_array()), what
    got = (pairs.n_pairs, pairs.n_full, pairs.n_sequential, pairs.n_conflicts, pairs.hasPairs())
    assert got == (want.n_pairs, want.n_full, want.n_sequential, want.n_conflicts, want.has_pairs()), what
    assert pairs.getPairSize() == want.n_pairs


def identify_both_ways(sp, lines, store_comment):
    """through the host-text and the device-text entry points"""
    import torch
    rs = ka.ReadSet(sp, refpairs.fastq_text(lines), store_comment=bool(store_comment))
    assert rs.n == len(lines)
    host = rs.identifyPairs()
    dtext = torch.frombuffer(bytearray(rs.text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    dev = rs.identifyPairs(device_text=dtext.data_ptr())
    return rs, host, dev


@pytest.mark.parametrize("case", refpairs.HAND_CASES, ids=[c[0] for c in refpairs.HAND_CASES])
def test_hand_worked_cases(case):
    label, lines, store_comment, mate, pairs = case
    sp = spectrum()
    rs, host, dev = identify_both_ways(sp, lines, store_comment)
    for got in (host, dev):
        assert got.mate.tolist() == mate, label
        assert [tuple(p) for p in got.pairs.tolist()] == pairs, label
        check(got, refpairs.identify_pairs(lines, store_comment), label)
        got.close()
    # and with the other setting of store_comment, against the restatement
    other = rs.identifyPairs(store_comment=not store_comment)
    check(other, refpairs.identify_pairs(lines, not store_comment), label)
    other.close()


@pytest.mark.parametrize("store_comment", [0, 1])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generated_batches(seed, store_comment):
    lines = refpairs.generate(seed)
    want = refpairs.identify_pairs(lines, store_comment)
    sp = spectrum()
    rs, host, dev = identify_both_ways(sp, lines, store_comment)
    check(host, want)
    check(dev, want)
    m, r1, r2 = host.device_ptrs()
    assert m and r1 and r2
    host.close(); dev.close()
    with pytest.raises(ka.KmerSpectrumError):
        host.device_ptrs()


def test_store_comment_defaults_to_the_ingest_s():
    lines = ["m 1:N:0:ACGT", "x", "m/2"]
    sp = spectrum()
    for sc in (0, 1):
        rs = ka.ReadSet(sp, refpairs.fastq_text(lines), store_comment=bool(sc))
        check(rs.identifyPairs(), refpairs.identify_pairs(lines, sc))
    assert refpairs.identify_pairs(lines, 0).mate == [2, -1, 0] and refpairs.identify_pairs(lines, 1).mate == [-1, -1, -1]


def test_empty_batch_and_batch_without_names():
    sp = spectrum()
    rs = ka.ReadSet(sp, b"")
    p = rs.identifyPairs()
    assert (p.n_reads, p.n_pairs, p.n_full, p.n_sequential, p.n_conflicts, p.hasPairs()) == (0, 0, 0, 0, 0, False)
    assert p.mate.size == 0 and p.pairs.shape == (0, 2)
    n = 1000
    bases = np.frombuffer(b"ACGT" * (n * 2), dtype=np.uint8)
    rs = ka.ReadSet.from_arrays(sp, bases, np.full(bases.size, 73, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64) * 8)
    p = rs.identifyPairs()
    assert (p.n_reads, p.n_pairs, p.n_full, p.n_sequential, p.n_conflicts, p.hasPairs()) == (n, n, 0, 0, 0, False)
    assert np.array_equal(p.mate, np.full(n, -1)) and np.array_equal(p.pairs[:, 0], np.arange(n)) and np.array_equal(p.pairs[:, 1], np.full(n, -1))


def test_name_span_outside_the_text_is_refused():
    sp = spectrum()
    rs = ka.ReadSet(sp, refpairs.fastq_text(["a/1", "a/2"]))
    out = C.c_void_p()
    short = np.frombuffer(rs.text[:10], dtype=np.uint8)
    rc = sp.lib.kmr_identify_pairs(sp.h, rs.r, short.ctypes.data_as(C.c_void_p), short.size, 1, C.byref(out))
    assert rc == -1 and not out.value
    assert b"name span" in sp.lib.kmr_last_error(sp.h)


def test_truncated_hash_changes_nothing():
    """kmr_tune pair_hash_bits down to a few bits: distinct common names share a sort key, and the byte-for-byte grouping inside a
    run of equal keys must give the 64-bit run's result"""
    lines = refpairs.generate(5, n_fragments=1500)
    want = refpairs.identify_pairs(lines, 0)
    sp = spectrum()
    rs = ka.ReadSet(sp, refpairs.fastq_text(lines), store_comment=False)
    full = rs.identifyPairs()
    assert sp.build_info("pair_hash_collisions") == 0
    check(full, want)
    for bits in (6, 3, 1):
        sp.tune(pair_hash_bits=bits)
        cut = rs.identifyPairs()
        collisions = sp.build_info("pair_hash_collisions")
        print("pair_hash_bits %d: %d runs of equal keys held more than one name" % (bits, collisions))
        assert collisions > 0
        assert collisions <= 2 ** bits
        assert np.array_equal(cut.mate, full.mate) and np.array_equal(cut.pairs, full.pairs)
        check(cut, want)
    sp.tune(pair_hash_bits=64)
    again = rs.identifyPairs()
    assert sp.build_info("pair_hash_collisions") == 0
    check(again, want)


def test_golden_1000_pairs_and_filtered_output():
    """tests/golden/1000.fastq is 500 adjacent /1 /2 pairs; the flow of the golden test of the selection (artifact filter, build,
    filterReads) with the mate the device found gives 1000-Filtered.fastq byte for byte"""
    g = lambda name: open(os.path.join(GOLDEN, name), "rb").read()
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, g("1000.fastq"))
    pairs = rs.identifyPairs()
    assert np.array_equal(pairs.mate, np.arange(1000, dtype=np.int64) ^ 1)
    assert (pairs.n_pairs, pairs.n_full, pairs.n_sequential, pairs.n_conflicts) == (500, 500, 500, 0)
    assert pairs.hasPairs() and pairs.getPairSize() == 500
    assert np.array_equal(pairs.pairs, np.arange(1000, dtype=np.int64).reshape(500, 2))
    f = ka.FilterKnownOddities(sp, g("artifact_sequences.fa"), edit_distance=1, min_read_length=25.0)
    res, frs = f.applyFilter(rs)
    sp.buildKmerSpectrumFromReadSet(frs)
    sp.finalize(2)
    sel = ka.ReadSelector(sp, frs, mate=pairs.mate, filter_results=res)
    text = sel.filterReads(2, 25.0, False, "MEDIAN", 64, "fastq")
    assert text.replace(b"\t", b" ") == g("1000-Filtered.fastq").replace(b"\t", b" ")


# ---- at scale -------------------------------------------------------------------------------------------------------------
# 2 000 000 reads: the restatement (a Python loop over strings and a dict) takes a few seconds per layout at this size
N_SCALE = 2_000_000


def scale_text(lines):
    """FASTQ text of 4-base reads with these name lines, built with numpy-free joins (the names are what matters)"""
    return ("\n".join("@%s\nACGT\n+\nIIII" % l for l in lines) + "\n").encode()


def scale_layout(layout):
    half = N_SCALE // 2
    if layout == "interleaved":
        return ["r%010d/%d" % (i >> 1, (i & 1) + 1) for i in range(N_SCALE)]
    if layout == "r1_then_r2":
        return ["r%010d/1" % i for i in range(half)] + ["r%010d/2" % i for i in range(half)]
    # a shuffled mix: pairs apart, singles, and a few thousand names that occur a second time
    rng = np.random.RandomState(77)
    lines = []
    for i in range(half - 4000):
        kind = i % 10
        if kind < 8:
            lines += ["s%09d/1" % i, "s%09d/2" % i]
        elif kind == 8:
            lines += ["s%09d" % i, "t%09d 1:N:0:ACGT" % i]
        else:
            lines += ["s%09d/A" % i, "s%09d/B" % i]
    for i in range(4000):
        lines += ["s%09d/%d" % (i * 10, 1 + (i & 1)), "s%09d/" % (i * 10 + 1)]
    assert len(lines) == N_SCALE
    perm = rng.permutation(N_SCALE)
    return [lines[j] for j in perm]


@pytest.mark.parametrize("layout", ["interleaved", "r1_then_r2", "shuffled"])
def test_at_scale(layout):
    lines = scale_layout(layout)
    t0 = time.perf_counter()
    want = refpairs.identify_pairs(lines, 1)
    t_ref = time.perf_counter() - t0
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 20, device=0))
    rs = ka.ReadSet(sp, scale_text(lines))
    assert rs.n == N_SCALE
    sp.tune(pairs_timing=1)
    pairs = rs.identifyPairs()
    print("%s: %d reads, %d pairs (%d sequential, %d full, %d conflicts); device %.2f ms (parse %.2f, sort %.2f), restatement %.1f s"
          % (layout, N_SCALE, pairs.n_pairs, pairs.n_sequential, pairs.n_full, pairs.n_conflicts, sp.build_info("pairs_ms"),
             sp.build_info("pairs_parse_ms"), sp.build_info("pairs_sort_ms"), t_ref))
    check(pairs, want, layout)
    half = N_SCALE // 2
    if layout == "r1_then_r2":
        assert np.array_equal(pairs.mate[:half], np.arange(half, dtype=np.int64) + half)
        assert np.array_equal(pairs.mate[half:], np.arange(half, dtype=np.int64))
        assert pairs.n_sequential == 0 and pairs.n_full == half
    elif layout == "interleaved":
        assert pairs.n_sequential == half and np.array_equal(pairs.mate, np.arange(N_SCALE, dtype=np.int64) ^ 1)
    else:
        assert pairs.n_conflicts > 0 and 0 < pairs.n_sequential < 100 and pairs.n_full > half // 2
    assert sp.build_info("pair_hash_collisions") == 0
