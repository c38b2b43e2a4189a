"""MeraculousCounter's mercount / mergraph text made on the device (kmr_dump_text*, kmernator_amd/csrc/kmr_dump.hpp) against the
oracle's file (OracleSpectrum.dump: the reference's dumpCounts / dumpGraphs, src/Meraculous.h:107-133) as WHOLE BYTES, in the
reference's iteration order -- not as sorted lines, unless a test says so."""
import ctypes as C
import os

import numpy as np
import pytest

import kmernator_amd as ka
from helpers import GOLDEN, KMR_MAP_WEAK, KMR_VALUE_EXT, OracleSpectrum, default_config, read_fastq, synth_reads

pytestmark = pytest.mark.gpu

MERA = dict(min_weight=0.0, min_quality_score=2)          # MeraculousCounter's settings
ERR_STATE = "KMR_ERR_STATE"


def product(cfg, mode=0, **tune):
    c = ka.default_config(cfg.k)
    for name, _ in cfg._fields_:
        setattr(c, name, getattr(cfg, name))
    c.build_mode = mode
    c.device = 0
    return ka.KmerSpectrum(c).tune(**tune)


def both(cfg, rb, min_depth=2, mode=0, **tune):
    o, p = OracleSpectrum(cfg), product(cfg, mode, **tune)
    o.add_reads(rb)
    p.buildKmerSpectrum(rb.bases, rb.quals, rb.offsets, 0, rb.discarded)
    o.finalize(min_depth)
    p.finalize(min_depth)
    assert o.stats() == p.stats()
    return o, p


def oracle_text(o, tmp_path, min_depth, graph):
    path = str(tmp_path / ("oracle.%s.%d" % ("g" if graph else "c", min_depth)))
    if os.path.exists(path):
        os.remove(path)
    o.dump(path, min_depth, graph)
    return open(path, "rb").read()


def device_text(p, min_depth, graph, lo=0, hi=None):
    """the text through kmr_dump_text, with kmr_dump_text_size == kmr_text_info == the real length checked on the way"""
    kind = "mergraph" if graph else "mercount"
    kept, nbytes = p.dumpTextSize(kind, min_depth, lo, hi)
    with (p.dumpGraphsText if graph else p.dumpCountsText)(min_depth, lo, hi) as t:
        assert (t.kept, t.bytes) == (kept, nbytes)
        text = t.numpy().tobytes()
    assert len(text) == nbytes
    return text, kept


def live(p):
    return int(p.build_info("device_blocks_live"))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_reference_goldens(tmp_path, mode):
    """1000.fastq, k = 21, MeraculousCounter's settings: both texts == the oracle's bytes, their sorted lines == the reference's own files"""
    rb = read_fastq(os.path.join(GOLDEN, "1000.fastq"))
    cfg = default_config(21, value_kind=KMR_VALUE_EXT, fastq_start_char=64, estimated_raw_kmers=56000, **MERA)
    o, p = both(cfg, rb, mode=mode)
    for graph, gold in ((False, "phix.mercount.m21"), (True, "phix.mergraph.m21.D2")):
        text, kept = device_text(p, 2, graph)
        assert text == oracle_text(o, tmp_path, 2, graph)
        assert kept == 5401
        assert sorted(text.decode().splitlines()) == sorted(open(os.path.join(GOLDEN, gold)).read().splitlines())


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("k", [13, 21, 31, 32, 33, 51, 63, 64, 65, 96, 97, 127])
def test_key_widths_and_value_kinds(tmp_path, k, ext):
    """k on both sides of every word and pad-bit border; reads with noisy qualities and N bases, so that the N and X tallies occur;
    min depth 0 .. 3 and one above every count"""
    rb = synth_reads(1500, read_len=150, genome_len=12000, seed=100 + k, quality="noisy", n_rate=0.004)
    kw = dict(value_kind=KMR_VALUE_EXT) if ext else {}
    cfg = default_config(k, estimated_raw_kmers=1500 * (150 - k + 1), **MERA, **kw)
    o, p = both(cfg, rb, min_depth=1)
    kinds = (False, True) if ext else (False,)
    for graph in kinds:
        for min_depth in (0, 1, 2, 3):
            want = oracle_text(o, tmp_path, min_depth, graph)
            assert len(want) > 0
            text, kept = device_text(p, min_depth, graph)
            assert text == want, (k, ext, graph, min_depth)
            assert 2 * kept == want.count(b"\n")
        assert device_text(p, 70000, graph) == (b"", 0)
        assert oracle_text(o, tmp_path, 70000, graph) == b""
    if ext:
        g = oracle_text(o, tmp_path, 1, True).decode().splitlines()
        cols = np.array([[int(x) for x in line.split("\t")[1].split()] for line in g[:20000]])
        # the X tallies (no neighbour, or one below the extension quality) are not all zero, left and right.  The N columns stay 0 in
        # any map built from reads: the reference takes a neighbour from the 2-bit form, where a non-ACGT base reads A
        assert cols.shape[1] == 13 and (cols[:, 5] > 0).any() and (cols[:, 11] > 0).any()
    else:
        with pytest.raises(ka.KmerSpectrumError, match=ERR_STATE) as ei:
            p.dumpGraphsText(2)
        assert "mergraph needs value_kind = KMR_VALUE_EXT" in str(ei.value)
        with pytest.raises(ka.KmerSpectrumError, match=ERR_STATE):
            p.dumpTextSize("mergraph", 2)


def test_number_widths(tmp_path):
    """A 300-base genome under 150 000 reads: counts of one to five digits with the saturated 65 535 among them, and tallies of six
    digits.  The widths are asserted on the EXPECTED text, so a shrunken input cannot hide a case."""
    rb = synth_reads(150000, read_len=150, genome_len=300, seed=9, err=0.01, quality="flat")
    cfg = default_config(21, value_kind=KMR_VALUE_EXT, estimated_raw_kmers=150000 * 130, **MERA)
    o, p = both(cfg, rb, min_depth=1)
    wc, wg = oracle_text(o, tmp_path, 1, False), oracle_text(o, tmp_path, 1, True)
    counts = [line.split(b"\t")[1] for line in wc.splitlines()]
    assert {len(c) for c in counts} >= {1, 2, 3, 4, 5} and b"65535" in counts
    assert max(len(x) for line in wg.splitlines() for x in line.split(b"\t")[1].split()) >= 6
    assert device_text(p, 1, False)[0] == wc
    assert device_text(p, 1, True)[0] == wg


def test_errors_before_finalize_and_bad_arguments():
    cfg = default_config(31, value_kind=KMR_VALUE_EXT, estimated_raw_kmers=10000, **MERA)
    p = product(cfg)
    with pytest.raises(ka.KmerSpectrumError, match=ERR_STATE):
        p.dumpCountsText(2)
    with pytest.raises(ka.KmerSpectrumError, match=ERR_STATE):
        p.dumpTextSize("mercount", 2)
    rb = synth_reads(200, read_len=100, genome_len=2000, seed=3)
    p.buildKmerSpectrum(rb.bases, rb.quals, rb.offsets)
    p.finalize(2)
    n = p.stats()["weak_entries"]
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        p.dumpTextSize(2, 2)                                  # unknown kind
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        p.dumpCountsText(2, n + 1, None)                      # entry_hi is clamped to n, entry_lo lies behind it
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        p.dumpCountsText(2, 5, 4)
    assert device_text(p, 2, False, n, None) == (b"", 0)     # an empty range at the end
    whole, kept = device_text(p, 2, False)
    assert device_text(p, 2, False, 0, n + 1000) == (whole, kept)
    with p.dumpCountsText(2) as t:
        small = np.zeros(8, dtype=np.uint8)
        assert p.lib.kmr_text_copy(t._t, small.ctypes.data_as(C.c_void_p), 8) == -6          # KMR_ERR_CAPACITY
    empty = product(cfg)
    empty.finalize(2)                                         # an empty map
    assert device_text(empty, 0, False) == (b"", 0) and device_text(empty, 0, True) == (b"", 0)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """a map of a few 10^5 entries, finalized at min depth 2 (so that a dump at min depth 3 leaves entries out), and the oracle's texts"""
    tmp = tmp_path_factory.mktemp("big")
    rb = synth_reads(60000, read_len=150, seed=21, quality="noisy", n_rate=0.001)
    cfg = default_config(31, value_kind=KMR_VALUE_EXT, estimated_raw_kmers=60000 * 120, **MERA)
    o, p = both(cfg, rb, min_depth=2)
    want = {graph: oracle_text(o, tmp, 3, graph) for graph in (False, True)}
    yield o, p, want, tmp
    p.close()


def test_ranges_concatenate(big):
    o, p, want, _ = big
    n = p.stats()["weak_entries"]
    assert n > 200000
    rng = np.random.default_rng(17)
    for graph in (False, True):
        kind = "mergraph" if graph else "mercount"
        # single-entry ranges: some hold a kept entry and some do not
        singles = [p.dumpTextSize(kind, 3, i, i + 1) for i in range(300)]
        assert {k for k, _ in singles} == {0, 1} and all((b == 0) == (k == 0) for k, b in singles)
        i_out = [k for k, _ in singles].index(0)
        cuts = sorted(set(rng.integers(0, n + 1, 40).tolist()) | {0, n, i_out, i_out + 1, 1000, 1001})
        cuts = sorted(cuts + [cuts[5], cuts[9], n])          # repeated cut points: empty ranges, one of them at the end
        parts, total_kept, seen = [], 0, set()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            text, kept = device_text(p, 3, graph, lo, hi)
            if hi == lo:
                assert (text, kept) == (b"", 0)
                seen.add("empty")
            elif hi == lo + 1:
                seen.add("single")
            if hi > lo and kept == 0:
                seen.add("none kept")
            parts.append(text)
            total_kept += kept
        assert seen == {"empty", "single", "none kept"}
        assert b"".join(parts) == want[graph]
        assert 2 * total_kept == want[graph].count(b"\n")


def test_file_forms_append_and_write_in_pieces(big):
    o, p, want, tmp = big
    for graph, dump in ((False, p.dumpCounts), (True, p.dumpGraphs)):
        path = str(tmp / ("file.%d" % graph))
        dump(path, 3)
        assert open(path, "rb").read() == want[graph]
        dump(path, 3)
        assert open(path, "rb").read() == want[graph] + want[graph]          # a second call appends
        # a staging bound of 1 MB: dozens of pieces
        assert len(want[graph]) > 8 << 20
        p.tune(dump_piece_bytes=1 << 20)
        path2 = path + ".pieces"
        dump(path2, 3)
        p.tune(dump_piece_bytes=0)
        assert open(path2, "rb").read() == want[graph]
    with pytest.raises(ka.KmerSpectrumError, match="cannot open"):
        p.dumpCounts(str(tmp / "no" / "such" / "directory"), 3)


def test_maps_that_were_not_just_built(big, tmp_path):
    o, p, want, _ = big
    cfg = o.cfg
    img = o.image(KMR_MAP_WEAK)
    q = product(cfg)
    q.load_image(KMR_MAP_WEAK, img)
    for graph in (False, True):
        assert device_text(q, 3, graph)[0] == want[graph]
    # merge: two spectra of different reads of one genome
    cfg2 = default_config(21, value_kind=KMR_VALUE_EXT, num_buckets_weak=2048, num_buckets_singleton=4096, **MERA)
    rb_a = synth_reads(3000, read_len=150, genome_len=30000, seed=70, quality="noisy", n_rate=0.001)
    rb_b = rb_a.slice(1500, 3000)
    rb_a = rb_a.slice(0, 1500)
    oa, pa = both(cfg2, rb_a)
    ob, pb = both(cfg2, rb_b)
    pa.merge_image(KMR_MAP_WEAK, pb.image(KMR_MAP_WEAK))
    oa.merge_add(ob)
    assert pa.stats()["weak_entries"] > 0
    for graph in (False, True):
        for min_depth in (2, 4):
            assert device_text(pa, min_depth, graph)[0] == oracle_text(oa, tmp_path, min_depth, graph)


def test_memory_returns_and_texts_are_independent(big):
    o, p, want, _ = big
    n = p.stats()["weak_entries"]
    p.dumpTextSize("mergraph", 3)          # (the handle's scan scratch is grow-only: have it before the baseline)
    base = live(p)
    a = p.dumpCountsText(3, 0, n // 2)
    b = p.dumpGraphsText(3, n // 2, None)
    assert live(p) == base + 2
    ta = a.numpy().tobytes()
    c = p.dumpCountsText(3, n // 2, None)          # a third text while two are live
    assert b.numpy().tobytes() == want[True][len(want[True]) - b.bytes:]
    assert a.numpy().tobytes() == ta == want[False][:a.bytes]
    assert ta + c.numpy().tobytes() == want[False]
    # the text where it lies: a torch view of the device memory
    import torch
    view = a.device_tensor()
    assert view.is_cuda and view.dtype == torch.uint8 and view.numel() == a.bytes
    assert view.cpu().numpy().tobytes() == ta
    del view
    a.close()
    assert live(p) == base + 2
    assert b.numpy().tobytes() == want[True][len(want[True]) - b.bytes:]
    b.close(); c.close()
    assert live(p) == base
    a.close()                                       # closing twice is harmless
    with pytest.raises(ka.KmerSpectrumError):
        a.numpy()
    p.dumpTextSize("mergraph", 3)
    assert live(p) == base


def test_tiles_per_block_change_no_byte(big):
    """kmr_tune "dump_tiles_per_block" at 2, 7 and more tiles than the text has: every block but the last walks several tiles, so
    all but a few hundredths of the 8 MB text's tile borders are crossed by the hand-off from tile to tile (at the default every
    block of a text this small bisects); the bytes stay the oracle's"""
    o, p, want, _ = big
    for graph in (False, True):
        tiles = -(-len(want[graph]) // 32768)
        assert tiles > 250
        for per_block in (2, 7, 100000):
            p.tune(dump_tiles_per_block=per_block)
            assert device_text(p, 3, graph)[0] == want[graph], (graph, per_block)
            assert int(p.build_info("dump_tiles_per_block")) == per_block
            assert int(p.build_info("dump_blocks")) == -(-tiles // per_block) < tiles
    p.tune(dump_tiles_per_block=0)
    assert device_text(p, 3, False)[0] == want[False]
    assert int(p.build_info("dump_tiles_per_block")) == 1 and int(p.build_info("dump_blocks")) == -(-len(want[False]) // 32768)
