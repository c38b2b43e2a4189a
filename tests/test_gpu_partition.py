"""selectReads' partitioned branch on the device (kmr_partition_reads, kmr_partition_read_batch; kmernator_amd/csrc/kmr_select.hpp):
--partition-by-depth, --remainder-trim and the per-input-file outputs, every byte and the segment table against the CPU
restatement of tests/refpartition.py; and the plain entry points (kmr_select_reads, kmr_filter_read_batch), which are its one round
over one input, through many units and tiles."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import kmernator_amd as ka
from helpers import GOLDEN
from refpartition import file_name, partition, passes_length, round_table

pytestmark = pytest.mark.gpu
K = 31
LABEL = b"MedianScore"


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def labels_of(n, action, lo, hi, to, tl, sc, wt):
    """FilterKnownOddities' AFTrim and setTrimHeaders' labels (src/ReadSelector.h:1015-1036); a discarded read has none"""
    out = []
    for i in range(n):
        if action is not None and action[i] == 2:
            out.append(b"")
            continue
        parts = []
        if action is not None and action[i] == 1:
            parts.append(b"AFTrim:%d+%d" % (lo[i], hi[i] - lo[i]))
        if wt[i]:
            parts.append(b"Trim:%d+%d" % (to[i], tl[i]))
        parts.append(LABEL + b":%d" % int(float(sc[i]) + 0.5))
        out.append(b" ".join(parts))
    return out


def fastq(names, seqs, quals):
    return b"".join(b"@" + names[i] + b"\n" + seqs[i] + b"\n+\n" + quals[i] + b"\n" for i in range(len(names)))


def flat_table(table):
    return np.array([c for row in table for c in row], dtype=np.uint64).reshape(-1, 4)


def device_table(sel):
    s = sel.segments
    return np.stack([s[k].reshape(-1) for k in ("first_pick", "picks", "first_byte", "bytes")], axis=1).astype(np.uint64)


class Case:
    """a read set with results of the earlier stages made up on the host, and a ReadSelector that holds them (the array form)"""

    def __init__(self, sp, names, seqs, quals, mate, action, lo, hi, to, tl, sc):
        n = len(names)
        self.n, self.seqs, self.quals, self.mate = n, seqs, quals, mate
        self.names = [nm.split(b" ")[0].split(b"\t")[0] for nm in names]          # what is printed of a name
        self.action, self.lo, self.hi, self.to, self.tl, self.sc = action, lo, hi, to, tl, sc
        self.wt = np.array([tl[i] < len(seqs[i]) for i in range(n)], dtype=np.uint8)
        self.labels = labels_of(n, action, lo, hi, to, tl, sc, self.wt)
        self.disc = [bool(a == 2) for a in action]
        self.rs = ka.ReadSet(sp, fastq(names, seqs, quals), input_quality_base=33)
        assert self.rs.n == n
        self.sel = ka.ReadSelector(sp, self.rs, mate=mate, filter_results=dict(action=action, min_pass=lo, max_pass=hi))
        self.sel.trims = (to, tl, sc, self.wt)

    def expect(self, rounds, input_starts, out_base=33, fasta=False):
        return partition(self.names, self.seqs, self.quals, self.labels, self.disc, self.to, self.tl, self.sc, self.mate, rounds, input_starts, out_base - 33, out_base, fasta)

    def close(self):
        self.sel.close()
        self.rs.close()


def random_seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


@pytest.fixture(scope="module")
def sp():
    s = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=100000, device=0))
    yield s
    s.close()


# ---------------------------------------------------------------- 1: a crafted batch through the array form

N_CRAFTED = 600
STARTS3 = [0, 250, 250, N_CRAFTED]          # three inputs, the middle one empty


def crafted_data():
    """600 reads of 1 to 150 bases.  Of every five reads (0, 3) and (1, 4) are pairs and 2 is single.  Scores sit on, half below and
    above every boundary of 16 / 8 / 4 / 2; trim lengths on both sides of 0.40 x L and of the remainder length 25; every 11th
    read carries an AFTrim label, every 13th is discarded."""
    rng = np.random.default_rng(31)
    n = N_CRAFTED
    L = [1 + (i * 37) % 150 for i in range(n)]
    assert set(L) == set(range(1, 151))
    names = [b"c%d/%d" % (i * 7, 1 + i % 2) + (b" comment" if i % 4 == 0 else (b"\ttab" if i % 9 == 0 else b"")) for i in range(n)]
    seqs = [random_seq(rng, l) for l in L]
    quals = [bytes(rng.integers(35, 74, l, dtype=np.uint8)) for l in L]
    mate = np.full(n, -1, dtype=np.int64)
    for b0 in range(0, n - 4, 5):
        mate[b0], mate[b0 + 3], mate[b0 + 1], mate[b0 + 4] = b0 + 3, b0, b0 + 4, b0 + 1
    scores = [16, 15.5, 17, 8, 7.5, 9, 4, 3.5, 5, 2, 1.5, 3, 0, 40]
    sc = np.array([scores[(i * 5 + i // 14) % 14] for i in range(n)], dtype=np.float32)
    tl = np.zeros(n, dtype=np.uint32)
    for i, l in enumerate(L):
        edge = int(np.floor(float(np.float32(0.40)) * l))
        tl[i] = min(l, [edge, edge + 1, l, 24, 25, 26, max(0, edge - 1), 1, 0, l][(i // 2 + i // 20) % 10])
    to = np.array([min(L[i] - int(tl[i]), i % 3) for i in range(n)], dtype=np.uint32)
    action = np.zeros(n, dtype=np.uint8)
    action[5::11] = 1
    action[3::13] = 2
    lo = np.where(action == 1, 2, 0).astype(np.uint32)
    hi = np.where(action == 1, 2 + np.array(L), np.array(L)).astype(np.uint32)
    # a discarded read whose mate passes the strictest round
    m = next(int(mate[i]) for i in range(3, n, 13) if mate[i] >= 0 and L[mate[i]] >= 60 and action[mate[i]] == 0)
    sc[m], tl[m], to[m] = 40, L[m], 0
    return names, seqs, quals, mate, action, lo, hi, to, tl, sc


@pytest.fixture(scope="module")
def crafted(sp):
    c = Case(sp, *crafted_data())
    yield c
    c.close()


@pytest.mark.parametrize("fmt,out_base", [("fastq", 33), ("fastq", 64), ("fasta", 33)])
@pytest.mark.parametrize("remainder", [-1.0, 25.0])
@pytest.mark.parametrize("both", [0, 1])
def test_crafted_batch_against_the_restatement(crafted, both, remainder, fmt, out_base):
    c = crafted
    rounds = round_table(2, 16, remainder, 0.40, 2 if both else 1)
    assert [r["depth"] for r in rounds] == [16, 8, 4, 2] + ([2] if remainder > 0 else [])
    want, table, rseg = c.expect(rounds, STARTS3, out_base, fmt == "fasta")
    files = c.sel.selectReads(2, 16, remainder, None, both, "MEDIAN", out_base, fmt, STARTS3, ["a", "b", "c"], "out", True)
    text = c.sel.writePicks(out_base, fmt)
    print("both %d remainder %s %s/%d: %d picks, %d bytes; picks per segment %s" % (both, remainder, fmt, out_base, c.sel.n_picked, len(text), [t[1] for row in table for t in row]))
    assert len(text) == len(want) and text == want
    assert np.array_equal(device_table(c.sel), flat_table(table))
    assert np.array_equal(c.sel.read_segment, rseg)
    assert [float(d) for d in c.sel.segments["round_depth"]] == [r["depth"] for r in rounds]
    assert list(c.sel.segments["round_is_remainder"]) == [r["is_remainder"] for r in rounds]
    # the case holds what it is meant to (judged on the expected side): every round and both non-empty inputs take reads, the
    # empty input none, and a discarded read is printed beside its passing mate
    picks = flat_table(table)[:, 1].reshape(len(rounds), 3)
    assert (picks[:, 0] > 0).all() and (picks[:, 2] > 0).all() and not picks[:, 1].any()
    if not both or remainder > 0:
        assert any(c.disc[i] and rseg[i] >= 0 for i in range(c.n))
    # every read in at most one segment, and the segments' counts are those of read_segment
    assert np.array_equal(np.bincount(rseg[rseg >= 0], minlength=len(rounds) * 3), picks.reshape(-1))
    assert np.array_equal(c.sel.picked_flags, rseg >= 0) and c.sel.n_picked == int((rseg >= 0).sum())
    # the files: names as the reference composes them, and each the slice of its segment
    want_files = []
    for r, rnd in enumerate(rounds):
        for f, prefix in enumerate("abc"):
            fp, np_, fb, nb = table[r][f]
            if np_:
                want_files.append((file_name("out", 2, rnd, True, prefix, True, fmt == "fasta"), want[fb:fb + nb]))
    assert files == want_files
    if not both and remainder <= 0:
        # what the rounds pick between them is what one selection at the minimum depth picks
        c.sel.pickAllPassingPairs(2, None, False)
        assert np.array_equal(c.sel.picked_flags, rseg >= 0)


def test_partition_off_is_the_plain_selection(crafted):
    c = crafted
    for both in (0, 1):
        for fmt, base in (("fastq", 33), ("fasta", 33), ("fastq", 64)):
            got = c.sel.selectReads(2.5, 0, 25.0, 0.5, both, "MEDIAN", base, fmt, separate_outputs=False)
            flags = c.sel.picked_flags.copy()
            seg = c.sel.segments
            assert seg["picks"].shape == (1, 1) and int(seg["picks"][0, 0]) == c.sel.n_picked and int(seg["bytes"][0, 0]) == len(got[0][1])
            c.sel.pickAllPassingPairs(2.5, 0.5, both)
            assert got == [("", c.sel.writePicks(base, fmt))] and len(got[0][1]) > 0
            assert np.array_equal(flags, c.sel.picked_flags)


# ---------------------------------------------------------------- 3: many units, many tiles a unit

N_MANY = 40_000


def many_data():
    rng = np.random.default_rng(77)
    n = N_MANY
    L = rng.integers(8, 41, n)
    names = [b"m%d" % i for i in range(n)]
    blob = random_seq(rng, int(L.sum()))
    qblob = bytes(rng.integers(35, 74, int(L.sum()), dtype=np.uint8))
    off = np.concatenate([[0], np.cumsum(L)])
    seqs = [blob[off[i]:off[i + 1]] for i in range(n)]
    quals = [qblob[off[i]:off[i + 1]] for i in range(n)]
    sc = rng.integers(0, 41, n).astype(np.float32)
    tl = np.minimum(L, rng.integers(0, 41, n)).astype(np.uint32)
    to = ((L - tl) // 2).astype(np.uint32)
    zero = np.zeros(n, dtype=np.uint32)
    return names, seqs, quals, np.arange(n, dtype=np.int64) ^ 1, np.zeros(n, dtype=np.uint8), zero, L.astype(np.uint32), to, tl, sc


@pytest.fixture(scope="module")
def many(sp):
    c = Case(sp, *many_data())
    yield c
    c.close()


@pytest.mark.parametrize("units", [0, 7, 64])
def test_many_units_and_tiles_against_the_restatement(sp, many, units):
    """40 000 reads, rounds 32 / 16 / 8 / 4 / 2 and a remainder, two inputs: 625 units of one tile by default; 7 units of 90 tiles
    and 64 of 10 (kmr_tune partition_units) walk the running per-segment bases through a unit"""
    c = many
    starts = [0, 17001, N_MANY]
    rounds = round_table(2, 32, 12.0, 0.40, 2)
    assert len(rounds) == 6
    want, table, rseg = c.expect(rounds, starts)
    sp.tune(partition_units=units)
    try:
        c.sel.selectReads(2, 32, 12.0, None, True, input_starts=starts, separate_outputs=False)
    finally:
        sp.tune(partition_units=0)
    text = c.sel.writePicks()
    print("units %d: %d picks of %d, %d bytes, picks per segment %s" % (units, c.sel.n_picked, c.n, len(text), [t[1] for row in table for t in row]))
    assert all(t[1] > 300 for row in table for t in row)
    assert np.array_equal(device_table(c.sel), flat_table(table))
    assert np.array_equal(c.sel.read_segment, rseg)
    for fp, np_, fb, nb in flat_table(table):
        assert hashlib.sha1(text[int(fb):int(fb + nb)]).digest() == hashlib.sha1(want[int(fb):int(fb + nb)]).digest()
    assert len(text) == len(want)


# ---------------------------------------------------------------- 3b: the plain entry points walk the same units and tiles

def expect_plain(c, min_score, both, mate, lo=0, hi=None):
    """the restatement's one round at min_score, no input_starts, over reads [lo, hi) of a case, with `mate` (indices into the
    cut, or None for pickAllPassingReads): (text, flags)"""
    hi = c.n if hi is None else hi
    rounds = round_table(min_score, 0, -1.0, 0.40, 2 if both else 1)
    assert len(rounds) == 1 and rounds[0]["depth"] == min_score and not rounds[0]["is_remainder"]
    want, table, rseg = partition(c.names[lo:hi], c.seqs[lo:hi], c.quals[lo:hi], c.labels[lo:hi], c.disc[lo:hi], c.to[lo:hi], c.tl[lo:hi], c.sc[lo:hi], mate, rounds, None, 0, 33, False)
    assert table[0][0][1] == int((rseg >= 0).sum()) and table[0][0][3] == len(want)
    return want, rseg >= 0


@pytest.fixture(scope="module")
def many_plain_want(many):
    return {"either": expect_plain(many, 8, False, many.mate), "both": expect_plain(many, 8, True, many.mate), "reads": expect_plain(many, 8, False, None)}


@pytest.mark.parametrize("units", [0, 7, 64])
def test_plain_entry_point_over_many_units_and_tiles(sp, many, many_plain_want, units):
    """kmr_select_reads over 40 000 reads, pairs i ^ 1: 625 units of one tile by default, 7 units of 90 tiles and 64 of 10"""
    c = many
    sp.tune(partition_units=units)
    try:
        for key, both in (("either", False), ("both", True)):
            want, flags = many_plain_want[key]
            assert c.sel.pickAllPassingPairs(8, None, both) == int(flags.sum())
            text = c.sel.writePicks()
            print("units %d, %s: %d picks of %d, %d bytes" % (units, key, c.sel.n_picked, c.n, len(text)))
            assert 300 < flags.sum() < c.n - 300
            assert len(text) == len(want) and text == want and np.array_equal(c.sel.picked_flags, flags)
        want, flags = many_plain_want["reads"]
        assert c.sel.pickAllPassingReads(8, None) == int(flags.sum())
        text = c.sel.writePicks()
        assert 300 < flags.sum() < c.n - 300
        assert len(text) == len(want) and text == want and np.array_equal(c.sel.picked_flags, flags)
    finally:
        sp.tune(partition_units=0)


CUT_AT = 2          # reads 2, 3, 4 of the many: the first passes a minimum score of 8, the next two do not


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129])
def test_plain_entry_point_at_unit_and_tile_edges(sp, many, n):
    """kmr_select_reads with two units over n reads cut from the many, pairs i ^ 1 and the last read single when n is odd: one tile
    short of, at and past a tile and two tiles.  Every batch of two reads or more picks a read and drops one; for n = 2 that can
    hold only read by read (a pair is picked or dropped whole), so every batch also runs through pickAllPassingReads"""
    m = many
    lo, hi = CUT_AT, CUT_AT + n
    mate = np.arange(n, dtype=np.int64) ^ 1
    mate[mate >= n] = -1
    c = Case(sp, m.names[lo:hi], m.seqs[lo:hi], m.quals[lo:hi], mate, m.action[lo:hi], m.lo[lo:hi], m.hi[lo:hi], m.to[lo:hi], m.tl[lo:hi], m.sc[lo:hi])
    sp.tune(partition_units=2)
    try:
        for use_mate in (True, False):
            want, flags = expect_plain(m, 8, False, mate if use_mate else None, lo, hi)
            if n >= (3 if use_mate else 2):
                assert flags.any() and not flags.all()
            got = c.sel.pickAllPassingPairs(8, None, False) if use_mate else c.sel.pickAllPassingReads(8, None)
            text = c.sel.writePicks()
            print("n %d, %s: %d picks, %d bytes" % (n, "pairs" if use_mate else "reads", got, len(text)))
            assert got == c.sel.n_picked == int(flags.sum())
            assert text == want and np.array_equal(c.sel.picked_flags, flags)
    finally:
        sp.tune(partition_units=0)
        c.close()


# ---------------------------------------------------------------- 4: the fused form on the reference's own fixture

def test_fused_form_on_the_reference_fixture():
    """tests/golden/1000.fastq as test_read_selector's golden test sets it up (artifact filter, k = 31, min depth 2, min read length
    25, quality base 64): partition_by_depth = min_depth reproduces 1000-Filtered.fastq; 16 with remainder 25 against the
    restatement over the oracle's score_and_trim; the text handed in as device memory gives the same bytes"""
    import torch
    from helpers import OracleSpectrum, ReadBatch, default_config, oracle_weighted_kmers
    from refsemantics import score_and_trim
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, golden("1000.fastq"))
    f = ka.FilterKnownOddities(sp, golden("artifact_sequences.fa"), edit_distance=1, min_read_length=25.0)
    res, frs = f.applyFilter(rs)
    assert frs.n == 1000
    sp.buildKmerSpectrumFromReadSet(frs)
    sp.finalize(2)
    mate = np.arange(1000, dtype=np.int64) ^ 1
    sel = ka.ReadSelector(sp, frs, mate=mate, filter_results=res)
    got = sel.selectReads(2, 2, -1.0, 25.0, False, "MEDIAN", 64, "fastq", output="1000-Filtered", input_prefixes=["1000"])
    want = golden("1000-Filtered.fastq").replace(b"\t", b" ")
    assert [nm for nm, _ in got] == ["1000-Filtered-MinDepth2-PartitionDepth2-1000.fastq"]
    assert got[0][1].replace(b"\t", b" ") == want
    # the oracle's trims of the filtered reads
    b, q, off, names = frs.arrays()
    n = frs.n
    seqs = [bytes(b[int(off[i]):int(off[i + 1])]) for i in range(n)]
    quals = [bytes(q[int(off[i]):int(off[i + 1])]) for i in range(n)]
    short = [nm.split(b" ")[0].split(b"\t")[0] for nm in names]
    ocfg = default_config(K, estimated_raw_kmers=46000)
    o = OracleSpectrum(ocfg)
    o.add_reads(ReadBatch.from_arrays(np.ascontiguousarray(b), np.ascontiguousarray(q), np.ascontiguousarray(off, dtype=np.uint64)))
    o.finalize(2)
    to, tl, sc, wt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    for i in range(n):
        keys, _, _ = oracle_weighted_kmers(ocfg, seqs[i], quals[i])
        to[i], tl[i], sc[i], wt[i] = score_and_trim(o.lookup(keys), seqs[i], K, 2, "MEDIAN")
    action = res["action"]
    labels = labels_of(n, action, res["min_pass"], res["max_pass"], to, tl, sc, wt)
    rounds = round_table(2, 16, 25.0, 25.0, 2)
    assert [r["is_remainder"] for r in rounds] == [False] * 4 + [True]
    want, table, rseg = partition(short, seqs, quals, labels, list(action == 2), to, tl, sc, mate, rounds, None, 64 - 33, 64, False)
    got = sel.selectReads(2, 16, 25.0, 25.0, True, "MEDIAN", 64, "fastq", separate_outputs=False)[0][1]
    print("1000.fastq, 16 over 2 with remainder 25: picks per round %s, %d bytes" % ([row[0][1] for row in table], len(want)))
    assert sum(1 for row in table if row[0][1]) >= 3
    assert got == want and np.array_equal(sel.read_segment, rseg) and np.array_equal(device_table(sel), flat_table(table))
    # the _dev form
    lib = sp.lib
    dtext = torch.frombuffer(bytearray(frs.text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    cfg = ka.KmrPartitionConfig()
    lib.kmr_partition_config_init(C.byref(cfg))
    cfg.select.min_read_length, cfg.select.both_pass, cfg.select.output_quality_base, cfg.partition_by_depth, cfg.remainder_trim = 25.0, 1, 64, 16, 25.0
    act = np.ascontiguousarray(action, dtype=np.uint8); lo = np.ascontiguousarray(res["min_pass"], dtype=np.uint32); hi = np.ascontiguousarray(res["max_pass"], dtype=np.uint32)
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    out = C.c_void_p()
    rc = lib.kmr_partition_read_batch_dev(sp.h, frs.r, dtext.data_ptr(), dtext.numel(), mate.ctypes.data_as(C.POINTER(C.c_int64)), act.ctypes.data_as(u8), lo.ctypes.data_as(u32), hi.ctypes.data_as(u32),
                                          None, 0, C.byref(cfg), C.byref(out))
    assert rc == 0, lib.kmr_last_error(sp.h)
    nb = C.c_uint64()
    assert lib.kmr_picks_info(out, None, C.byref(nb)) == 0 and nb.value == len(want)
    buf = np.zeros(nb.value, dtype=np.uint8)
    assert lib.kmr_picks_copy(out, buf.ctypes.data_as(C.c_void_p), nb.value, None) == 0
    lib.kmr_picks_free(out)
    assert buf.tobytes() == want
    sel.close(); frs.close(); rs.close(); f.close(); sp.close()


@pytest.mark.parametrize("units", [0, 7])
def test_plain_fused_form_on_the_reference_fixture(units):
    """kmr_filter_read_batch on the same fixture (min depth 2, min read length 25, quality base 64) writes 1000-Filtered.fastq
    whatever the number of units"""
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, golden("1000.fastq"))
    f = ka.FilterKnownOddities(sp, golden("artifact_sequences.fa"), edit_distance=1, min_read_length=25.0)
    res, frs = f.applyFilter(rs)
    sp.buildKmerSpectrumFromReadSet(frs)
    sp.finalize(2)
    sel = ka.ReadSelector(sp, frs, mate=np.arange(1000, dtype=np.int64) ^ 1, filter_results=res)
    sp.tune(partition_units=units)
    got = sel.filterReads(2.0, 25.0, False, "MEDIAN", 64, "fastq")
    want = golden("1000-Filtered.fastq").replace(b"\t", b" ")
    assert len(want) > 0 and got.replace(b"\t", b" ") == want and sel.n_picked == want.count(b"\n") // 4
    sel.close(); frs.close(); rs.close(); f.close(); sp.close()


# ---------------------------------------------------------------- 5: edges

def _live(sp):
    return int(sp.build_info("device_blocks_live"))


def test_edges_of_the_partition(sp, crafted):
    lib = sp.lib
    c = crafted
    # an empty batch
    empty = ka.ReadSet(sp, b"")
    sel = ka.ReadSelector(sp, empty)
    sel.trims = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    assert sel.selectReads(2, 16, 25.0) == [] and sel.n_picked == 0 and sel.bytes == 0 and sel.segments["picks"].shape == (5, 1)
    sel.close(); empty.close()
    # no read passes: zero bytes, every segment empty
    assert c.sel.selectReads(1000, 16000, 25.0, 151.0, input_starts=STARTS3, input_prefixes="abc") == []
    assert c.sel.n_picked == 0 and c.sel.bytes == 0 and not c.sel.segments["picks"].any() and (c.sel.read_segment == -1).all()
    # partition_by_depth below min_depth: no round
    assert c.sel.selectReads(8, 4, 25.0) == [] and c.sel.segments["picks"].shape == (0, 1) and (c.sel.read_segment == -1).all()
    # every read lands in the remainder: nothing is as long as 151 bases, two bases are enough for the remainder
    files = c.sel.selectReads(0, 1, 2.0, 151.0, input_prefixes=["x"], output="o")
    ok = np.array([not c.disc[i] and passes_length(float(c.tl[i]), len(c.seqs[i]), 2.0) for i in range(c.n)])
    m = c.mate
    want_flags = np.array([ok[i] or (m[i] >= 0 and ok[m[i]]) for i in range(c.n)])
    assert [nm for nm, _ in files] == ["o-MinDepth0-Remainder-x.fastq"]
    assert list(c.sel.segments["round_is_remainder"]) == [False, False, True] and list(c.sel.segments["picks"][:, 0]) == [0, 0, int(want_flags.sum())]
    assert np.array_equal(c.sel.read_segment, np.where(want_flags, 2, -1))
    # 32 rounds
    c.sel.selectReads(1, 2 ** 31, -1.0, 0.0)
    want, table, rseg = c.expect(round_table(1, 2 ** 31, -1.0, 0.0, 1), None)
    assert c.sel.segments["picks"].shape == (32, 1) and c.sel.writePicks() == want and np.array_equal(c.sel.read_segment, rseg)
    assert float(c.sel.segments["round_depth"][0]) == 2.0 ** 31 and len(set(rseg[rseg >= 0])) >= 5
    # rounds x inputs: 4 x 64 = 256 is the bound, 4 x 65 is one above
    starts = list(range(0, 64)) + [c.n]
    c.sel.selectReads(2, 16, -1.0, input_starts=starts)
    want, table, rseg = c.expect(round_table(2, 16), starts)
    assert c.sel.segments["picks"].shape == (4, 64) and c.sel.writePicks() == want and np.array_equal(device_table(c.sel), flat_table(table))
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_UNSUPPORTED"):
        c.sel.selectReads(2, 16, -1.0, input_starts=list(range(0, 65)) + [c.n])
    # input_starts that does not end at n_reads
    with pytest.raises(ka.KmerSpectrumError, match="input_starts"):
        c.sel.selectReads(2, 16, -1.0, input_starts=[0, 10, c.n - 1])
    # a short buffer
    c.sel.selectReads(2, 16, 25.0)
    buf = np.zeros(c.sel.bytes, dtype=np.uint8)
    assert lib.kmr_picks_copy(c.sel._picks, buf.ctypes.data_as(C.c_void_p), c.sel.bytes - 1, None) == -6
    assert lib.kmr_picks_copy(c.sel._picks, buf.ctypes.data_as(C.c_void_p), c.sel.bytes, None) == 0
    # the segment accessors on picks of the plain entry point
    c.sel.pickAllPassingPairs(2, None, False)
    seg = c.sel._segments()
    assert seg["picks"].shape == (1, 1) and int(seg["picks"][0, 0]) == c.sel.n_picked and int(seg["bytes"][0, 0]) == c.sel.bytes and float(seg["round_depth"][0]) == 2.0
    c.sel.writePicks()
    assert np.array_equal(c.sel.read_segment, np.where(c.sel.picked_flags, 0, -1))


def test_partition_picks_give_every_block_back(sp, crafted):
    """device_blocks_live returns to where it was once the picks are freed, also after a call that failed behind its allocations"""
    c = crafted
    c.sel.close()
    base = _live(sp)
    assert len(c.sel.selectReads(2, 16, 25.0)) > 0
    assert _live(sp) == base + 3         # the text, the flags and the segment of every read
    c.sel.selectReads(2, 16, -1.0, input_starts=STARTS3)
    assert _live(sp) == base + 3         # the earlier picks were freed
    c.sel.close()
    assert _live(sp) == base
    good = c.sel.mate
    c.sel.mate = good.copy()
    c.sel.mate[0] = c.n + 5
    for _ in range(2):
        with pytest.raises(ka.KmerSpectrumError, match="mate"):
            c.sel.selectReads(2, 16, 25.0)
        assert _live(sp) == base
    c.sel.mate = good


# ---------------------------------------------------------------- 6: the Python layer

def test_python_layer_names_and_slices(crafted):
    c = crafted
    rounds = round_table(2, 16, 25.0, 0.40, 1)
    want, table, _ = c.expect(rounds, STARTS3)
    files = c.sel.selectReads(2, 16, 25.0, input_starts=STARTS3, input_prefixes=["lib1", "lib2", "lib3"], output="results/run")
    names = [nm for nm, _ in files]
    assert names == ["results/run-MinDepth2-%s-%s.fastq" % (d, p) for d in ("PartitionDepth16", "PartitionDepth8", "PartitionDepth4", "PartitionDepth2", "Remainder") for p in ("lib1", "lib3")]
    k = 0
    for r in range(5):
        for f in (0, 2):
            fp, np_, fb, nb = table[r][f]
            assert files[k][1] == want[fb:fb + nb] and nb > 0
            k += 1
    assert c.sel.selectReads(2, 16, 25.0, input_starts=STARTS3, output="results/run", separate_outputs=False) == [("results/run", want)]
    # without prefixes: the reference's name for reads of no input file
    assert c.sel.selectReads(2, 2, -1.0)[0][0] == "-MinDepth2-PartitionDepth2-transformed-1.fastq"
    assert c.sel.selectReads(2, 0, -1.0, format="fasta")[0][0] == "-MinDepth2-transformed-1.fasta"
