"""Duplicate-fragment collapse on the device (kmr_dedup_fragments*, kmr_dedup.hpp) against the sequential restatement of
DuplicateFragmentFilter::_filterDuplicateFragments in tests/refdedup.py: discard flags, the four skip counters, affected, the
group list and the consensus batch's bases, qualities, lengths and names, byte for byte."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kmernator_amd as ka
from kmernator_amd import _lib
from helpers import GOLDEN
import refdedup

pytestmark = pytest.mark.gpu
K = 31


def spectrum(**kw):
    return ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 16, device=0, **kw))


def consensus_records(res):
    """the consensus batch as refdedup has it: [(name, bases, quals)]"""
    cs = res.consensus
    assert cs.n == res.n_new_reads == res.n_groups * (2 if res.paired else 1)
    b, q, o, names = cs.arrays()
    assert int(o[0]) == 0 and int(o[-1]) == cs.total_bases
    text = cs.text
    assert text.count(b"\n") == cs.n and (cs.n == 0 or text.endswith(b"\n"))
    out = []
    for i in range(cs.n):
        lo, hi = int(o[i]), int(o[i + 1])
        out.append((names[i].decode(), b[lo:hi].tobytes().decode(), q[lo:hi].tobytes().decode()))
    assert b"".join(n + b"\n" for n in names) == text
    return out


def check(res, want, what=""):
    assert np.array_equal(res.discarded, want.discarded_array()), what
    assert list(res.skipped) == want.skipped, what
    assert res.affected == want.affected, what
    assert np.array_equal(res.groups, want.group_array()), what
    assert consensus_records(res) == want.consensus, what
    assert np.array_equal(res.consensus_mate, (np.arange(res.n_new_reads) ^ 1) if res.paired else np.full(res.n_new_reads, -1)), what


def run(sp, rs, pairs, discarded, cfg, device_text=None):
    f = ka.DuplicateFragmentFilter(sp, cfg["dedup_mode"], cfg["dedup_length"], cfg["start_offset"])
    return f._pass(rs, pairs, discarded, cfg["paired"], device_text)


def device_text_of(rs):
    import torch
    t = torch.frombuffer(bytearray(rs.text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("case", refdedup.HAND_CASES, ids=[c[0] for c in refdedup.HAND_CASES])
def test_hand_worked_cases(case):
    label, reads, cfg, discarded, expect = case
    sp = spectrum()
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    pairs = rs.identifyPairs()
    assert [tuple(p) for p in pairs.pairs.tolist()] == refdedup.pair_list(reads)
    dt = device_text_of(rs)
    for res in (run(sp, rs, pairs, discarded, cfg), run(sp, rs, pairs, discarded, cfg, dt.data_ptr())):
        assert [tuple(g) for g in res.groups.tolist()] == expect["groups"], label
        assert list(res.skipped) == expect["skipped"] and res.discarded.tolist() == expect["discarded"] and res.affected == expect["affected"], label
        assert consensus_records(res) == expect["consensus"], label
        check(res, refdedup.run_case(case), label)
        res.close()


@functools.lru_cache(maxsize=None)
def generated(seed):
    reads, discarded = refdedup.generate(seed)
    return reads, discarded, refdedup.pair_list(reads), refdedup.fastq_text(reads)


@pytest.mark.parametrize("geometry", [(4, 0), (24, 0), (24, 4), (32, 8), (48, 0), (64, 0)], ids=lambda g: "len%d_off%d" % g)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generated_batches(seed, mode, geometry):
    """the paired pass, then the single pass on its discards (what --dedup-single runs); seed 1 also through the device-text entry points"""
    reads, discarded, pair_list, text = generated(seed)
    sp = spectrum()
    rs = ka.ReadSet(sp, text)
    pairs = rs.identifyPairs()
    assert [tuple(p) for p in pairs.pairs.tolist()] == pair_list
    cfg = dict(dedup_mode=mode, dedup_length=geometry[0], start_offset=geometry[1])
    want = refdedup.filter_duplicate_fragments(reads, pair_list, discarded, paired=True, **cfg)
    want1 = refdedup.filter_duplicate_fragments(reads, pair_list, want.discarded, paired=False, **cfg)
    f = ka.DuplicateFragmentFilter(sp, mode, *geometry)
    dt = device_text_of(rs) if seed == 1 else None
    res = f.filterDuplicateFragments(rs, pairs, discarded, dedup_single=True, device_text=None if dt is None else dt.data_ptr())
    check(res, want, "paired")
    check(res.single, want1, "single")
    # (windows of 64 and 128 bases leave few of the 30 to 150 base reads long enough)
    assert res.n_groups > (20 if geometry[0] <= 32 else 5) and (geometry[0] > 32 or res.single.n_groups > 2)
    res.close()


def test_one_large_group_among_many_small_ones():
    """a member loop longer than a wavefront, more groups than one block of wavefronts takes"""
    rng = np.random.default_rng(5)
    rnd = lambda n: "".join("ACGT"[v] for v in rng.integers(0, 4, n))
    qual = lambda n: "".join(chr(33 + int(v)) for v in rng.integers(2, 41, n))
    reads = []
    frags = [(rnd(24), rnd(24), 300)] + [(rnd(24), rnd(24), 2) for _ in range(230)]
    order = [i for i, f in enumerate(frags) for _ in range(f[2])]
    rng.shuffle(order)
    for j, i in enumerate(order):
        l1, l2 = int(rng.integers(24, 100)), int(rng.integers(24, 100))
        reads.append(("r%d/1" % j, frags[i][0] + rnd(l1 - 24), qual(l1)))
        reads.append(("r%d/2" % j, frags[i][1] + rnd(l2 - 24), qual(l2)))
    pair_list = refdedup.pair_list(reads)
    want = refdedup.filter_duplicate_fragments(reads, pair_list, None, dedup_mode=2, dedup_length=24)
    assert sorted(m for _, m in want.groups)[-2:] == [2, 300] and len(want.groups) == 231
    sp = spectrum()
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    res = ka.DuplicateFragmentFilter(sp, 2).filterDuplicateFragments(rs, rs.identifyPairs())
    check(res, want)


def test_empty_no_pairs_no_duplicates_and_one_group():
    sp = spectrum()
    f = ka.DuplicateFragmentFilter(sp, 2, 8)
    # empty
    rs = ka.ReadSet(sp, b"")
    res = f.filterDuplicateFragments(rs, rs.identifyPairs(), dedup_single=True)
    for r in (res, res.single):
        assert (r.n_groups, r.n_new_reads, r.affected, r.skipped) == (0, 0, 0, (0, 0, 0, 0)) and r.discarded.size == 0 and r.consensus.n == 0 and r.groups.shape == (0, 2)
    # no pairs: single reads only; the paired pass counts every record as unpaired
    reads = [("s%d" % i, "ACGTACGTACGTACGT"[i % 4:] + "ACGT"[i % 4] * (i // 4 + 1), "I" * (17 - i % 4 + i // 4)) for i in range(12)]
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    pairs = rs.identifyPairs()
    res = f.filterDuplicateFragments(rs, pairs, dedup_single=True)
    pl = refdedup.pair_list(reads)
    check(res, refdedup.filter_duplicate_fragments(reads, pl, None, dedup_mode=2, dedup_length=8))
    check(res.single, refdedup.filter_duplicate_fragments(reads, pl, None, dedup_mode=2, dedup_length=8, paired=False))
    assert res.skipped == (0, 0, 12, 0) and res.n_groups == 0 and consensus_records(res) == []
    # no duplicates among pairs
    rng = np.random.default_rng(3)
    rnd = lambda n: "".join("ACGT"[v] for v in rng.integers(0, 4, n))
    reads = [("p%d/%d" % (i // 2, 1 + i % 2), rnd(40), "I" * 40) for i in range(200)]
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    res = ka.DuplicateFragmentFilter(sp, 2, 16).filterDuplicateFragments(rs, rs.identifyPairs())
    check(res, refdedup.filter_duplicate_fragments(reads, refdedup.pair_list(reads), None, dedup_mode=2, dedup_length=16))
    assert res.n_groups == 0 and not res.discarded.any()
    # every pair is one group
    a, b = rnd(16), rnd(16)
    reads = [("q%d/%d" % (i // 2, 1 + i % 2), (a if i % 2 == 0 else b) + rnd(i % 7), "I" * (16 + i % 7)) for i in range(70)]
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    res = ka.DuplicateFragmentFilter(sp, 1, 16).filterDuplicateFragments(rs, rs.identifyPairs())
    want = refdedup.filter_duplicate_fragments(reads, refdedup.pair_list(reads), None, dedup_mode=1, dedup_length=16)
    check(res, want)
    assert want.groups == [(0, 35)] and res.discarded.all()


def test_mode_off_and_refused_configurations():
    sp = spectrum()
    reads = refdedup.HAND_CASES[0][1]
    rs = ka.ReadSet(sp, refdedup.fastq_text(reads))
    pairs = rs.identifyPairs()
    res = ka.DuplicateFragmentFilter(sp, 0, 4).filterDuplicateFragments(rs, pairs, discarded=[0, 1, 0, 0])          # the stage is off
    assert res.n_groups == 0 and res.discarded.tolist() == [0, 1, 0, 0] and res.skipped == (0, 0, 0, 0)
    buf = np.frombuffer(rs.text, dtype=np.uint8)

    def rc_of(**fields):
        c = _lib.KmrDedupConfig()
        sp.lib.kmr_dedup_config_init(C.byref(c))
        c.dedup_mode = 1
        for k, v in fields.items():
            setattr(c, k, v)
        out = C.c_void_p()
        rc = sp.lib.kmr_dedup_fragments(sp.h, rs.r, buf.ctypes.data_as(C.c_void_p), buf.size, pairs._live(), None, C.byref(c), C.byref(out))
        if out.value:
            sp.lib.kmr_dedup_free(out)
        return rc
    assert rc_of() == 0
    assert rc_of(edit_distance=1) == -7 and rc_of(consensus=0) == -7 and rc_of(dedup_length=68) == -7
    assert rc_of(dedup_length=22) == -1 and rc_of(start_offset=2) == -1 and rc_of(struct_size=8) == -1
    # the pair list of another batch
    other = ka.ReadSet(sp, refdedup.fastq_text(reads[:2]))
    with pytest.raises(ka.KmerSpectrumError, match="pair list belongs"):
        ka.DuplicateFragmentFilter(sp, 1, 4).filterDuplicateFragments(other, pairs)
    # a text that is not the batch's
    out = C.c_void_p()
    c = ka.DuplicateFragmentFilter(sp, 2, 4).cfg
    assert sp.lib.kmr_dedup_fragments(sp.h, rs.r, buf.ctypes.data_as(C.c_void_p), 10, pairs._live(), None, C.byref(c), C.byref(out)) == -1 and not out.value
    assert b"name span" in sp.lib.kmr_last_error(sp.h)


def test_end_to_end_on_the_golden_reads():
    """1000.fastq (Phred-64, ingested at base 64; the batch holds it at the handle's base 33, which is what refdedup is given) with
    every read pair written twice under distinct names: ingest, identifyPairs, dedup, the spectrum of the surviving reads plus the
    consensus reads, FilterReads' output of both batches.  The consensus batch also goes through identifyPairs and the artifact filter."""
    src = refdedup.parse_fastq(open(os.path.join(GOLDEN, "1000.fastq"), "rb").read())
    raw = []
    for i in range(0, len(src), 2):
        for copy in "ab":
            for e in (0, 1):
                name = src[i + e][0]
                stem, tail = (name[:-2], name[-2:]) if name[-2] == "/" else (name, "")
                raw.append((stem + copy + tail, src[i + e][1], src[i + e][2]))
    reads = [(n, b, "".join(chr(ord(c) - 31) for c in q)) for n, b, q in raw]          # as the reference rescales them (src/ReadSet.cpp:324-337)
    pair_list = refdedup.pair_list(reads)
    assert len(pair_list) == len(reads) // 2
    want = refdedup.filter_duplicate_fragments(reads, pair_list, None, dedup_mode=2, dedup_length=24)
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 20, device=0))
    rs = ka.ReadSet(sp, refdedup.fastq_text(raw), input_quality_base=64)
    assert rs.n == len(reads) and rs.arrays()[1].tobytes().decode() == "".join(q for _, _, q in reads)
    pairs = rs.identifyPairs()
    res = ka.DuplicateFragmentFilter(sp, 2).filterDuplicateFragments(rs, pairs)
    check(res, want)
    assert res.n_groups >= 400
    # what refdedup's consensus reads give as a batch of their own: the yardstick of everything the consensus batch goes through
    ref_cons = ka.ReadSet(sp, refdedup.fastq_text(want.consensus))
    cmate = np.arange(len(want.consensus), dtype=np.int64) ^ 1
    got_pairs, ref_pairs = res.consensus.identifyPairs(), ref_cons.identifyPairs()
    assert np.array_equal(got_pairs.mate, cmate) and np.array_equal(ref_pairs.mate, cmate) and np.array_equal(res.consensus_mate, cmate)
    af = ka.FilterKnownOddities(sp, open(os.path.join(GOLDEN, "artifact_sequences.fa"), "rb").read())
    got_af, got_filtered = af.applyFilter(res.consensus, mate=cmate)
    ref_af, ref_filtered = af.applyFilter(ref_cons, mate=cmate)
    for key in ref_af:
        assert np.array_equal(got_af[key], ref_af[key]), key
    for x, y in zip(got_filtered.arrays()[:3], ref_filtered.arrays()[:3]):
        assert np.array_equal(x, y)
    # the spectrum: surviving reads of the main batch, then the consensus batch
    pb, pq, po = C.c_void_p(), C.c_void_p(), C.c_void_p()
    sp.lib.kmr_reads_device_ptrs(rs.r, C.byref(pb), C.byref(pq), C.byref(po))
    ddisc = res.device_ptrs()[0]
    sp.buildKmerSpectrumDevice(pb, pq, po, rs.n, rs.total_bases, 0, C.c_void_p(ddisc))
    sp.sync()
    sp.buildKmerSpectrumFromReadSet(res.consensus, rs.n)
    sp.finalize(2)
    # ... against a build from refdedup's surviving reads plus its consensus reads
    keep = [r for r, d in zip(reads, want.discarded) if not d] + [(n, b, q) for n, b, q in want.consensus]
    sp2 = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 20, device=0))
    bases = np.frombuffer("".join(r[1] for r in keep).encode(), dtype=np.uint8)
    quals = np.frombuffer("".join(r[2] for r in keep).encode(), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(r[1]) for r in keep])]).astype(np.uint64)
    sp2.buildKmerSpectrum(bases, quals, offs)
    sp2.finalize(2)
    d1, d2 = sp.digest(), sp2.digest()
    assert d1["entries"] > 0
    for key in ("entries", "count_sum", "dir_sum", "hash_sum", "hash_xor"):
        assert d1[key] == d2[key], key
    assert abs(d1["weighted_sum"] - d2["weighted_sum"]) <= 1e-6 * abs(d2["weighted_sum"])
    # the output of the main batch: no original of a duplicated pair
    filt = {"action": (res.discarded * 2).astype(np.uint8), "min_pass": np.zeros(rs.n, np.uint32), "max_pass": np.zeros(rs.n, np.uint32)}
    main = ka.ReadSelector(sp, rs, mate=pairs.mate, filter_results=filt).filterReads(min_score=0.0, min_read_length=0.0)
    main_names = {l.split(b" ")[0][1:].decode() for l in main.split(b"\n")[0::4] if l}
    gone = {name for (name, _, _), d in zip(reads, want.discarded) if d}
    assert len(gone) == want.affected and not (main_names & gone)
    assert main_names <= {n for n, _, _ in reads}
    # the output of the consensus batch: byte for byte what the same selection writes of refdedup's records
    cons = ka.ReadSelector(sp, res.consensus, mate=cmate).filterReads(min_score=0.0, min_read_length=0.0)
    ref_sel = ka.ReadSelector(sp, ref_cons, mate=cmate)
    ref_text = ref_sel.filterReads(min_score=0.0, min_read_length=0.0)
    assert cons == ref_text
    # which records that is: with minimum score 0 and minimum length 0 a read passes when more than one base of it survives the trim
    # (passesLength, src/ReadSelector.h:219-228) and a pair is written when either end passes
    to, tl, score, trimmed = sp.scoreAndTrimReadSet(ref_cons, 0.0)
    passing = np.asarray(tl) > 1
    present = [n for (n, _, _), p in zip(want.consensus, passing | passing[cmate]) if p]
    lines = cons.decode().split("\n")
    assert [l.split(" ")[0][1:] for l in lines[0:len(lines) - 1:4]] == present and len(present) > len(want.consensus) // 2
    # ... each with the bases and qualities of refdedup's record inside its trim
    by_name = {n: (b, q) for n, b, q in want.consensus}
    index = {n: i for i, (n, _, _) in enumerate(want.consensus)}
    for at in range(0, len(lines) - 1, 4):
        name = lines[at].split(" ")[0][1:]
        i = index[name]
        b, q = by_name[name]
        if int(tl[i]) > 1:
            assert lines[at + 1] == b[int(to[i]):int(to[i]) + int(tl[i])] and lines[at + 3] == q[int(to[i]):int(to[i]) + int(tl[i])], name
    res.close()
