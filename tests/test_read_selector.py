"""selectReads / writePicks on the device (kmr_select_reads, kmr_filter_read_batch; kmernator_amd/csrc/kmr_select.hpp): the
picks and every byte of FilterReads' output against the reference's goldens (test/runFilterTests.sh) and against the CPU
restatement of tests/refsemantics.py, which is pinned to those goldens."""
import ctypes as C
import os

import numpy as np
import pytest

import kmernator_amd as ka
from kmernator_amd import _lib
from helpers import GOLDEN, OracleSpectrum, ReadBatch, default_config, oracle_weighted_kmers, synth_reads
from refsemantics import filterreads_output, passes_length, score_and_trim

K = 31
LABEL = {"SUM": b"Score", "MEDIAN": b"MedianScore", "MIN": b"MinScore", "MAX": b"MaxScore", "AVG": b"AvgScore"}
NEW_SYMBOLS = ["kmr_select_config_init", "kmr_select_reads", "kmr_select_reads_dev", "kmr_filter_read_batch", "kmr_filter_read_batch_dev",
               "kmr_picks_info", "kmr_picks_copy", "kmr_picks_device_ptr", "kmr_picks_free"]


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


# ---------------------------------------------------------------- CPU: the ABI without a device

def _select_config(**kw):
    c = ka.KmrSelectConfig()
    assert ka.load().kmr_select_config_init(C.byref(c)) == 0
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def test_new_symbols_are_exported():
    lib = ka.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.kmr_abi_version() == 1


def test_select_config_defaults_and_size():
    """the reference's defaults: --min-depth 2, --min-read-length 0.40, --min-passing-in-pair 1 (src/ReadSelector.h:72),
    --fastq-output-base-quality 33, FASTQ, median score"""
    c = _select_config()
    assert c.struct_size == C.sizeof(ka.KmrSelectConfig) == 32
    assert (c.minimum_score, c.both_pass, c.output_quality_base, c.format, c.scoring_type) == (2.0, 0, 33, 0, 1)
    assert c.min_read_length == float(np.float32(0.40))
    assert ka.load().kmr_select_config_init(None) == -1


@pytest.mark.parametrize("entry", ["kmr_select_reads", "kmr_select_reads_dev", "kmr_filter_read_batch", "kmr_filter_read_batch_dev"])
def test_bad_config_and_null_handle_are_refused(entry):
    """the configuration is checked before anything else, so the refusal and its reason can be seen without a device
    (kmr_last_error(NULL) holds the text of a failure that has no handle)"""
    lib = ka.load()
    fn = getattr(lib, entry)
    fused = "filter" in entry

    def call(cfg):
        out = C.c_void_p(1)
        args = [None, None, None, 0, None, None, None, None] + ([] if fused else [None, None, None, None]) + [C.byref(cfg) if cfg is not None else None, C.byref(out)]
        rc = fn(*args)
        assert out.value is None          # *out is cleared on every failure
        return rc, lib.kmr_last_error(None).decode()
    for bad, why in ((dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(format=2), "format"),
                     (dict(output_quality_base=0), "output_quality_base"), (dict(output_quality_base=48), "output_quality_base"), (dict(scoring_type=5), "scoring_type")):
        rc, text = call(_select_config(**bad))
        assert rc == -1 and why in text, (bad, rc, text)
    rc, text = call(None)
    assert rc == -1 and "NULL" in text
    rc, text = call(_select_config())
    assert rc == -1 and "NULL handle" in text and entry in text
    assert lib.kmr_picks_info(None, None, None) == -1 and lib.kmr_picks_copy(None, None, 0, None) == -1 and lib.kmr_picks_device_ptr(None, None) == -1
    lib.kmr_picks_free(None)


# ---------------------------------------------------------------- the restatement for any pairing (one read at a time)

def record_text(name, seq, qual, label, discarded, to, tl, shift, out_base, fasta):
    """Read::toFastq / toFasta (src/Sequence.cpp:761-779) of one read"""
    tl = 0 if discarded else min(int(tl), max(0, len(seq) - int(to)))
    if discarded or tl <= 1:
        s, q = b"N", bytes([out_base + 1])
    else:
        s = seq[int(to):int(to) + tl]
        q = bytes((c + shift) & 0xff for c in qual[int(to):int(to) + tl])
    head = name + ((b" " + label) if label else b"")
    return (b">" + head + b"\n" + s + b"\n") if fasta else (b"@" + head + b"\n" + s + b"\n+\n" + q + b"\n")


def expected_selection(names, seqs, quals, labels, disc, to, tl, sc, mate, min_score, mrl, both, shift=0, out_base=33, fasta=False):
    """pickAllPassingReads (mate None) / pickAllPassingPairs over any pairing (src/ReadSelector.h:547-596), picks in ascending
    read index (optimizePickOrder), then writePicks: (text, picked flags)"""
    n = len(names)
    mrl = float(np.float32(mrl))
    passing = [(not disc[i]) and bool(sc[i] >= min_score) and passes_length(float(tl[i]), len(seqs[i]), mrl) for i in range(n)]
    picked = np.zeros(n, dtype=bool)
    out = []
    for i in range(n):
        j = -1 if mate is None else int(mate[i])
        picked[i] = passing[i] if j < 0 else ((passing[i] and passing[j]) if both else (passing[i] or passing[j]))
        if picked[i]:
            out.append(record_text(names[i], seqs[i], quals[i], labels[i], disc[i], to[i], tl[i], shift, out_base, fasta))
    return b"".join(out), picked


def trim_labels(n, action, min_pass, max_pass, to, tl, sc, wt, scoring):
    """the labels FilterKnownOddities and setTrimHeaders (src/ReadSelector.h:1015-1036) leave on each read"""
    labels = []
    for i in range(n):
        parts = []
        if action is not None and action[i] == 2:
            labels.append(b"")
            continue
        if action is not None and action[i] == 1:
            parts.append(b"AFTrim:%d+%d" % (min_pass[i], max_pass[i] - min_pass[i]))
        if wt[i]:
            parts.append(b"Trim:%d+%d" % (to[i], tl[i]))
        parts.append(LABEL[scoring] + b":%d" % int(float(sc[i]) + 0.5))
        labels.append(b" ".join(parts))
    return labels


def host_reads(read_set):
    b, q, off, names = read_set.arrays()
    seqs = [bytes(b[int(off[i]):int(off[i + 1])]) for i in range(read_set.n)]
    quals = [bytes(q[int(off[i]):int(off[i + 1])]) for i in range(read_set.n)]
    return [nm.split(b" ")[0].split(b"\t")[0] for nm in names], seqs, quals


def fastq_text(rb, names):
    return b"".join(b"@" + names[i] + b"\n" + rb.seq(i) + b"\n+\n" + rb.qual(i) + b"\n" for i in range(rb.n))


def both_routes(sel, min_score, mrl, both, scoring, out_base, fmt, select_min_score=None):
    """the text and the pick flags through kmr_filter_read_batch and through kmr_select_reads on host arrays"""
    fused = sel.filterReads(min_score, mrl, both, scoring, out_base, fmt)
    fused_flags = sel.picked_flags.copy()
    assert sel.bytes == len(fused) and sel.n_picked == int(fused_flags.sum())
    sel.scoreAndTrimReads(min_score, scoring)
    sel.pickAllPassingPairs(min_score if select_min_score is None else select_min_score, mrl, both)
    text = sel.writePicks(out_base, fmt)
    return fused, fused_flags, text, sel.picked_flags.copy()


# ---------------------------------------------------------------- GPU 1: the reference's goldens, whole file

@pytest.mark.gpu
@pytest.mark.parametrize("gold_name,mrl,both,out_base", [
    ("1000-Filtered-0.85.fastq", 0.85, False, 64), ("1000-Filtered-0.85.std.fastq", 0.85, False, 33),
    ("1000-Filtered-readlength.fastq", 1.0, False, 64), ("1000-Filtered-readlength-both.fastq", 1.0, True, 64), ("1000-Filtered.fastq", 25.0, False, 64)])
@pytest.mark.parametrize("fq", ["1000.fastq", "1000.std.fastq"])
def test_filterreads_goldens_written_by_the_device(fq, gold_name, mrl, both, out_base):
    """test/runFilterTests.sh:43-63, every golden, WHOLE FILE: ingest, artifact filter, spectrum, scoreAndTrimReads, selection and
    the output text all on the device; nothing is formatted on the host"""
    gold = golden(gold_name)
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, golden(fq))
    assert rs.input_quality_base == (33 if "std" in fq else 64)
    f = ka.FilterKnownOddities(sp, golden("artifact_sequences.fa"), edit_distance=1, min_read_length=mrl)
    res, frs = f.applyFilter(rs)
    assert frs.n == 1000
    sp.buildKmerSpectrumFromReadSet(frs)
    sp.finalize(2)
    sel = ka.ReadSelector(sp, frs, mate=np.arange(1000, dtype=np.int64) ^ 1, filter_results=res)
    fused, fused_flags, text, flags = both_routes(sel, 2, mrl, both, "MEDIAN", out_base, "fastq")
    want = gold.replace(b"\t", b" ")
    print("golden %s from %s: %d bytes wanted, fused %d, select %d, picks %d" % (gold_name, fq, len(want), len(fused), len(text), sel.n_picked))
    assert fused.replace(b"\t", b" ") == want
    assert text.replace(b"\t", b" ") == want
    assert np.array_equal(fused_flags, flags) and int(flags.sum()) == gold.count(b"\n") // 4
    assert np.array_equal(sel.picks, np.nonzero(flags)[0])
    assert int((res["action"] == 2).sum()) == {0.85: 5, 1.0: 51, 25.0: 0}[mrl]


# ---------------------------------------------------------------- GPU 2: against the restatement at size

N_SIZE = 200_000


def size_reads():
    """200 000 x 150 bp: half from a genome read 30 times over, half from one read 0.3 times over (most of whose k-mers are seen once
    and fall to min depth 2), 1 % substitutions, noisy qualities, N at 0.2 % of the bases, shuffled so that the pairs (2i, 2i + 1)
    mix both kinds; names of 3 to 30 characters, some with a comment behind a blank or a tab"""
    half = N_SIZE // 2
    a = synth_reads(half, read_len=150, genome_len=half * 150 // 30, seed=11, err=0.01, quality="noisy", n_rate=0.002)
    b = synth_reads(half, read_len=150, genome_len=half * 150 * 10 // 3, seed=12, err=0.01, quality="noisy", n_rate=0.002)
    perm = np.random.default_rng(13).permutation(N_SIZE)
    bases = np.concatenate([a.bases, b.bases]).reshape(N_SIZE, 150)[perm].reshape(-1)
    quals = np.concatenate([a.quals, b.quals]).reshape(N_SIZE, 150)[perm].reshape(-1)
    rb = ReadBatch.from_arrays(np.ascontiguousarray(bases), np.ascontiguousarray(quals), np.arange(N_SIZE + 1, dtype=np.uint64) * np.uint64(150))
    names = []
    for i in range(N_SIZE):
        nm = b"r%d" % i if i % 4 == 0 else (b"lane%d:tile%d:%d" % (i % 8, i % 1201, i * 7919 % 1000003) if i % 4 == 1 else b"HWI-ST%d_%d#%d/%d" % (i % 97, i, i % 13, 1 + (i & 1)))
        names.append(nm + (b" 1:N:0:ATCACG" if i % 3 == 0 else (b"\tlength=150" if i % 7 == 0 else b"")))
    return rb, names


def test_size_case_has_every_kind_of_read_on_the_oracle():
    """the choice of genomes, error and N rates checked on the CPU: the oracle spectrum of all 200 000 reads and
    scoreAndTrimReads' restatement over the first 3000 pairs give passing and failing reads, trimmed and untrimmed ones, reads with
    nothing left beside a passing mate, and pairs with exactly one passing read"""
    rb, _ = size_reads()
    cfg = default_config(K, estimated_raw_kmers=N_SIZE * (150 - K + 1))
    o = OracleSpectrum(cfg)
    o.add_reads(rb, threads=8)
    o.finalize(2)
    n = 6000
    tl, sc, wt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for i in range(n):
        keys, _, _ = oracle_weighted_kmers(cfg, rb.seq(i), rb.qual(i))
        _, tl[i], sc[i], wt[i] = score_and_trim(o.lookup(keys), rb.seq(i), K, 2, "MEDIAN")
    for mrl in (0.5, 100.0):
        p = np.array([sc[i] >= 2 and passes_length(tl[i], 150, mrl) for i in range(n)])
        one = p[0::2] ^ p[1::2]
        empty_mate = ((tl[0::2] <= 1) & p[1::2]) | ((tl[1::2] <= 1) & p[0::2])
        print("min length %s: %d of %d pass, %d trimmed, %d pairs with one passing read, %d of them with nothing left of the other" % (mrl, p.sum(), n, wt.sum(), one.sum(), empty_mate.sum()))
        assert 500 < p.sum() < n - 500 and 500 < wt.sum() < n - 500 and one.sum() > 200 and empty_mate.sum() > 50


@pytest.fixture(scope="module")
def size_case():
    rb, names = size_reads()
    text = fastq_text(rb, names)
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=N_SIZE * (150 - K + 1), device=0))
    rs = ka.ReadSet(sp, text, input_quality_base=33)
    assert rs.n == N_SIZE
    sp.buildKmerSpectrumFromReadSet(rs)
    sp.finalize(2)
    short, seqs, quals = host_reads(rs)
    assert short == [nm.split(b" ")[0].split(b"\t")[0] for nm in names]
    yield sp, rs, short, seqs, quals
    rs.close()
    sp.close()


def fastq_to_fasta(text):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("both,mrl,out_base,scoring,fmt", [
    (0, 0.5, 33, "MEDIAN", "fastq"), (1, 0.5, 64, "MEDIAN", "fastq"), (0, 100.0, 64, "AVG", "fastq"), (1, 60.0, 33, "MIN", "fastq"),
    (0, 0.5, 33, "MAX", "fasta"), (1, 100.0, 33, "AVG", "fasta"), (0, 0.5, 33, "SUM", "fastq"), (1, 0.5, 33, "SUM", "fastq")])
def test_selection_and_text_match_the_restatement_at_size(size_case, both, mrl, out_base, scoring, fmt):
    """200 000 reads: the device's text and pick flags against filterreads_output fed from kmr_score_read_batch + kmr_reads_copy;
    every read is compared.  The sum score stays 0 as in the reference (scoreReadBySumKmer only assigns it when byAvg), so with
    --min-depth 2 as the read threshold nothing passes: that is what the fused route must give for SUM, and the host-array route
    selects with a read threshold of 0 there"""
    sp, rs, names, seqs, quals = size_case
    n = rs.n
    sel_min = 0.0 if scoring == "SUM" else 2.0
    to, tl, sc, wt = sp.scoreAndTrimReadSet(rs, 2, scoring)
    labels = trim_labels(n, None, None, None, to, tl, sc, wt, scoring)
    disc = [False] * n
    mrl32 = float(np.float32(mrl))

    def expect(min_score):
        text = filterreads_output(names, seqs, quals, labels, disc, to, tl, sc, min_score, mrl32, both, qual_shift=out_base - 33, out_base=out_base)
        p = np.array([bool(sc[i] >= min_score) and passes_length(float(tl[i]), 150, mrl32) for i in range(n)])
        pair = (p[0::2] & p[1::2]) if both else (p[0::2] | p[1::2])
        return (fastq_to_fasta(text) if fmt == "fasta" else text), p, np.repeat(pair, 2)
    want, p, want_flags = expect(sel_min)
    # the case holds what it is meant to test (judged on the expected side alone)
    n_mask = int((want_flags & (tl <= 1)).sum())
    dropped_one = int(((p[0::2] ^ p[1::2]) & ~want_flags[0::2]).sum())
    print("both %d mrl %s base %d %s %s: %d of %d picked, %d bytes, %d trimmed, %d printed as N, %d pairs dropped with one passing read" % (
        both, mrl, out_base, scoring, fmt, want_flags.sum(), n, len(want), int(wt.sum()), n_mask, dropped_one))
    assert 1000 < want_flags.sum() < n - 1000
    assert 1000 < wt.sum() < n - 1000 and (want_flags & wt).sum() > 1000 and (want_flags & ~wt).sum() > 1000
    if both:
        assert dropped_one > 1000 and n_mask == 0
    else:
        assert n_mask > 1000 and want.count(b"\nN\n") >= n_mask
    sel = ka.ReadSelector(sp, rs, mate=np.arange(n, dtype=np.int64) ^ 1)
    fused, fused_flags, text, flags = both_routes(sel, 2.0, mrl, both, scoring, out_base, fmt, select_min_score=sel_min)
    assert len(text) == len(want) and text == want
    assert np.array_equal(flags, want_flags)
    if scoring == "SUM":
        want, _, want_flags = expect(2.0)
        assert want == b"" and not want_flags.any()
    assert fused == want and np.array_equal(fused_flags, want_flags)
    sel.close()


# ---------------------------------------------------------------- GPU 3: singles, odd pairings, artifact-filter results

@pytest.fixture(scope="module")
def filtered_case():
    """6000 reads of mixed depth through the artifact filter's quality screen (Q2 bases and N's cut reads: AFTrim labels, discards,
    remnants appended as extra reads), then the spectrum of what is left"""
    n = 6000
    a = synth_reads(n // 2, read_len=150, genome_len=n // 2 * 150 // 25, seed=21, err=0.01, quality="noisy", n_rate=0.003)
    b = synth_reads(n // 2, read_len=150, genome_len=n // 2 * 150 * 4, seed=22, err=0.01, quality="noisy", n_rate=0.003)
    perm = np.random.default_rng(23).permutation(n)
    rb = ReadBatch.from_arrays(np.ascontiguousarray(np.concatenate([a.bases, b.bases]).reshape(n, 150)[perm].reshape(-1)),
                               np.ascontiguousarray(np.concatenate([a.quals, b.quals]).reshape(n, 150)[perm].reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(150))
    names = [b"q%d" % (i * i) + (b" 2:N:0:GG" if i % 2 else b"") for i in range(n)]
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=n * 120, device=0))
    rs = ka.ReadSet(sp, fastq_text(rb, names), input_quality_base=33)
    f = ka.FilterKnownOddities(sp, golden("artifact_sequences.fa"), edit_distance=1, min_read_length=0.4)
    res, frs = f.applyFilter(rs)
    assert frs.n > n and (res["action"] == 1).sum() > 100 and (res["action"] == 2).sum() > 20
    sp.buildKmerSpectrumFromReadSet(frs)
    sp.finalize(2)
    mate = np.full(frs.n, -1, dtype=np.int64)       # of every five reads: (0, 3) and (1, 4) are pairs, 2 is single; the remnants are single
    for b0 in range(0, n - 4, 5):
        mate[b0], mate[b0 + 3], mate[b0 + 1], mate[b0 + 4] = b0 + 3, b0, b0 + 4, b0 + 1
    action = np.zeros(frs.n, dtype=np.uint8); lo = np.zeros(frs.n, dtype=np.uint32); hi = np.zeros(frs.n, dtype=np.uint32)
    action[:n], lo[:n], hi[:n] = res["action"], res["min_pass"], res["max_pass"]
    yield sp, frs, res, mate, (action, lo, hi), host_reads(frs)
    frs.close(); rs.close(); f.close(); sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired,both,fmt,out_base", [(False, 0, "fastq", 33), (True, 0, "fastq", 64), (True, 1, "fastq", 33), (True, 0, "fasta", 33)])
def test_singles_odd_pairings_and_artifact_labels(filtered_case, paired, both, fmt, out_base):
    """mate None (pickAllPassingReads); singles between pairs that are not adjacent; the artifact filter's remnants as singles; AFTrim
    labels; discarded reads printed as a label-less N beside a passing mate"""
    sp, frs, res, mate, (action, lo, hi), (names, seqs, quals) = filtered_case
    n = frs.n
    to, tl, sc, wt = sp.scoreAndTrimReadSet(frs, 2, "MEDIAN")
    labels = trim_labels(n, action, lo, hi, to, tl, sc, wt, "MEDIAN")
    disc = list(action == 2)
    m = mate if paired else None
    want, want_flags = expected_selection(names, seqs, quals, labels, disc, to, tl, sc, m, 2, 0.5, both, out_base - 33, out_base, fmt == "fasta")
    n_af = int((want_flags & (action == 1)).sum())
    n_disc = int((want_flags & (action == 2)).sum())
    print("paired %s both %d %s: %d of %d picked (%d remnants), %d with AFTrim, %d discarded reads printed" % (
        paired, both, fmt, want_flags.sum(), n, want_flags[res["action"].size:].sum(), n_af, n_disc))
    assert 500 < want_flags.sum() < n - 500 and n_af > 20 and want.count(b" AFTrim:") == n_af
    assert want_flags[res["action"].size:].any()                      # remnants among the picks
    if paired and not both:
        assert n_disc > 3 and (b"\nN\n" in want)
    else:
        assert n_disc == 0
    sel = ka.ReadSelector(sp, frs, mate=m, filter_results=res)
    fused, fused_flags, text, flags = both_routes(sel, 2.0, 0.5, both, "MEDIAN", out_base, fmt)
    assert text == want and fused == want
    assert np.array_equal(flags, want_flags) and np.array_equal(fused_flags, want_flags)
    if paired:         # pickAllPassingReads ignores the pairing
        sel.pickAllPassingReads(2.0, 0.5)
        w1, f1 = expected_selection(names, seqs, quals, labels, disc, to, tl, sc, None, 2, 0.5, 0)
        assert sel.writePicks() == w1 and np.array_equal(sel.picked_flags, f1)
    sel.close()


@pytest.mark.gpu
def test_text_in_device_memory(filtered_case):
    """the _dev forms take the FASTQ text as a device pointer and give the same bytes"""
    import torch
    sp, frs, res, mate, (action, lo, hi), _ = filtered_case
    lib = sp.lib
    sel = ka.ReadSelector(sp, frs, mate=mate, filter_results=res)
    want = sel.filterReads(2.0, 0.5, False)
    dtext = torch.frombuffer(bytearray(frs.text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    cfg = _select_config(min_read_length=0.5)
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    to, tl, sc, wt = sp.scoreAndTrimReadSet(frs, 2, "MEDIAN")
    wt8 = wt.astype(np.uint8)
    for fused in (True, False):
        out = C.c_void_p()
        head = [sp.h, frs.r, dtext.data_ptr(), dtext.numel(), mate.ctypes.data_as(C.POINTER(C.c_int64)), action.ctypes.data_as(u8), lo.ctypes.data_as(u32), hi.ctypes.data_as(u32)]
        if fused:
            rc = lib.kmr_filter_read_batch_dev(*head, C.byref(cfg), C.byref(out))
        else:
            rc = lib.kmr_select_reads_dev(*head, to.ctypes.data_as(u32), tl.ctypes.data_as(u32), sc.ctypes.data_as(C.POINTER(C.c_float)), wt8.ctypes.data_as(u8), C.byref(cfg), C.byref(out))
        assert rc == 0, lib.kmr_last_error(sp.h)
        npk, nb = C.c_uint64(), C.c_uint64()
        assert lib.kmr_picks_info(out, C.byref(npk), C.byref(nb)) == 0 and nb.value == len(want)
        buf = np.zeros(nb.value, dtype=np.uint8)
        assert lib.kmr_picks_copy(out, buf.ctypes.data_as(C.c_void_p), nb.value, None) == 0
        dp = C.c_void_p()
        assert lib.kmr_picks_device_ptr(out, C.byref(dp)) == 0 and dp.value
        lib.kmr_picks_free(out)
        assert buf.tobytes() == want
    sel.close()


# ---------------------------------------------------------------- GPU 4: edges

def _live(sp):
    return int(sp.build_info("device_blocks_live"))


@pytest.mark.gpu
def test_edges_of_the_selection():
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=100000, device=0))
    lib = sp.lib
    rng = np.random.default_rng(5)
    seq = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 80)])
    seq3 = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 60)])
    rec1, rec3 = b"one MedianScore:2\n" + seq + b"\n+\n" + b"I" * 80 + b"\n", b"three MedianScore:2\n" + seq3 + b"\n+\n" + b"5" * 60 + b"\n"
    text = b"@one extra\n" + seq + b"\n+\n" + b"I" * 80 + b"\n@two\nA\n+\nI\n@three\n" + seq3 + b"\n+\n" + b"5" * 60 + b"\n"
    rs = ka.ReadSet(sp, text, input_quality_base=33)
    assert rs.n == 3
    sel = ka.ReadSelector(sp, rs, mate=np.array([1, 0, -1], dtype=np.int64))
    # the fused entry before kmr_finalize
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
        sel.filterReads(2.0, 0.5)
    sp.buildKmerSpectrumFromReadSet(rs)
    sp.buildKmerSpectrumFromReadSet(rs)          # every k-mer twice: depth 2
    sp.finalize(2)
    # a read of length 1 never passes (passesLength: length <= 1) and prints as N beside its passing mate
    assert sel.filterReads(2.0, 0.5, False) == b"@" + rec1 + b"@two MedianScore:0\nN\n+\n\"\n@" + rec3
    assert list(sel.picks) == [0, 1, 2]
    assert sel.filterReads(2.0, 0.5, True) == b"@" + rec3
    assert sel.filterReads(2.0, 70.0, False, output_quality_base=64, format="fasta") == b">one MedianScore:2\n" + seq + b"\n>two MedianScore:0\nN\n"
    assert sel.filterReads(2.0, 0.5, False, output_quality_base=64) == b"@one MedianScore:2\n" + seq + b"\n+\n" + b"h" * 80 + b"\n@two MedianScore:0\nN\n+\nA\n@three MedianScore:2\n" + seq3 + b"\n+\n" + b"T" * 60 + b"\n"
    # nothing passes: zero picks, zero bytes
    assert sel.filterReads(1e9, 0.5) == b"" and sel.n_picked == 0 and sel.bytes == 0 and not sel.picked_flags.any()
    # everything passes
    text2 = text.replace(b"@two\nA\n+\nI\n", b"")
    rs2 = ka.ReadSet(sp, text2, input_quality_base=33)
    sel2 = ka.ReadSelector(sp, rs2)
    assert sel2.filterReads(2.0, 0.0) == b"@" + rec1 + b"@" + rec3 and sel2.n_picked == rs2.n == 2 and sel2.picked_flags.all()
    sel2.close()
    rs2.close()
    # host arrays of the caller's own: the label follows them
    sel.trims = (np.array([3, 0, 0], np.uint32), np.array([40, 1, 60], np.uint32), np.full(3, 7.4, np.float32), np.array([1, 0, 0], np.uint8))
    assert sel.pickAllPassingPairs(0.0, 0.0) == 3
    assert sel.writePicks() == b"@one Trim:3+40 MedianScore:7\n" + seq[3:43] + b"\n+\n" + b"I" * 40 + b"\n@two MedianScore:7\nN\n+\n\"\n@three MedianScore:7\n" + seq3 + b"\n+\n" + b"5" * 60 + b"\n"
    # a short buffer
    buf = np.zeros(sel.bytes, dtype=np.uint8)
    assert lib.kmr_picks_copy(sel._picks, buf.ctypes.data_as(C.c_void_p), sel.bytes - 1, None) == -6
    assert lib.kmr_picks_copy(sel._picks, buf.ctypes.data_as(C.c_void_p), sel.bytes, None) == 0
    # arguments: a mate outside the batch, a text that does not hold the names, af arrays not all there, a bad configuration
    sel.mate = np.array([7, 0, -1], dtype=np.int64)
    with pytest.raises(ka.KmerSpectrumError, match="mate"):
        sel.pickAllPassingPairs(0.0, 0.0)
    sel.mate = None
    rs.text = rs.text[:20]
    with pytest.raises(ka.KmerSpectrumError, match="name"):
        sel.pickAllPassingReads(0.0, 0.0)
    rs.text = text
    cfg = _select_config(output_quality_base=50)
    out = C.c_void_p()
    assert lib.kmr_filter_read_batch(sp.h, rs.r, text, len(text), None, None, None, None, C.byref(cfg), C.byref(out)) == -1
    assert b"output_quality_base" in lib.kmr_last_error(sp.h)
    one = np.zeros(3, np.uint8)
    cfg = _select_config()
    assert lib.kmr_filter_read_batch(sp.h, rs.r, text, len(text), None, one.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, C.byref(cfg), C.byref(out)) == -1
    sel.close()
    # an empty batch
    empty = ka.ReadSet(sp, b"")
    sel = ka.ReadSelector(sp, empty)
    assert sel.filterReads(2.0, 0.5) == b"" and sel.n_picked == 0 and sel.picks.size == 0
    sel.scoreAndTrimReads(2.0)
    assert sel.pickAllPassingReads(2.0, 0.5) == 0 and sel.writePicks() == b""
    sel.close()
    sp.close()


@pytest.mark.gpu
def test_picks_give_every_block_back(filtered_case):
    """device_blocks_live returns to where it was once the picks are freed, also after a call that failed behind its allocations"""
    sp, frs, res, mate, _, _ = filtered_case
    sel = ka.ReadSelector(sp, frs, mate=mate, filter_results=res)
    sel.filterReads(2.0, 0.5)            # the handle's grow-only scoring buffers exist from here on
    sel.close()
    base = _live(sp)
    sel = ka.ReadSelector(sp, frs, mate=mate, filter_results=res)
    assert len(sel.filterReads(2.0, 0.5)) > 0
    assert _live(sp) == base + 2         # the text and the flags
    sel.scoreAndTrimReads(2.0)
    sel.pickAllPassingPairs(2.0, 0.5, True)
    assert _live(sp) == base + 2         # the earlier picks were freed
    sel.close()
    assert _live(sp) == base
    bad = mate.copy()
    bad[0] = frs.n + 5
    sel = ka.ReadSelector(sp, frs, mate=bad, filter_results=res)
    for _ in range(2):
        with pytest.raises(ka.KmerSpectrumError):
            sel.filterReads(2.0, 0.5)
        assert _live(sp) == base
    sel.close()


# ---------------------------------------------------------------- the C++ host side (include/kmernator_amd.hpp: ReadSelector)

def _build_select_demo(tmp_path):
    import subprocess
    from helpers import ROOT
    exe = str(tmp_path / "select_demo")
    lib_dir = os.path.join(ROOT, "kmernator_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "select_demo.cpp"), "-L" + lib_dir, "-lkmernator_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_read_selector_compiles_and_links(tmp_path):
    """the C++ ReadSelector against the library, warnings as errors (it runs in the GPU test below)"""
    assert os.path.exists(_build_select_demo(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("gold_name,mrl,both,out_base", [("1000-Filtered-readlength-both.fastq", "1.0", 1, 64), ("1000-Filtered-0.85.std.fastq", "0.85", 0, 33)])
def test_cpp_read_selector_writes_the_goldens(tmp_path, gold_name, mrl, both, out_base):
    """tests/cpp/select_demo.cpp: artifact filter, spectrum and ReadSelector through the C++ classes; the selector is handed the
    filter's results and the mates of the INPUT reads and extends them itself.  Whole file, both routes"""
    import subprocess
    exe = _build_select_demo(tmp_path)
    out = str(tmp_path / "picks")
    p = subprocess.run([exe, os.path.join(GOLDEN, "1000.fastq"), os.path.join(GOLDEN, "artifact_sequences.fa"), out, mrl, str(both), str(out_base)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    want = golden(gold_name).replace(b"\t", b" ")
    n = want.count(b"\n") // 4
    assert p.stdout.split() == ["reads", "1000", "picks", str(n), str(n), "flagged", str(n)]
    assert open(out + ".fused", "rb").read().replace(b"\t", b" ") == want
    assert open(out + ".select", "rb").read().replace(b"\t", b" ") == want
