"""Coverage normalization on the device (kmr_normalize_reads, kmr_normalize_read_batch; kmernator_amd/csrc/kmr_normalize.hpp):
selectReads with --max-kmer-output-depth, RANDOM.  Text, flags, segment table and kmr_normalize_info against the CPU restatement
of tests/refnormalize.py, byte for byte, over the directed batches of tests/normalizecases.py."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import kmernator_amd as ka
import normalizecases as nc
from helpers import GOLDEN
from refnormalize import Normalizer, file_name, pair_list

pytestmark = pytest.mark.gpu
K = 31


@pytest.fixture(scope="module")
def sp():
    s = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=100000, device=0))
    yield s
    s.close()


class Dev:
    """a Batch on the device: its ReadSet and a ReadSelector that holds the made-up results of the earlier stages"""

    def __init__(self, sp, b):
        self.sp, self.b = sp, b
        self.rs = ka.ReadSet(sp, b.fastq(), input_quality_base=33)
        assert self.rs.n == b.n
        self.sel = ka.ReadSelector(sp, self.rs, pairs=None if b.read1 is None else (b.read1, b.read2), filter_results=dict(action=b.action, min_pass=b.lo, max_pass=b.hi))
        self.sel.trims = (b.to, b.tl, b.sc, b.wt)

    def run(self, out_base=33, fmt="fastq", **override):
        """the array form through the Python layer; returns what compare() takes"""
        c = dict(self.b.cfg, **override)
        got = self.sel.selectReads(c["min_score"], 0, -1.0, c["min_read_length"], c["both_pass"], "MEDIAN", out_base, fmt, self.b.input_starts, separate_outputs=False,
                                   max_kmer_output_depth=c["target_depth"], seed=c["seed"], first_read_idx=c["first_read_idx"], by_pair=c["by_pair"])
        return self.result(got[0][1])

    def result(self, text):
        s = self.sel
        seg = s.segments
        assert seg["picks"].shape[0] == 1 and not seg["round_is_remainder"][0]
        table = [tuple(int(seg[k][0, j]) for k in ("first_pick", "picks", "first_byte", "bytes")) for j in range(seg["picks"].shape[1])]
        return dict(text=text, table=table, read_segment=s.read_segment.copy(), info=dict(s.normalize_info), flags=s.picked_flags.copy(), n_picked=s.n_picked,
                    depth=float(seg["round_depth"][0]))

    def close(self):
        self.sel.close()
        self.rs.close()


def compare(got, want, what=""):
    print("%s: %d records in %d picks of %d candidates, %d draws, %d bytes, per input %s" % (what, len(want["reads"]), want["info"]["n_picks"], want["info"]["n_candidates"],
                                                                                           want["info"]["n_draws"], len(want["text"]), [t[1] for t in want["table"]]))
    assert got["info"] == want["info"]
    assert got["table"] == want["table"]
    assert np.array_equal(got["read_segment"], want["read_segment"])
    assert np.array_equal(got["flags"], want["read_segment"] >= 0) and got["n_picked"] == len(want["reads"])
    assert len(got["text"]) == len(want["text"]) and got["text"] == want["text"]


# ---------------------------------------------------------------- 1: sizes around a wavefront and a unit

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129])
def test_sizes(sp, n):
    """interleaved pairs over every score class; 64 slots are a unit, so 65 reads are two units and a read, 129 four and a read"""
    b = nc.interleaved(n)
    d = Dev(sp, b)
    try:
        for by_pair in (True, False):
            compare(d.run(by_pair=by_pair), b.expect(by_pair=by_pair), "n %d by_pair %d" % (n, by_pair))
    finally:
        d.close()


# ---------------------------------------------------------------- 2: the directed batches, every format

MAKERS = {
    "blocks": lambda: nc.blocks(70),
    "both_pass_halves": nc.both_pass_halves,
    "boundaries": lambda: nc.single_reads_over(600),
    "truncation": nc.truncation,
    "reversed_pairs": nc.reversed_pairs,
    "by_read_full_pairs": nc.by_read_full_pairs,
    "blocks_both_pass": lambda: nc.blocks(70, both_pass=True),
    "blocks_by_read": lambda: nc.blocks(70, by_pair=False),
}


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_directed_batches(sp, name):
    b = MAKERS[name]()
    d = Dev(sp, b)
    try:
        for fmt, base in (("fastq", 33), ("fastq", 64), ("fasta", 33)):
            want = b.expect(out_base=base, fasta=fmt == "fasta")
            got = d.run(base, fmt)
            compare(got, want, "%s %s/%d" % (name, fmt, base))
            assert got["depth"] == float(np.float32(b.cfg["min_score"]))
        if name == "boundaries":
            assert all(got["flags"][i] for i in b.witness["at_T"]) and not any(got["flags"][i] for i in b.witness["at_T_plus_1"])
        if name == "both_pass_halves":
            assert not any(got["flags"][i] for i in b.witness["halves"]) and got["n_picked"] > 0
    finally:
        d.close()


def test_first_global_read_idx_above_2_32_and_two_seeds(sp):
    """the batch starts at a global index above 2^32 (the second counter word of the draw); the generator has found reads on both
    sides of the boundary there.  Another seed picks another subset."""
    b = nc.single_reads_over(600, first=(1 << 32) + 12345)
    d = Dev(sp, b)
    try:
        got = d.run()
        compare(got, b.expect(), "first 2^32 + 12345")
        assert all(got["flags"][i] for i in b.witness["at_T"]) and not any(got["flags"][i] for i in b.witness["at_T_plus_1"])
        low = d.run(first_read_idx=12345)
        compare(low, b.expect(first_read_idx=12345), "first 12345")
        assert not np.array_equal(low["flags"], got["flags"])
        other = d.run(seed=8)
        compare(other, b.expect(seed=8), "seed 8")
        assert not np.array_equal(other["flags"], got["flags"])
    finally:
        d.close()


# ---------------------------------------------------------------- 3: one batch equals its two halves

def test_a_batch_equals_its_halves(sp):
    b = nc.interleaved(4001)
    cut = 2000
    whole = b.expect()
    d = Dev(sp, b)
    lo, hi = Dev(sp, b.half(0, cut)), Dev(sp, b.half(cut, b.n))
    try:
        got = d.run()
        compare(got, whole, "whole")
        a, c = lo.run(), hi.run()
        assert a["text"] + c["text"] == got["text"]
        assert np.array_equal(np.concatenate([a["flags"], c["flags"]]), got["flags"])
        assert {k: a["info"][k] + c["info"][k] for k in a["info"]} == got["info"]
    finally:
        d.close(); lo.close(); hi.close()


# ---------------------------------------------------------------- 4: many units, many tiles a unit, mates far apart

@pytest.fixture(scope="module")
def many(sp):
    b = nc.blocks(9000, extra=1001, max_len=60)
    d = Dev(sp, b)
    yield d, b.expect()
    d.close()


@pytest.mark.parametrize("units", [0, 5])
def test_many_units_and_tiles(sp, many, units):
    """19 001 reads in an R1 and an R2 block: 594 units of one tile by default, 5 units of 119 tiles with kmr_tune partition_units"""
    d, want = many
    sp.tune(partition_units=units)
    try:
        got = d.run()
    finally:
        sp.tune(partition_units=0)
    assert all(t[1] > 300 for t in want["table"])
    for key in ("info", "table"):
        assert got[key] == want[key]
    assert np.array_equal(got["read_segment"], want["read_segment"])
    for fp, np_, fb, nb in want["table"]:
        assert hashlib.sha1(got["text"][fb:fb + nb]).digest() == hashlib.sha1(want["text"][fb:fb + nb]).digest()
    assert len(got["text"]) == len(want["text"])


# ---------------------------------------------------------------- 5: the C entry points: _dev and the fused form

def _call(sp, name, d, text_ptr, text_len, cfg, trims=True, r1=None, r2=None, starts=None):
    lib, b = sp.lib, d.b
    p = ka.ReadSelector._p
    act, lo, hi = (np.ascontiguousarray(x) for x in (b.action, b.lo, b.hi))
    to, tl, sc, wt = (np.ascontiguousarray(b.to, dtype=np.uint32), np.ascontiguousarray(b.tl, dtype=np.uint32), np.ascontiguousarray(b.sc, dtype=np.float32), np.ascontiguousarray(b.wt, dtype=np.uint8))
    st = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
    out = C.c_void_p()
    args = [sp.h, d.rs.r, text_ptr, text_len, p(r1, C.c_int64), p(r2, C.c_int64), 0 if r1 is None else r1.size, p(act, C.c_uint8), p(lo, C.c_uint32), p(hi, C.c_uint32)]
    if trims:
        args += [p(to, C.c_uint32), p(tl, C.c_uint32), p(sc, C.c_float), p(wt, C.c_uint8)]
    args += [p(st, C.c_uint64), 0 if st is None else st.size - 1, C.byref(cfg), C.byref(out)]
    rc = getattr(lib, name)(*args)
    return rc, out


def _config(sp, b, **override):
    c = dict(b.cfg, **override)
    cfg = ka.KmrNormalizeConfig()
    assert sp.lib.kmr_normalize_config_init(C.byref(cfg)) == 0 and cfg.struct_size == C.sizeof(cfg) and cfg.method == 0 and cfg.target_depth == 0
    cfg.select.minimum_score, cfg.select.min_read_length, cfg.select.both_pass = c["min_score"], c["min_read_length"], int(c["both_pass"])
    cfg.target_depth, cfg.seed, cfg.first_global_read_idx, cfg.by_pair = c["target_depth"], c["seed"], c["first_read_idx"], int(c["by_pair"])
    return cfg


def _picks_text(lib, out):
    n, nb = C.c_uint64(), C.c_uint64()
    assert lib.kmr_picks_info(out, C.byref(n), C.byref(nb)) == 0
    buf = np.zeros(max(1, nb.value), dtype=np.uint8)
    assert lib.kmr_picks_copy(out, buf.ctypes.data_as(C.c_void_p), nb.value, None) == 0
    v = [C.c_uint64() for _ in range(3)]
    assert lib.kmr_normalize_info(out, *[C.byref(x) for x in v]) == 0
    return buf[:nb.value].tobytes(), n.value, dict(zip(("n_picks", "n_candidates", "n_draws"), (x.value for x in v)))


def test_dev_form_takes_the_text_on_the_device(sp):
    import torch
    b = nc.blocks(70)
    d = Dev(sp, b)
    try:
        want = b.expect()
        dtext = torch.frombuffer(bytearray(d.rs.text), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        rc, out = _call(sp, "kmr_normalize_reads_dev", d, dtext.data_ptr(), dtext.numel(), _config(sp, b), r1=b.read1, r2=b.read2, starts=b.input_starts)
        assert rc == 0, sp.lib.kmr_last_error(sp.h)
        text, n, info = _picks_text(sp.lib, out)
        sp.lib.kmr_picks_free(out)
        assert text == want["text"] and n == len(want["reads"]) and info == want["info"]
    finally:
        d.close()


REF_T = 3


def test_fused_form_on_the_reference_fixture():
    """tests/golden/1000.fastq (k = 31, min depth 2, min read length 25, quality base 64, pairs (2i, 2i + 1)): scoreAndTrimReads on the
    device and then the normalization, against the restatement over the oracle's score_and_trim; FASTQ and FASTA, the text from host
    memory and from device memory"""
    import torch
    from helpers import OracleSpectrum, ReadBatch, default_config, oracle_weighted_kmers
    from refsemantics import score_and_trim
    text = open(os.path.join(GOLDEN, "1000.fastq"), "rb").read()
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, text)
    n = rs.n
    assert n == 1000
    r1, r2 = np.arange(0, n, 2, dtype=np.int64), np.arange(1, n, 2, dtype=np.int64)
    sel = ka.ReadSelector(sp, rs, pairs=(r1, r2))
    assert sel.has_pairs
    # before the spectrum is finalized the fused form has nothing to score with
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
        sel.selectReads(2, max_kmer_output_depth=REF_T)
    sp.buildKmerSpectrumFromReadSet(rs)
    sp.finalize(2)
    bs, q, off, names = rs.arrays()
    seqs = [bytes(bs[int(off[i]):int(off[i + 1])]) for i in range(n)]
    quals = [bytes(q[int(off[i]):int(off[i + 1])]) for i in range(n)]
    short = [nm.split(b" ")[0].split(b"\t")[0] for nm in names]
    ocfg = default_config(K, estimated_raw_kmers=46000)
    o = OracleSpectrum(ocfg)
    o.add_reads(ReadBatch.from_arrays(np.ascontiguousarray(bs), np.ascontiguousarray(q), np.ascontiguousarray(off, dtype=np.uint64)))
    o.finalize(2)
    to, tl, sc, wt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    for i in range(n):
        keys, _, _ = oracle_weighted_kmers(ocfg, seqs[i], quals[i])
        to[i], tl[i], sc[i], wt[i] = score_and_trim(o.lookup(keys), seqs[i], K, 2, "MEDIAN")
    zero = np.zeros(n, dtype=np.uint8)
    labels = nc.labels_of(n, zero, zero, zero, to, tl, sc, wt)
    pairs = pair_list(n, r1, r2)
    for fmt in ("fastq", "fasta"):
        want = Normalizer(REF_T, 2, 25.0, True, False, seed=5, first_read_idx=77).run(short, seqs, quals, labels, [False] * n, to, tl, sc, pairs, [0, 400, n], 64 - 33, 64, fmt == "fasta")
        files = sel.selectReads(2, 0, -1.0, 25.0, False, "MEDIAN", 64, fmt, [0, 400, n], ["a", "b"], "o", True, max_kmer_output_depth=REF_T, seed=5, first_read_idx=77)
        print("1000.fastq %s: %d picks of %d candidates, %d draws, per input %s" % (fmt, want["info"]["n_picks"], want["info"]["n_candidates"], want["info"]["n_draws"], [t[1] for t in want["table"]]))
        assert want["info"]["n_draws"] > 50 and 0 < want["info"]["n_picks"] < want["info"]["n_candidates"]
        assert sel.normalize_info == want["info"] and sel.n_picked == len(want["reads"])
        assert files == [(file_name("o", 2, REF_T, p, True, fmt == "fasta"), want["text"][fb:fb + nb]) for p, (fp, np_, fb, nb) in zip("ab", want["table"])]
        assert np.array_equal(sel.read_segment, want["read_segment"])
    # the fused _dev form: FASTA as above
    dtext = torch.frombuffer(bytearray(rs.text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    cfg = ka.KmrNormalizeConfig()
    sp.lib.kmr_normalize_config_init(C.byref(cfg))
    cfg.select.minimum_score, cfg.select.min_read_length, cfg.select.output_quality_base, cfg.select.format = 2, 25.0, 64, 1
    cfg.target_depth, cfg.seed, cfg.first_global_read_idx, cfg.by_pair = REF_T, 5, 77, 1
    i64, st = C.POINTER(C.c_int64), np.array([0, 400, n], dtype=np.uint64)
    out = C.c_void_p()
    rc = sp.lib.kmr_normalize_read_batch_dev(sp.h, rs.r, dtext.data_ptr(), dtext.numel(), r1.ctypes.data_as(i64), r2.ctypes.data_as(i64), r1.size, None, None, None,
                                             st.ctypes.data_as(C.POINTER(C.c_uint64)), 2, C.byref(cfg), C.byref(out))
    assert rc == 0, sp.lib.kmr_last_error(sp.h)
    got, n_rec, info = _picks_text(sp.lib, out)
    sp.lib.kmr_picks_free(out)
    assert got == want["text"] and info == want["info"]
    sel.close(); rs.close(); sp.close()


def test_cpp_host_side_writes_the_python_layer_s_file(tmp_path):
    """tests/cpp/normalize_demo.cpp (ReadSelector::selectReadsNormalized of include/kmernator_amd.hpp, fused) on tests/golden/1000.fastq:
    the file name of the reference and the bytes and counts the Python layer gives for the same configuration, which the test above
    holds to the restatement"""
    import subprocess
    from test_normalize_cases import build_cpp_demo
    fastq = os.path.join(GOLDEN, "1000.fastq")
    p = subprocess.run([build_cpp_demo(tmp_path), fastq, str(tmp_path / "o"), str(REF_T), "5", "77"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=46000, device=0))
    rs = ka.ReadSet(sp, open(fastq, "rb").read())
    sp.buildKmerSpectrumFromReadSet(rs)
    sp.finalize(2)
    sel = ka.ReadSelector(sp, rs, pairs=(np.arange(0, rs.n, 2), np.arange(1, rs.n, 2)))
    files = sel.selectReads(2, 0, -1.0, 25.0, False, "MEDIAN", 64, "fastq", None, ["reads"], str(tmp_path / "o"), True, max_kmer_output_depth=REF_T, seed=5, first_read_idx=77)
    assert len(files) == 1 and files[0][0].endswith("o-MinDepth2-MaxDepth%d-reads.fastq" % REF_T) and len(files[0][1]) > 10000
    assert open(files[0][0], "rb").read() == files[0][1]
    i = sel.normalize_info
    lines = p.stdout.splitlines()
    assert lines[0] == "%s %d" % (files[0][0], len(files[0][1]))
    assert lines[1] == "reads %d records %d picks %d candidates %d draws %d" % (rs.n, sel.n_picked, i["n_picks"], i["n_candidates"], i["n_draws"])
    sel.close(); rs.close(); sp.close()


# ---------------------------------------------------------------- 6: what is refused

def _live(sp):
    return int(sp.build_info("device_blocks_live"))


def test_errors(sp):
    lib = sp.lib
    b = nc.interleaved(65)
    d = Dev(sp, b)
    try:
        base = _live(sp)
        buf, tp, tn = d.sel._text_args()
        good = dict(r1=b.read1, r2=b.read2)

        def rc_of(cfg=None, form="kmr_normalize_reads", trims=True, **kw):
            rc, out = _call(sp, form, d, tp, tn, cfg if cfg is not None else _config(sp, b), trims=trims, **dict(good, **kw))
            assert out.value is None or rc == 0
            if rc == 0:
                lib.kmr_picks_free(out)
            assert _live(sp) == base
            return rc
        assert rc_of() == 0
        assert rc_of(_config(sp, b, target_depth=0)) == -1
        c = _config(sp, b); c.struct_size -= 4
        assert rc_of(c) == -1
        c = _config(sp, b); c.method = 1
        assert rc_of(c) == -7 and b"OPTIMAL" in lib.kmr_last_error(sp.h)
        c = _config(sp, b); c.use_logscale = 1
        assert rc_of(c) == -7
        # the pair list: an index past the batch, below -1, a pair without a read, a read named twice, read1 without read2
        for r1, r2, why in ((np.array([0, 65]), np.array([1, 2]), b"outside"), (np.array([0, -2]), np.array([1, 2]), b"outside"), (np.array([0, -1]), np.array([1, -1]), b"without a read"),
                            (np.array([0, 1]), np.array([1, 2]), b"twice"), (np.array([3, 4]), np.array([3, 5]), b"twice")):
            assert rc_of(r1=r1.astype(np.int64), r2=r2.astype(np.int64)) == -1
            assert why in lib.kmr_last_error(sp.h), lib.kmr_last_error(sp.h)
        assert rc_of(r2=None) == -1
        # input_starts that does not end at the batch
        assert rc_of(starts=[0, 10, 64]) == -1
        # the fused form on a handle that is not finalized
        assert rc_of(form="kmr_normalize_read_batch", trims=False) == -5
        # kmr_normalize_info is for normalized picks
        d.sel.pickAllPassingReads(0.5)
        assert lib.kmr_normalize_info(d.sel._picks, None, None, None) == -1
        # the Python layer: the reference's option check, and the method
        with pytest.raises(ka.KmerSpectrumError, match="exclude"):
            d.sel.selectReads(2, 16, max_kmer_output_depth=5)
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_UNSUPPORTED"):
            d.sel.selectReads(2, max_kmer_output_depth=5, normalization_method="OPTIMAL")
        # NULL pair list: every read a half pair, whatever n_pairs says
        want = nc.Batch.half(b, 0, b.n)
        want.read1 = want.read2 = None
        rc, out = _call(sp, "kmr_normalize_reads", d, tp, tn, _config(sp, b))
        assert rc == 0
        text, n, info = _picks_text(lib, out)
        lib.kmr_picks_free(out)
        e = want.expect()
        assert text == e["text"] and info == e["info"]
    finally:
        d.close()


# ---------------------------------------------------------------- 7: the Python layer

def test_python_layer_names_and_counts(sp):
    b = nc.blocks(70)
    d = Dev(sp, b)
    try:
        want = b.expect()
        assert d.sel.has_pairs          # 70 pairs of 145 reads: by_pair defaults to it
        files = d.sel.selectReads(b.cfg["min_score"], input_starts=b.input_starts, input_prefixes=["R1", "R2", "rest"], output="run/out", max_kmer_output_depth=nc.T, seed=b.cfg["seed"])
        assert files == [(file_name("run/out", 0, nc.T, p), want["text"][fb:fb + nb]) for p, (fp, np_, fb, nb) in zip(("R1", "R2", "rest"), want["table"])]
        assert [nm for nm, _ in files] == ["run/out-MinDepth0-MaxDepth9-%s.fastq" % p for p in ("R1", "R2", "rest")]
        n = d.sel.pickCoverageNormalizedSubset(nc.T, b.cfg["min_score"], None, True, False, seed=b.cfg["seed"])
        assert n == want["info"]["n_picks"] and d.sel.n_picked == len(want["reads"])
        whole = nc.Batch.half(b, 0, b.n)
        whole.read1, whole.read2 = b.read1, b.read2
        assert d.sel.writePicks() == whole.expect()["text"]
        # a ReadPairs from identifyPairs feeds the selector as it is
        pairs = d.rs.identifyPairs()
        s2 = ka.ReadSelector(sp, d.rs, pairs=pairs)
        assert s2.has_pairs == pairs.hasPairs() and np.array_equal(s2.pairs[0], pairs.pairs[:, 0])
        s2.close(); pairs.close()
    finally:
        d.close()
