"""The artifact filter's report on the device (kmr_artifact_filter_report, kmr_artifact_filter_apply_report; artifact_classify_kernel,
artifact_write_kernel in kmernator_amd/csrc/kmr_artifact_report.hpp) held to tests/refartifact_report.py, the reference's Recorder
restated from its source, on the families of tests/artifactreportcases.py (proven on the CPU, in tests/test_artifact_report_cases.py,
to reach every rule and to notice every deliberate deviation).

Everything compared is an integer or a byte: the three counters, every file, the table text, the per-read segments; in the fused form
also the six result arrays and the read set afterwards against kmr_artifact_filter_apply alone."""
import ctypes as C

import numpy as np
import pytest

import artifactreportcases as arc
import kmernator_amd as ka
import refartifact_report as rr

pytestmark = pytest.mark.gpu

KEYS = ("value", "min_pass", "max_pass", "action", "remnant_off", "remnant_len")


class Device:
    """one handle per quality base and one filter per configuration, for the module's lifetime"""

    def __init__(self):
        self.sps, self.filters = {}, {}

    def sp(self, base=33):
        if base not in self.sps:
            self.sps[base] = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1000, device=0, fastq_start_char=base))
        return self.sps[base]

    def filter(self, c):
        key = (c.in_base, c.fasta, tuple(sorted(c.kw.items())))
        if key not in self.filters:
            self.filters[key] = ka.FilterKnownOddities(self.sp(c.in_base), c.fasta, **dict(c.kw, build_edits=0))
        return self.filters[key]

    def read_set(self, c):
        sp = self.sp(c.in_base)
        rs = ka.ReadSet.from_arrays(sp, *c.arrays()) if c.names is None else ka.ReadSet(sp, c.fastq(), input_quality_base=c.in_base)
        assert rs.n == c.n
        return rs

    def close(self):
        for f in self.filters.values():
            f.close()
        for sp in self.sps.values():
            sp.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def device_text(rs):
    """the name text in device memory: (the tensor, its pointer)"""
    import torch
    t = torch.frombuffer(bytearray(rs.text or b"\0"), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def assert_report(what, rep, c, want, flt):
    for got, exp, key in zip(rep.counts(), want.counts(), ("discarded", "trimmed", "bases")):
        assert np.array_equal(got, exp), (what, key, got, exp)
    assert rep.files("out", c.prefixes()) == want.files("out", c.prefixes()), what
    assert rep.toString() == want.table(flt), what
    assert np.array_equal(rep.read_segment, want.read_segment(c.n)), what
    n_records = sum(len(recs) for row in want.records for recs in row)
    assert (rep.n_records, rep.bytes) == (n_records, sum(len(b) for _, b in want.files())), what
    assert rep.device_text()[1] == rep.bytes and (rep.bytes == 0 or rep.device_text()[0]), what


def run_all_routes(dev, c, print_bases, want, **options):
    """the report from host arrays and the fused form, each from host text and from device text"""
    f, flt = dev.filter(c), arc.reference_filter(c.id)
    rs = dev.read_set(c)
    keep, dtext = device_text(rs)
    alone, alone_rs = f.applyFilter(rs, c.mate())
    ref = arc.decisions(c.id)[0]
    for key in KEYS:
        assert np.array_equal(alone[key], ref[key]), (c.id, key)
    kw = dict(pairs=c.pair_arrays(), input_starts=c.input_starts, output_quality_base=c.out_base, print_bases=print_bases, **options)
    for text in (None, dtext):
        with f.report(rs, alone, device_text=text, **kw) as rep:
            assert_report((c.id, "report", text is not None), rep, c, want, flt)
        got, frs, rep = f.applyFilter(rs, report=True, device_text=text, **kw)
        with rep:
            assert_report((c.id, "fused", text is not None), rep, c, want, flt)
        for key in KEYS:
            assert np.array_equal(got[key], alone[key]), (c.id, "fused", key)
        a, b = frs.arrays(), alone_rs.arrays()
        assert frs.n == alone_rs.n and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3], (c.id, "fused batch")
        frs.close()
    res, none, rep = f.applyFilterReport(rs, want_reads=False, want_results=False, **kw)      # nothing asked for but the report
    with rep:
        assert res is None and none is None
        assert_report((c.id, "fused, report only"), rep, c, want, flt)
    alone_rs.close()
    rs.close()


@pytest.mark.parametrize("print_bases", [False, True])
@pytest.mark.parametrize("case_id", [i for i in arc.ids() if i != "random-r1r2"])
def test_family_equals_the_restatement(dev, case_id, print_bases):
    c = arc.CASES[case_id]
    run_all_routes(dev, c, print_bases, arc.expected(case_id, print_bases=print_bases))


@pytest.mark.parametrize("units", [0, 2, 5])
def test_random_batch_across_unit_boundaries(dev, units):
    """2200 reads in an R1 and an R2 block, 1200 units of the pair list: one unit of the partition by default, 2 and 5 with kmr_tune
    partition_units, so that the stable partition crosses unit boundaries"""
    c = arc.CASES["random-r1r2"]
    sp = dev.sp(c.in_base)
    sp.tune(partition_units=units)
    try:
        run_all_routes(dev, c, units == 5, arc.expected(c.id, print_bases=units == 5))
    finally:
        sp.tune(partition_units=0)


@pytest.mark.parametrize("case_id", ["many-sequences", "singles", "random-r1r2"])
def test_both_counting_paths_agree(dev, case_id):
    """the counters summed in LDS per unit and by global atomics: the default takes LDS while 24 bytes a sequence index fit 6 KiB"""
    c = arc.CASES[case_id]
    f, flt, sp = dev.filter(c), arc.reference_filter(case_id), dev.sp(c.in_base)
    rs = dev.read_set(c)
    want = arc.expected(case_id)
    ran = {}
    try:
        for knob in (-1, 0, 1):
            sp.tune(artifact_report_lds=knob)
            got, _, rep = f.applyFilterReport(rs, pairs=c.pair_arrays(), input_starts=c.input_starts, want_reads=False)
            ran[knob] = int(sp.build_info("artifact_report_lds"))
            with rep:
                assert_report((case_id, "knob", knob), rep, c, want, flt)
    finally:
        sp.tune(artifact_report_lds=-1)
    rs.close()
    assert ran == {-1: 0 if case_id == "many-sequences" else 1, 0: 0, 1: 1}


@pytest.mark.parametrize("artifact_output,phix_output", [(False, True), (True, False), (False, False)])
def test_an_output_switched_off_keeps_the_counts(dev, artifact_output, phix_output):
    c = arc.CASES["pairs"]
    want = arc.expected("pairs", artifact_output=artifact_output, phix_output=phix_output)
    assert [n for n, _ in want.files()] == [n for n, on in (("-transformed-1-Artifact.fastq", artifact_output), ("-transformed-1-PhiX.fastq", phix_output)) if on]
    assert all(np.array_equal(a, b) for a, b in zip(want.counts(), arc.expected("pairs").counts()))
    run_all_routes(dev, c, False, want, artifact_output=artifact_output, phix_output=phix_output)


def test_empty_batch_and_batch_without_records(dev):
    c = arc.CASES["singles"]
    f, sp = dev.filter(c), dev.sp()
    empty = ka.ReadSet(sp, b"", input_quality_base=33)
    assert empty.n == 0
    for pairs in (None, (np.zeros(0, np.int64), np.zeros(0, np.int64))):
        res, frs, rep = f.applyFilterReport(empty, pairs=pairs)
        with rep:
            assert (rep.n_records, rep.bytes, rep.files(), rep.text()) == (0, 0, [], b"") and not any(a.any() for a in rep.counts())
            assert rep.toString() == "Final Filter Matches to reads:0\nDiscarded Reads:0\nTrimmed Reads:0\nDiscarded/Trimmed Bases:0\n\n\tDiscarded\tAffected\tBasesRemoved\tMatch\n"
        with f.report(empty, {k: np.zeros(0, np.uint32) for k in KEYS}, pairs=pairs) as rep:
            assert (rep.n_records, rep.bytes, rep.files()) == (0, 0, [])
        frs.close()
    empty.close()
    clean = arc.Case("clean-only", ["clean", "clean", "quality", "clean"])      # a trim is counted, nothing is written
    rs = ka.ReadSet(sp, clean.fastq(), input_quality_base=33)
    res, frs, rep = f.applyFilterReport(rs, pairs=([0, 3], [1, 2]))
    with rep:
        d, t, b = rep.counts()
        assert (rep.n_records, rep.bytes, rep.files()) == (0, 0, []) and int(t.sum()) == 1 and int(d.sum()) == 0
        assert res["action"].tolist() == [0, 0, 1, 0] and int(b.sum()) == 100 - int(res["max_pass"][2] - res["min_pass"][2])
        assert (rep.read_segment == -1).all()
    frs.close()
    rs.close()


def test_filter_names(dev):
    c = arc.CASES["labels-1-100"]
    f, flt = dev.filter(c), arc.reference_filter(c.id)
    assert [f.getFilterName(i) for i in range(1, f.n_sequences + 1)] == ["x", "L" * 100, "MinQualityTrim3"]
    assert [f.getFilterName(i).encode() for i in range(1, f.n_sequences + 1)] == [rr.filter_name(flt, i) for i in range(1, flt.n_seq + 1)]
    buf = C.create_string_buffer(101)
    lib = dev.sp().lib
    assert lib.kmr_artifact_filter_name(f.f, 2, buf, 100) == -6 and lib.kmr_artifact_filter_name(f.f, 2, buf, 101) == 0 and buf.value == b"L" * 100
    assert lib.kmr_artifact_filter_name(f.f, 0, buf, 100) == -1 and lib.kmr_artifact_filter_name(f.f, f.n_sequences + 1, buf, 100) == -1


def test_every_refusal_returns_its_code_and_leaves_the_handle_usable(dev):
    c = arc.CASES["pairs"]
    f, sp = dev.filter(c), dev.sp()
    lib = sp.lib
    rs = dev.read_set(c)
    res, _ = f.applyFilter(rs, c.mate(), want_reads=False)
    want, flt = arc.expected("pairs"), arc.reference_filter("pairs")
    r1, r2 = c.pair_arrays()
    u32, u8, i64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    text = np.frombuffer(rs.text, dtype=np.uint8)

    def cfg(**kw):
        x = ka.KmrArtifactReportConfig()
        lib.kmr_artifact_report_config_init(C.byref(x))
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def raw(config=None, a=r1, b=r2, n_pairs=None, value=None, flt_handle=None, fused=False, starts=None):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.int64)
        value = np.ascontiguousarray(res["value"] if value is None else value, dtype=np.uint32)
        starts = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
        rep, out = C.c_void_p(1), C.c_void_p(1)
        head = [sp.h, (flt_handle or f).f, rs.r, text.ctypes.data_as(C.c_void_p), text.size, None if a is None else a.ctypes.data_as(i64), None if b is None else b.ctypes.data_as(i64),
                (0 if a is None else a.size) if n_pairs is None else n_pairs]
        tail = [None if starts is None else starts.ctypes.data_as(C.POINTER(C.c_uint64)), 0 if starts is None else starts.size - 1, C.byref(config or cfg()), C.byref(rep)]
        if fused:
            rc = lib.kmr_artifact_filter_apply_report(*head, None, None, None, None, None, None, C.byref(out), *tail)
            assert rc == 0 or out.value is None
            if rc == 0:
                lib.kmr_reads_free(out)
        else:
            rc = lib.kmr_artifact_filter_report(*head, value.ctypes.data_as(u32), res["action"].ctypes.data_as(u8), res["min_pass"].ctypes.data_as(u32),
                                                res["max_pass"].ctypes.data_as(u32), *tail)
        assert rc == 0 or rep.value is None
        if rc == 0:
            lib.kmr_artifact_report_free(rep)
        return rc, lib.kmr_last_error(sp.h).decode()

    no_phix = ka.FilterKnownOddities(sp, c.fasta, **dict(c.kw, build_edits=0, phix_idx=0))
    twice, outside, nobody = r1.copy(), r1.copy(), r1.copy()
    twice[1] = 0                       # (2, -1) becomes (0, -1): read 0 is named by two pairs
    nobody[1] = -1                     # ... and (-1, -1) here
    outside[0] = c.n
    bad_value = res["value"].copy()
    bad_value[3] = f.n_sequences + 1
    refusals = [
        (dict(config=cfg(struct_size=24)), "struct_size"),
        (dict(config=cfg(output_quality_base=48)), "output_quality_base"),
        (dict(b=None), "read1 and read2 go together"),
        (dict(a=outside), "outside the batch"),
        (dict(a=np.full(r1.size, -2)), "outside the batch"),
        (dict(a=nobody), "pair without a read"),
        (dict(a=twice), "names a read twice"),
        (dict(a=r1[1:], b=r2[1:]), "leaves a read out"),
        (dict(a=r1, b=r2, n_pairs=0), "leaves a read out"),
        (dict(flt_handle=no_phix), "phix_idx is 0"),
        (dict(starts=[0, 5, c.n - 1]), "input_starts ends at"),
        (dict(starts=[1, 5, c.n]), "input_starts[0]"),
    ]
    for fused in (False, True):
        for kw, why in refusals + ([] if fused else [(dict(value=bad_value), "above the filter's n_sequences")]):
            rc, msg = raw(fused=fused, **kw)
            assert rc == -1 and why in msg, (fused, kw.keys(), rc, msg)
            assert raw(fused=fused)[0] == 0                                    # the handle goes on working
    with pytest.raises(ka.KmerSpectrumError, match="phix_idx is 0"):
        no_phix.report(rs, res, pairs=(r1, r2), phix_output=True)
    with no_phix.report(rs, res, pairs=(r1, r2)) as rep:                       # phix_output follows the filter: off
        assert [n for n, _ in rep.files()] == ["-transformed-1-Artifact.fastq"]
    no_phix.close()
    buf = np.zeros(3, dtype=np.uint64)
    with f.report(rs, res, pairs=(r1, r2)) as rep:
        assert lib.kmr_artifact_report_counts(rep._rep, buf.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, f.n_sequences) == -6      # KMR_ERR_CAPACITY
        assert_report("after the refusals", rep, c, want, flt)
    rs.close()


def test_cpp_report_equals_the_restatement(tmp_path):
    """tests/cpp/report_demo.cpp: the filter, its results and the report through the C++ classes, reads paired (2i, 2i + 1)"""
    import subprocess
    from test_artifact_report_cases import build_report_demo
    kinds = ["phix", "clean", "quality_discard", "adapter", "clean", "adapter_short", "quality", "quality", "clean", "clean", "quality_discard", "phix"]
    c = arc.Case("cpp", kinds, pairs=[(i, i + 1) for i in range(0, len(kinds), 2)], kw=dict(edit_distance=0, phix_idx=arc.ac.IDX[b"phix"]))
    flt = arc.ra.Filter(arc.ra.Config(**dict(c.kw, build_edits=0)), c.fasta)
    res, _ = flt.apply(c.seqs, c.quals, c.mate(), c.names)
    want = rr.report(flt, res, c.names, c.seqs, c.quals, c.pairs)
    fq, fa, out = tmp_path / "reads.fastq", tmp_path / "artifacts.fa", tmp_path / "records"
    fq.write_bytes(c.fastq())
    fa.write_bytes(c.fasta)
    p = subprocess.run([build_report_demo(tmp_path), str(fq), str(fa), str(out), str(flt.cfg.phix_idx)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    d, t, b = want.counts()
    lines = ["%d %d %d %s" % (d[i], t[i], b[i], rr.filter_name(flt, i).decode()) for i in range(b.size) if b[i]]
    art, phix = want.file_bytes(0, 0), want.file_bytes(1, 0)
    lines += ["segment %d 0 %d" % (len(want.records[0][0]), len(art)), "segment %d %d %d" % (len(want.records[1][0]), len(art), len(phix))]
    assert p.stdout.splitlines() == lines and len(art) and len(phix)
    assert out.read_bytes() == art + phix
