"""The artifact filter's report on the CPU: the restatement of the reference's Recorder (tests/refartifact_report.py) is consistent
with itself on the reference's own fixture, the directed families of tests/artifactreportcases.py hold what they are written for and
notice every deliberate deviation of the restatement -- so the device comparison of tests/test_gpu_artifact_report.py cannot pass on
cases without teeth -- and the parts of the C interface that need no device: the config's defaults and every refusal that is decided
before the handle is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import artifactreportcases as arc
import kmernator_amd as ka
import refartifact as ra
import refartifact_report as rr
from kmernator_amd import _lib
from helpers import GOLDEN, OracleArtifactFilter, artifact_config, read_fastq

NEW_SYMBOLS = ["kmr_artifact_report_config_init", "kmr_artifact_filter_report", "kmr_artifact_filter_report_dev", "kmr_artifact_filter_apply_report",
               "kmr_artifact_filter_apply_report_dev", "kmr_artifact_report_counts", "kmr_artifact_report_picks", "kmr_artifact_report_free", "kmr_artifact_filter_name"]


def outputs(rep, flt):
    """everything a report hands out, comparable"""
    return [a.tolist() for a in rep.counts()], rep.table(flt), rep.files()


# ---------------------------------------------------------------- the reference's own fixture

def test_restatement_is_consistent_on_the_golden_fixture():
    """test/1000.fastq under runFilterTests.sh's artifact settings (edit distance 1 built in, --min-read-length 25): the 51 reads
    whose names carry AFTrim in test/1000-Filtered.fastq are the trimmed ones, nothing is discarded, so no file is written; the
    table's rows add up to its totals"""
    rb = read_fastq(os.path.join(GOLDEN, "1000.fastq"))
    gold = read_fastq(os.path.join(GOLDEN, "1000-Filtered.fastq"))
    fa = open(os.path.join(GOLDEN, "artifact_sequences.fa"), "rb").read()
    kw = dict(edit_distance=1, fastq_start_char=64, min_read_length=25.0)
    o = OracleArtifactFilter(artifact_config(**kw), fa)
    flt = ra.Filter(ra.Config(**kw), fa, o.entries(), o.info()[2])
    seqs, quals = [rb.seq(i) for i in range(rb.n)], [rb.qual(i) for i in range(rb.n)]
    res, _ = flt.apply(seqs, quals, names=rb.names)
    rep = rr.report(flt, res, rb.names, seqs, quals, in_base=64, out_base=33, phix_output=False)
    d, t, b = rep.counts()
    n_aftrim = sum(1 for nm in gold.names if b"AFTrim" in nm)
    assert n_aftrim == 51 and int(t.sum()) == n_aftrim
    removed = sum(len(seqs[i]) - int(m.group(1)) for i in range(rb.n) for m in [re.search(rb"AFTrim:\d+\+(\d+)", gold.names[i])] if m)
    assert int(b.sum()) == removed + sum(len(seqs[i]) for i in range(rb.n) if res["action"][i] == 2)
    n_records = sum(body.count(b"\n+\n") for _, body in rep.files())
    assert n_records == int(d.sum()) == int((res["action"] == 2).sum())
    lines = rep.table(flt).split("\n")
    assert lines[:6] == ["Final Filter Matches to reads:%d" % t.sum(), "Discarded Reads:%d" % d.sum(), "Trimmed Reads:%d" % t.sum(), "Discarded/Trimmed Bases:%d" % b.sum(),
                         "", "\tDiscarded\tAffected\tBasesRemoved\tMatch"]
    rows = [ln.split("\t") for ln in lines[6:] if ln]
    assert len(rows) == int((b > 0).sum()) and all(r[0] == "" and len(r) == 5 for r in rows)
    assert [sum(int(r[k]) for r in rows) for k in (1, 2, 3)] == [int(d.sum()), int(t.sum()), int(b.sum())]
    assert [r[4] for r in rows] == [rr.filter_name(flt, i).decode() for i in range(b.size) if b[i] > 0]
    assert rows[-1][4] == "MinQualityTrim3" and int(rows[-1][2]) == 51      # the golden trims are quality trims


# ---------------------------------------------------------------- the families hold what they are written for

def test_every_kind_of_read_meets_its_rule():
    """a read of each kind on its own comes to the action and value its name promises"""
    c = arc.CASES["singles"]
    res = arc.decisions("singles")[0]
    n_seq = arc.reference_filter("singles").n_seq
    for i, kind in enumerate(c.kinds):
        act, v = arc.ALONE[kind]
        assert (int(res["action"][i]), int(res["value"][i])) == (act, n_seq if v == "q" else v), (i, kind)
    res = arc.decisions("singles-nameless")[0]
    for i, kind in enumerate(arc.CASES["singles-nameless"].kinds):
        act, v = arc.ALONE[kind]
        assert (int(res["action"][i]), int(res["value"][i])) == (act, n_seq if v == "q" else v), (i, kind)


def test_pairs_family_reaches_every_pair_rule():
    res = arc.decisions("pairs")[0]
    act, val = res["action"].tolist(), res["value"].tolist()
    phix, ref = arc.ac.IDX[b"phix"], arc.ac.IDX[b"reference"]
    assert (act[0], act[1], val[0], val[1]) == (2, 2, phix, 0)                 # the clean mate of a PhiX read goes with it
    assert act[4] == act[5] == 2 and val[4] != val[5]                          # both discarded, read1 the higher index
    assert (act[6], act[7], val[7]) == (2, 0, 0)
    assert (act[8], act[9]) == (1, 2)
    assert (act[10], act[11], val[10]) == (2, 2, ref) and arc.ALONE["adapter"][0] == 1      # the mate's trim became a discard
    assert (act[12], act[13]) == (2, 0)
    assert (act[16], act[17]) == (1, 1)
    rep = arc.expected("pairs")
    art = [r for r, _ in rep.records[0][0]]
    assert art == [2, 5, 4, 6, 9, 10, 11, 12]                                   # unit order, read1 first: 5 before 4
    assert [r for r, _ in rep.records[1][0]] == [0, 1, 14, 15]
    two = arc.expected("pairs-two-inputs")
    assert [r for r, _ in two.records[0][1]] == [4, 0] and [r for r, _ in two.records[0][0]] == [2]      # filed under read1's input
    three = arc.expected("three-inputs")
    assert not three.records[0][1] and not three.records[1][1] and len(three.files()) == 4


def test_names_and_labels():
    rep = arc.expected("names")
    recs = [b for _, b in rep.records[0][0]]
    assert recs[0].startswith(b"@blank MinQualityTrim3\nN\n+\n") and rep.records[1][0][0][1].startswith(b"@tab\nN\n+\n")
    assert tuple(len(b) for b in recs[1:]) == arc.RECORD_SIZES
    lab = arc.expected("labels-1-100")
    a, b = (x for _, x in lab.records[0][0])
    assert a.startswith(b"@read0/1 x\nN\n") and b.startswith(b"@read1/2 " + b"L" * 100 + b"\nN\n")
    for cid, lo in (("shift-64-to-33", 33), ("shift-33-to-64", 64)):
        body = arc.expected(cid).file_bytes(0, 0).split(b"\n")[3]
        assert set(body) == {lo + 2, lo + 40}                                   # '#' and 'I' of base 33, moved
    many = arc.expected("many-sequences")
    d, t, bases = many.counts()
    assert d.size == arc.MANY_SEQ + 2 and 24 * d.size > 6144
    assert [int(i) for i in np.nonzero(bases)[0]] == [1, 150, 299, 300, 301]


def test_random_batch_mixes_everything():
    c = arc.CASES["random-r1r2"]
    rep = arc.expected("random-r1r2")
    d, t, b = rep.counts()
    assert c.n == 2200 and all(len(rep.records[row][j]) > 20 for row in range(2) for j in range(2))
    assert int(t.sum()) > 100 and int((d > 0).sum()) >= 4
    seg = rep.read_segment(c.n)
    assert (seg[:arc.RANDOM_HALF] == 1).any() and (seg[arc.RANDOM_HALF:] == 0).any()      # records filed under the mate's input, both ways


@pytest.mark.parametrize("variant", rr.VARIANTS)
def test_every_deviation_is_noticed_by_its_family_and_by_no_other(variant):
    cid = arc.SENSITIVE[variant]
    flt = arc.reference_filter(cid)
    assert outputs(arc.expected(cid), flt) != outputs(arc.expected(cid, variant=variant), flt), (variant, cid)
    for other in arc.UNTOUCHED[variant]:
        flt = arc.reference_filter(other)
        assert outputs(arc.expected(other), flt) == outputs(arc.expected(other, variant=variant), flt), (variant, other)


def test_print_bases_is_the_bases_printed_deviation():
    for cid in ("singles", "pairs-nameless"):
        flt = arc.reference_filter(cid)
        assert outputs(arc.expected(cid, print_bases=True), flt) == outputs(arc.expected(cid, variant="bases_printed"), flt)


# ---------------------------------------------------------------- the C interface without a device

def _config(**kw):
    c = ka.KmrArtifactReportConfig()
    assert ka.load().kmr_artifact_report_config_init(C.byref(c)) == 0
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def test_new_symbols_are_exported():
    lib = ka.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_report_config_defaults_and_size():
    c = _config()
    assert c.struct_size == C.sizeof(ka.KmrArtifactReportConfig) == 20
    assert (c.artifact_output, c.phix_output, c.output_quality_base, c.print_bases) == (1, 1, 33, 0)
    assert ka.load().kmr_artifact_report_config_init(None) == -1


@pytest.mark.parametrize("entry", ["kmr_artifact_filter_report", "kmr_artifact_filter_report_dev", "kmr_artifact_filter_apply_report", "kmr_artifact_filter_apply_report_dev"])
def test_bad_config_and_null_handle_are_refused(entry):
    """the configuration is checked before anything else, so the refusal and its reason can be seen without a device"""
    lib = ka.load()
    fn = getattr(lib, entry)
    fused = "apply" in entry

    def call(cfg):
        rep, out = C.c_void_p(1), C.c_void_p(1)
        mid = [None] * 6 + [C.byref(out)] if fused else [None] * 4
        rc = fn(None, None, None, None, 0, None, None, 0, *mid, None, 0, C.byref(cfg) if cfg is not None else None, C.byref(rep))
        assert rep.value is None and (not fused or out.value is None)          # cleared on every failure
        return rc, lib.kmr_last_error(None).decode()
    for bad, why in ((dict(struct_size=16), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(output_quality_base=0), "output_quality_base"),
                     (dict(output_quality_base=48), "output_quality_base")):
        rc, text = call(_config(**bad))
        assert rc == -1 and why in text, (bad, rc, text)
    rc, text = call(None)
    assert rc == -1 and "NULL" in text
    rc, text = call(_config())
    assert rc == -1 and "NULL handle" in text and entry in text


def test_null_objects_are_refused():
    lib = ka.load()
    buf = C.create_string_buffer(8)
    assert lib.kmr_artifact_report_counts(None, None, None, None, 0) == -1 and lib.kmr_artifact_report_picks(None, None) == -1
    assert lib.kmr_artifact_filter_name(None, 1, buf, 8) == -1
    lib.kmr_artifact_report_free(None)


# ---------------------------------------------------------------- the C++ host side (include/kmernator_amd.hpp: FilterKnownOddities::report)

def build_report_demo(tmp_path):
    import subprocess
    from helpers import ROOT
    exe = str(tmp_path / "report_demo")
    lib_dir = os.path.join(ROOT, "kmernator_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "report_demo.cpp"), "-L" + lib_dir, "-lkmernator_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_report_compiles_and_links(tmp_path):
    """the C++ wrapper against the library, warnings as errors (it runs in tests/test_gpu_artifact_report.py)"""
    assert os.path.exists(build_report_demo(tmp_path))
