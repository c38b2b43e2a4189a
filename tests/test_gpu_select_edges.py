"""Every directed case of tests/selectcases.py through kmr_select_reads (ReadSelector.pickAllPassing* / writePicks) and through
kmr_partition_reads (ReadSelector.selectReads over the same host arrays, one round, the case's inputs) against the restatement of
tests/refselect.py, byte for byte: the text, the pick flags, n_picked, bytes, and from the partition the segment table and every
read's segment.  One case per family also goes through kmr_select_reads_dev, the text in device memory (ReadSelector.device_text_of_reads).  tests/test_select_cases.py
proves on the CPU that the cases reach the edges they are named for.  No spectrum is built: a case is a handful of launches."""
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import selectcases as sc

pytestmark = pytest.mark.gpu
K = 31


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def cases(family):
    return sc.family(family, cu_count()) if family == "B" else sc.family(family)


@functools.lru_cache(maxsize=None)
def wanted(family, index):
    """the restatement's answers for kmr_select_reads (one input) and kmr_partition_reads (the case's inputs), computed once"""
    case = cases(family)[index]
    return sc.run(case), sc.run(case, input_starts=True)


def read_set(sp, case):
    cfg, reads = case["cfg"], case["reads"]
    if case["kind"] == "fastq":
        rs = ka.ReadSet(sp, sc.text_of(case), input_quality_base=cfg["in_base"])
    elif case["kind"] == "fasta":
        rs = ka.ReadSet.from_fasta(sp, sc.text_of(case))
    else:
        offsets = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.uint64)
        rs = ka.ReadSet.from_arrays(sp, np.frombuffer(b"".join(r[1] for r in reads), dtype=np.uint8), np.frombuffer(b"".join(r[2] for r in reads), dtype=np.uint8), offsets)
    assert rs.n == len(reads) and (case["kind"] != "fastq" or rs.input_quality_base == cfg["in_base"]), case["label"]
    b, q, _, names = rs.arrays()          # the batch holds the bytes the restatement is given; a name's span starts at its name
    assert b.tobytes() == b"".join(r[1] for r in reads) and q.tobytes() == b"".join(r[2] for r in reads), case["label"]
    cut = lambda line: line.split(b" ")[0].split(b"\t")[0]
    assert [cut(nm) for nm in names] == [cut(r[0]) if case["kind"] != "arrays" else b"" for r in reads], case["label"]
    return rs


def selector(sp, rs, case, with_mates=True):
    af = case["af"]
    sel = ka.ReadSelector(sp, rs, mate=case["mate"] if with_mates else None, filter_results=None if af is None else dict(action=af[0], min_pass=af[1], max_pass=af[2]))
    sel.trims = (case["to"], case["tl"], case["sc"], case["wt"])
    sel.bimodal_words = case["words"]
    sel.scoring = sc.SCORINGS[case["cfg"]["scoring"]]
    return sel


def check(label, want, text, flags, n_picked, n_bytes):
    assert n_picked == want.n_picked and n_bytes == want.bytes == len(text), label
    assert np.array_equal(flags, want.picked), (label, np.nonzero(flags != want.picked)[0][:10])
    if text != want.text:
        at = next(i for i in range(min(len(text), len(want.text))) if text[i] != want.text[i])
        raise AssertionError((label, at, text[max(0, at - 60):at + 40], want.text[max(0, at - 60):at + 40]))


def pick(sel, case):
    """the case's plain selection: pickAllPassingPairs, or pickAllPassingReads where the case says the mates are not to count"""
    cfg = case["cfg"]
    if case["use_mate"]:
        return sel.pickAllPassingPairs(cfg["min_score"], cfg["min_read_length"], cfg["both_pass"])
    return sel.pickAllPassingReads(cfg["min_score"], cfg["min_read_length"])


def run_case(family, index, device_text=False):
    case = cases(family)[index]
    cfg, label = case["cfg"], case["label"]
    want_select, want_partition = wanted(family, index)
    fmt = "fasta" if cfg["fasta"] else "fastq"
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 16, device=0, fastq_start_char=cfg["in_base"]))
    rs = read_set(sp, case)
    sel = selector(sp, rs, case)          # it knows the mates; pickAllPassingReads has to look past them
    if device_text:
        import torch
        dt = torch.frombuffer(bytearray(rs.text), dtype=torch.uint8).to("cuda:0") if rs.text else None          # a batch without names has no text
        torch.cuda.synchronize()
        sel.device_text_of_reads = (dt.data_ptr(), dt.numel()) if dt is not None else (0, 0)
        n = pick(sel, case)
        text = sel.writePicks(cfg["out_base"], fmt)
        check(label + " device text", want_select, text, sel.picked_flags, sel.n_picked, sel.bytes)
        assert n == want_select.n_picked
    else:
        n = pick(sel, case)
        text = sel.writePicks(cfg["out_base"], fmt)
        check(label + " select", want_select, text, sel.picked_flags, sel.n_picked, sel.bytes)
        assert n == want_select.n_picked
        if not case["use_mate"]:          # a partition decides by the mates it is given: none
            sel.close()
            sel = selector(sp, rs, case, with_mates=False)
        files = sel.selectReads(cfg["min_score"], 0, -1.0, cfg["min_read_length"], cfg["both_pass"], output_quality_base=cfg["out_base"], format=fmt, input_starts=cfg["input_starts"])
        check(label + " partition", want_partition, b"".join(t for _, t in files), sel.picked_flags, sel.n_picked, sel.bytes)
        seg = sel.segments
        table = [tuple(int(seg[k][0, j]) for k in ("first_pick", "picks", "first_byte", "bytes")) for j in range(seg["picks"].shape[1])]
        assert seg["picks"].shape[0] == 1 and table == want_partition.table, (label, table, want_partition.table)
        assert np.array_equal(sel.read_segment, want_partition.read_segment), label
        assert [t for _, t in files] == [want_partition.text[t[2]:t[2] + t[3]] for t in want_partition.table if t[1]], label
    sel.close()
    rs.close()
    sp.close()


def _ids(family):
    return [c["label"] for c in sc.family(family)]


@pytest.mark.parametrize("index", range(len(sc.family("L"))), ids=_ids("L"))
def test_length(index):
    run_case("L", index)


@pytest.mark.parametrize("index", range(len(sc.family("S"))), ids=_ids("S"))
def test_score(index):
    run_case("S", index)


@pytest.mark.parametrize("index", range(len(sc.family("B"))), ids=_ids("B"))
def test_labels(index):
    """B-longest: as many picks with the longest label as the writer's largest grid has wavefronts, then as many with a one-part label"""
    if cases("B")[index]["label"] == "B-longest":
        assert len(cases("B")[index]["reads"]) == 2 * 4 * 8 * cu_count()
    run_case("B", index)


@pytest.mark.parametrize("index", range(len(sc.family("G"))), ids=_ids("G"))
def test_geometry(index):
    run_case("G", index)


@pytest.mark.parametrize("index", range(len(sc.family("C"))), ids=_ids("C"))
def test_slices(index):
    run_case("C", index)


@pytest.mark.parametrize("index", range(len(sc.family("Q"))), ids=_ids("Q"))
def test_reads_without_qualities(index):
    run_case("Q", index)


@pytest.mark.parametrize("index", range(len(sc.family("P"))), ids=_ids("P"))
def test_pairs_and_inputs(index):
    run_case("P", index)


DEVICE_TEXT = {"L": "L-0.4", "S": "S-pinned", "B": "B-widths-MEDIAN", "G": "G-64-33", "C": "C-33-64", "Q": "Q-arrays-33-64", "P": "P-either"}


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_from_device_text(family):
    run_case(family, _ids(family).index(DEVICE_TEXT[family]), device_text=True)
