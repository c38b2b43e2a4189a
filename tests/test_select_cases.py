"""The directed cases of the selection and its output text (tests/selectcases.py) against the restatement (tests/refselect.py) on the
CPU: the unswitched restatement gives what refsemantics.filterreads_output gives wherever that one is defined and right; every case
changes under each rule it is written to notice; every rule refselect can switch is noticed by a named family; every family reaches
the edge it is aimed at, asserted on the expected output alone -- so the device comparison of tests/test_gpu_select_edges.py cannot
pass on cases that miss their line."""
import functools
import re

import numpy as np
import pytest

import refbimodal
import refselect
import refsemantics
import selectcases as sc

# which family is answerable for which rule (test_every_rule_has_a_family holds the list complete)
ANSWERS = {
    "product_in_double": "L", "fraction_strict": "L", "absolute_strict": "L", "score_strict": "S", "score_truncates": "S", "score_half_even": "S",
    "score_half_in_float": "S", "mask_at_zero": "C", "no_slice_clamp": "C", "aftrim_unsigned": "B", "inv_on_equal": "B", "label_parts_swapped": "B",
    "name_ends_at_blank_only": "G", "masked_qual_from_input_base": "C", "shift_wrong_sign": "G", "ref_qual_shifted": "Q", "ref_qual_every_byte": "Q",
    "both_pass_as_either": "P", "failed_mate_left_out": "P",
}


def _all():
    return [(f, i) for f in sc.FAMILIES for i in range(len(sc.family(f)))]


def _ids():
    return [c["label"] for f in sc.FAMILIES for c in sc.family(f)]


@functools.lru_cache(maxsize=None)
def base(family, index):
    return sc.run(sc.family(family)[index], input_starts=True)


def case_named(label):
    for i, c in enumerate(sc.family(label[0])):
        if c["label"] == label:
            return c, base(label[0], i)
    raise KeyError(label)


def records(text, fasta=False):
    """the records of an output text as lists of lines (a FASTQ quality line may start with '@': four lines each)"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    per = 2 if fasta else 4
    assert (len(lines) - 1) % per == 0
    return [lines[i:i + per] for i in range(0, len(lines) - 1, per)]


@pytest.mark.parametrize("family,index", _all(), ids=_ids())
def test_the_case_notices_its_rules(family, index):
    case = sc.family(family)[index]
    want = sc.signature(base(family, index))
    for rule in case["rules"]:
        assert sc.signature(sc.run(case, rule, input_starts=True)) != want, (case["label"], rule)


def test_every_rule_has_a_family():
    assert set(ANSWERS) == set(refselect.RULES) and len(refselect.RULES) == 19
    for rule, f in ANSWERS.items():
        assert any(rule in c["rules"] for c in sc.family(f)), (rule, f)
    for f in sc.FAMILIES:          # labels are what the device test's ids are made of
        labels = [c["label"] for c in sc.family(f)]
        assert len(set(labels)) == len(labels) and all(l.startswith(f + "-") for l in labels)
    with pytest.raises(AssertionError):
        sc.run(sc.family("P")[0], "no_such_rule")


def test_sizes_stay_small():
    for f in sc.FAMILIES:
        for c in sc.family(f):
            assert len(c["reads"]) <= 300 or c["label"] == "B-longest", c["label"]


# ---- against the older restatement, where it is defined and right: real qualities, FASTQ, defined scores, slices inside the read
def through_filterreads_output(case, keep=None):
    """refsemantics.filterreads_output decides over the pairs (2i, 2i + 1).  A case of singles is given to it as every read twice (a
    pair of twins passes exactly when the read does), and its text is then every record twice."""
    cfg = case["cfg"]
    idx = list(range(len(case["reads"]))) if keep is None else list(keep)
    twins = case["mate"] is None or not case["use_mate"]
    if not twins:
        assert all(int(case["mate"][i]) == (i ^ 1) for i in idx)
    order = [i for i in idx for _ in range(2 if twins else 1)]
    af = case["af"]
    labels = []
    for i in order:
        if af is not None and af[0][i] == 2:          # a discarded read was never scored: no label (scoreAndTrimReads :1195-1197)
            labels.append(b"")
            continue
        aftrim =(int(af[1][i]), int(af[2][i])) if af is not None and af[0][i] == 1 else None
        labels.append(refbimodal.label_of(sc.SCORINGS[cfg["scoring"]], int(case["to"][i]), int(case["tl"][i]), case["sc"][i], bool(case["wt"][i]),
                                          0 if case["words"] is None else int(case["words"][i]), aftrim))
    text = refsemantics.filterreads_output([case["reads"][i][0].split(b" ")[0].split(b"\t")[0] for i in order], [case["reads"][i][1] for i in order],
                                           [case["reads"][i][2] for i in order], labels, [af is not None and af[0][i] == 2 for i in order],
                                           [case["to"][i] for i in order], [case["tl"][i] for i in order], [case["sc"][i] for i in order],
                                           np.float32(cfg["min_score"]), cfg["min_read_length"], cfg["both_pass"], cfg["out_base"] - cfg["in_base"], cfg["out_base"])
    return text, twins


# Which cases go through it whole: L, S-round, the FASTQ cases of G, and the adjacent pairs of P.  Left out, and why: S-threshold and
# S-pinned hold scores whose label the reference does not define; Q holds 127s, which the old restatement moves like qualities; B and C
# hold trims past the read's end, where it decides the mask before it clamps and prints a base or an empty line.  Of B the labels,
# and of C the slices that lie inside their reads, are checked below.
@pytest.mark.parametrize("label", [c["label"] for c in sc.family("L")] + [c["label"] for c in sc.family("S") if c["label"].startswith("S-round")]
                         + [c["label"] for c in sc.family("G") if "fasta" not in c["label"]] + ["P-either", "P-both"])
def test_the_restatement_agrees_with_filterreads_output(label):
    case, res = case_named(label)
    keep = range(8) if label.startswith("P-") else None          # the adjacent pairs of P
    old, twins = through_filterreads_output(case, keep)
    mine = records(res.text)
    if keep is not None:
        mine = [r for r in mine if int(r[0][2:].split(b" ")[0]) < 8]          # names r0 .. r13
    want = [r for r in mine for _ in range(2 if twins else 1)]
    assert records(old) == want


@pytest.mark.parametrize("scoring", sc.SCORINGS)
def test_the_labels_of_b_agree_with_the_bimodal_restatement(scoring):
    """every label of B-widths against refbimodal.label_of, which composes it from the same parts on its own"""
    case, res = case_named("B-widths-" + scoring)
    af = case["af"]
    for i, r in enumerate(records(res.text)):
        aftrim = (int(af[1][i]), int(af[2][i])) if af[0][i] == 1 else None
        want = refbimodal.label_of(scoring, int(case["to"][i]), int(case["tl"][i]), case["sc"][i], bool(case["wt"][i]), int(case["words"][i]), aftrim)
        assert r[0] == b"@" + case["reads"][i][0] + b" " + want, i


@pytest.mark.parametrize("label", ["C-33-33", "C-33-64"])
def test_the_inside_slices_of_c_agree_with_filterreads_output(label):
    """the pairs of C whose trims lie inside their reads, and the discarded one, as a batch of their own"""
    case, res = case_named(label)
    L = len(case["reads"][0][1])
    keep = [i for p in range(len(case["reads"]) // 2 - 2) if int(case["to"][2 * p]) + int(case["tl"][2 * p]) <= L for i in (2 * p, 2 * p + 1)]
    assert len(keep) >= 2 * 8 and any(case["af"][0][i] == 2 for i in keep)
    old, twins = through_filterreads_output(case, keep)
    mine = records(res.text)
    assert not twins and records(old) == [mine[i] for i in keep]          # everything up to the last four reads is picked: record i is read i


def test_the_writer_launch_b_longest_is_sized_for():
    """B-longest needs a wavefront to write two picks, so its size follows the writer's grid: at most 8 blocks per CU of SEL_WAVES
    wavefronts, pick p on wavefront p mod the grid's.  The launch and the constants are held to that here."""
    import os
    from helpers import ROOT
    src = os.path.join(ROOT, "kmernator_amd", "csrc")
    stages, select = open(os.path.join(src, "kmr_stages.hip")).read(), open(os.path.join(src, "kmr_select.hpp")).read()
    assert "select_write_kernel, dim3((unsigned)std::min<uint64_t>((pk->n_picked + SEL_WAVES - 1) / SEL_WAVES, (uint64_t)num_cus(h) * 8)), dim3(SEL_THREADS)" in stages
    assert "SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64" in select
    assert "for (uint64_t p = (uint64_t)blockIdx.x * SEL_WAVES + wave; p < n_picked; p += (uint64_t)gridDim.x * SEL_WAVES)" in select
    case, _ = case_named("B-longest")
    assert len(case["reads"]) == 2 * (256 // 64) * 8 * 256


# ---- reach
def test_l_stands_on_the_float_boundary():
    hand = {"L-0.1": [0, 1, 1, 1, 0], "L-0.6": [0, 1, 1, 1, 0], "L-0.4": [0, 1, 1, 1, 0, 1, 0], "L-one": [0, 1, 1, 0, 0, 0],
            "L-above-one": [1, 1, 0, 1, 0], "L-25": [0, 1, 1, 1, 0], "L-zero": [0, 0, 1, 1, 0, 0]}
    assert set(hand) == {c["label"] for c in sc.family("L")}
    for label, flags in hand.items():
        case, res = case_named(label)
        assert res.picked.tolist() == [bool(f) for f in flags], label
    # the three triples of the float / double disagreement: the product in double drops exactly the boundary read
    for label in ("L-0.1", "L-0.6", "L-0.4"):
        case, res = case_named(label)
        assert (res.picked ^ sc.run(case, "product_in_double").picked).tolist()[:3] == [False, True, False], label
    case, _ = case_named("L-above-one")
    assert np.float32(case["cfg"]["min_read_length"]) > np.float32(1.0) and np.float32(case["cfg"]["min_read_length"]) - np.float32(1.0) < 2e-7
    assert case_named("L-one")[0]["cfg"]["min_read_length"] == 1.0


def test_s_stands_on_the_threshold_and_the_halves():
    case, res = case_named("S-threshold")
    assert res.picked.tolist() == [False, True, True, False, False, True, False, True, False]
    assert float(case["sc"][0]) < 2.5 == float(case["sc"][1]) < float(case["sc"][2]) and float(case["sc"][2]) - float(case["sc"][0]) < 1e-6
    # beside a passing mate all nine are printed; four of them under the project's own rule
    case, res = case_named("S-pinned")
    assert res.picked.all()
    shown = [r[0].split(b"MedianScore:")[1] for r in records(res.text)][0::2]
    assert shown == [b"2", b"3", b"3", b"0", b"0", b"2147483647", b"-2147483648", b"2147483647", b"-2147483648"]
    assert [refselect.score_int(s)[1] for s in case["sc"][0::2]] == [True] * 4 + [False] * 5
    for s, name in enumerate(sc.SCORINGS):
        case, res = case_named("S-round-" + name)
        shown = [r[0].split(b" ")[1] for r in records(res.text)]
        assert shown == [refselect.SCORE_LABEL[s] + b":%d" % v for v in (3, 2, 0, 0, 0, 0, 1, 2, 4, 0, 7, 65535)]
    assert {bytes(l) for l in refselect.SCORE_LABEL} == {b"Score", b"MedianScore", b"MinScore", b"MaxScore", b"AvgScore"}


def test_b_prints_every_width_and_the_longest_label():
    widths = {k: set() for k in ("af_min", "af_pos", "af_neg", "to", "tl", "pos", "score_pos", "score_neg")}
    means, inv = set(), set()
    case, res = case_named("B-widths-MEDIAN")
    for r in records(res.text)[0::2]:
        m = re.search(rb" AFTrim:(\d+)\+(-?)(\d+)( (Inv)?Bimodal@(\d+):(\d+)/(\d+))? Trim:(\d+)\+(\d+) MedianScore:(-?)(\d+)$", r[0])
        assert m, r[0]
        widths["af_min"].add(len(m.group(1)))
        widths["af_neg" if m.group(2) else "af_pos"].add(len(m.group(3)))
        widths["to"].add(len(m.group(9)))
        widths["tl"].add(len(m.group(10)))
        widths["score_neg" if m.group(11) else "score_pos"].add(len(m.group(12)))
        if m.group(4):
            widths["pos"].add(len(m.group(6)))
            means.add((int(m.group(7)), int(m.group(8))))
            inv.add((bool(m.group(5)), int(m.group(7)) < int(m.group(8)), int(m.group(7)) == int(m.group(8))))
    assert all(w == set(range(1, 11)) for w in widths.values()), widths
    assert means == set(sc.MEANS) and inv == {(True, True, False), (False, False, False), (False, False, True)}
    assert b"Bimodal@4294967295:1/1" in res.text
    for name in sc.SCORINGS:
        assert case_named("B-widths-" + name)[1].picked.all()
    # the longest label there is: every number at its widest, the negative difference, Inv, the longest name
    case, res = case_named("B-longest")
    G = len(case["reads"]) // 2
    assert G == 4 * 8 * 256 and res.picked.all() and res.n_picked == 2 * G
    recs = records(res.text)
    long_label = b" AFTrim:4294967295+-4294967295 InvBimodal@4294967295:10000/65535 Trim:4294967295+4294967295 MedianScore:-2147483647"
    assert len(long_label) == (8 + 10 + 1 + 11) + (12 + 10 + 1 + 5 + 1 + 5) + (6 + 10 + 1 + 10) + (13 + 11)
    assert all(r == [b"@a" + long_label, b"N", b"+", b'"'] for r in recs[:G]) and all(r == [b"@b MedianScore:5", b"ACGTAC", b"+", b"555555"] for r in recs[G:])
    assert refselect.score_int(case["sc"][0])[1]


def test_g_puts_every_border_on_every_edge_lane():
    for label in ("G-33-33", "G-33-64", "G-64-33", "G-64-64"):
        case, res = case_named(label)
        assert res.picked.all()
        seen, name_lengths = set(), set()
        for r in records(res.text):
            hdr, bl = len(r[0]) + 1, len(r[1])
            assert len(r[3]) == bl and r[0].endswith(b" MedianScore:5")
            name_lengths.add(len(r[0]) - 1 - 14)
            for kind, at in (("header newline", hdr - 1), ("base newline", hdr + bl), ("plus", hdr + bl + 1), ("plus newline", hdr + bl + 2), ("last newline", hdr + 2 * bl + 3)):
                seen.add((kind, at % 64))
        assert seen >= {(k, lane) for k in ("header newline", "base newline", "plus", "plus newline", "last newline") for lane in sc.LANES}, label
        assert name_lengths >= set(sc.NAME_LENGTHS)
        ends = {n[len(n.split(b" ")[0].split(b"\t")[0]):][:1] for n, _, _ in case["reads"]}
        assert ends == {b"", b" ", b"\t"}
        assert b"\t" not in res.text and b" c" not in res.text
    case, res = case_named("G-33-64")
    assert all(min(r[3]) >= 64 + 2 for r in records(res.text))
    case, res = case_named("G-64-33")
    assert all(max(r[3]) <= 33 + 40 for r in records(res.text))
    case, res = case_named("G-fasta")
    seen = set()
    for r in records(res.text, fasta=True):
        assert r[0][:1] == b">"
        seen |= {("header newline", len(r[0]) % 64), ("base newline", (len(r[0]) + 1 + len(r[1])) % 64)}
    assert seen >= {(k, lane) for k in ("header newline", "base newline") for lane in sc.LANES}


def test_c_reaches_every_clamp_and_mask():
    L = 30
    shown = [None, None, None, (10, 20), (0, 30), None, None, None, None, (0, 2), (28, 2), (28, 2), None, None, (2, 28)]
    for label, masked_qual in (("C-33-33", b'"'), ("C-33-64", b"A")):
        case, res = case_named(label)
        recs = records(res.text)
        n = len(shown)
        assert res.picked.tolist() == [True] * (2 * n + 2) + [False] * 4 and len(recs) == 2 * n + 2
        for j, want in enumerate(shown):
            name, seq, qual = case["reads"][2 * j]
            r = recs[2 * j]
            assert r[0] == b"@" + name + b" Trim:%d+%d MedianScore:5" % (case["to"][2 * j], case["tl"][2 * j])
            if want is None:
                assert r[1:] == [b"N", b"+", masked_qual], (label, j)
            else:
                a, k = want
                assert r[1] == seq[a:a + k] and len(r[3]) == k and r[3] == bytes(c + case["cfg"]["out_base"] - 33 for c in qual[a:a + k]), (label, j)
        assert recs[2 * n] == [b"@" + case["reads"][2 * n][0], b"N", b"+", masked_qual]          # discarded: masked and without a label
    case, res = case_named("C-fasta")
    assert [len(r[1]) for r in records(res.text, fasta=True)][0:2 * len(shown):2] == [1 if s is None else s[1] for s in shown]
    assert {int(t) for t in case["to"]} >= {L - 1, L, L + 5} and {int(t) for t in case["tl"]} >= {0, 1, 2}


def test_q_prints_the_reference_quality():
    for label, shift in (("Q-fasta-33-33", 0), ("Q-fasta-33-64", 31), ("Q-fasta-64-33", -31)):
        case, res = case_named(label)
        recs = records(res.text)
        assert res.picked.tolist() == [True] * 7 + [False]
        assert [r[3] for r in recs] == [b"g" * int(t) for t in case["tl"][:7]] and [len(r[1]) for r in recs] == [int(t) for t in case["tl"][:7]]
        assert recs[0][0] == b"@contig0 Trim:0+2 MedianScore:5"
    for label, shift in (("Q-arrays-33-33", 0), ("Q-arrays-33-64", 31)):
        case, res = case_named(label)
        q = [r[2] for r in case["reads"]]
        mv = lambda b: bytes(c + shift for c in b)
        assert res.picked.tolist() == [True] * 7 + [False, True, True]
        got = [r[3] for r in records(res.text)]
        assert got == [b"g" * 20, b"g" * 10,                       # 127 first: no qualities, wherever the slice starts
                       mv(q[2]),                                   # real first: the 127s behind it are bytes like any other
                       b"g" * 6,                                   # the slice starts on a 127
                       mv(q[4][2:9]), mv(q[5][9:14]), mv(q[6]), b"gg", mv(q[9])]
        assert got[4][-1] == 127 + shift and 127 + shift in got[2]
        assert all(r[0] == b"@ Trim:%d+%d MedianScore:5" % (case["to"][i], case["tl"][i]) for r, i in zip(records(res.text), [0, 1, 2, 3, 4, 5, 6, 8, 9]))


def test_p_decides_by_pair_and_files_by_input():
    want = {"P-either": [1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 1], "P-both": [0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0], "P-reads": [1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0],
            "P-reads-base64": [1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0]}
    for label, flags in want.items():
        case, res = case_named(label)
        assert res.picked.tolist() == [bool(f) for f in flags], label
        assert [r[0].split(b" ")[0] for r in records(res.text)] == [b"@r%d" % i for i, f in enumerate(flags) if f]
        assert res.table == [(0, sum(flags), 0, len(res.text))]
    case, res = case_named("P-either-two-inputs")
    assert case["cfg"]["input_starts"] == [0, 5, 14] and res.picked[4] and res.picked[5] and int(case["mate"][4]) == 5          # the border falls inside a picked pair
    assert res.text == case_named("P-either")[1].text
    first = sum(len(b"\n".join(r)) + 1 for r in records(res.text)[:5])
    assert res.table == [(0, 5, 0, first), (5, 6, first, len(res.text) - first)] and res.read_segment.tolist() == [0] * 5 + [1, -1, -1, 1, -1, 1, 1, 1, 1]
    case, res = case_named("P-reads-three-inputs")
    assert res.table[0] == (0, 0, 0, 0) and [t[1] for t in res.table] == [0, 3, 4]
    assert (case_named("P-either")[0]["mate"] == -1).sum() == 2
