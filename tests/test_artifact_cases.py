"""The artifact filter's independent reference (tests/refartifact.py) and its directed cases (tests/artifactcases.py) on the
CPU: the reference reproduces the reference program's own AFTrim labels, computes the exact-match filter set itself, agrees with
the C++ oracle on every family in everything the device hands out -- and the families are proven to discriminate: for every
deliberate deviation refartifact can switch on, at least 8 reads of the family named for it change.  So the device comparison of
tests/test_gpu_artifact_edges.py cannot pass on cases that do not reach the line they were written for."""
import os
import re

import numpy as np
import pytest

import artifactcases as ac
import refartifact as ra
from helpers import GOLDEN, OracleArtifactFilter, ReadBatch, apply_artifact_result, artifact_config, read_fastq

KEYS = ("value", "min_pass", "max_pass", "action", "remnant_off", "remnant_len")


def fasta(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("fq,start", [("1000.fastq", 64), ("1000.std.fastq", 33)])
def test_reference_reproduces_the_golden_aftrim_labels(fq, start):
    """test/1000-Filtered.fastq (runFilterTests.sh:24,63: edit distance 1 built in, --min-read-length 25): the 51 reads the
    reference program trimmed, their offsets and lengths, and the other 949 untouched"""
    rb = read_fastq(os.path.join(GOLDEN, fq))
    gold = read_fastq(os.path.join(GOLDEN, "1000-Filtered.fastq"))
    kw = dict(edit_distance=1, fastq_start_char=start, min_read_length=25.0)
    o = OracleArtifactFilter(artifact_config(**kw), fasta("artifact_sequences.fa"))
    f = ra.Filter(ra.Config(**kw), fasta("artifact_sequences.fa"), o.entries(), o.info()[2])
    seqs, quals = [rb.seq(i) for i in range(rb.n)], [rb.qual(i) for i in range(rb.n)]
    res, after = f.apply(seqs, quals, names=rb.names)
    n_trim = 0
    for i in range(rb.n):
        m = re.search(rb"AFTrim:(\d+)\+(\d+)", gold.names[i])
        if m:
            n_trim += 1
            lo, ln = int(m.group(1)), int(m.group(2))
            assert (res["action"][i], res["min_pass"][i], res["max_pass"][i] - res["min_pass"][i]) == (1, lo, ln), (i, gold.names[i])
            assert res["value"][i] == f.n_seq == 25
            assert after[0][i] == seqs[i][lo:lo + ln] and after[1][i] == quals[i][lo:lo + ln]
        else:
            assert res["action"][i] == 0 and res["value"][i] == 0, (i, gold.names[i])
            assert after[0][i] == seqs[i] and after[1][i] == quals[i]
        assert after[2][i] == rb.names[i]
    assert n_trim == 51 and len(after[0]) == 1000 and not res["past_buffer"].any()


@pytest.mark.parametrize("kw", [dict(), dict(ac.CLASSES), dict(match_length=12), dict(match_length=20), dict(match_length=28, **ac.CLASSES)])
def test_own_filter_set_of_the_small_table_equals_the_oracles(kw):
    kw = dict(kw, build_edits=0)
    o = OracleArtifactFilter(artifact_config(**kw), ac.FASTA)
    f = ra.Filter(ra.Config(**kw), ac.FASTA)
    ko, vo = o.entries()
    kr, vr = f.entries()
    assert (f.n_seq, len(f.table), f.num_errors) == o.info() and f.n_seq == ac.N_SEQ
    assert np.array_equal(kr, ko) and np.array_equal(vr, vo)
    # the short sequence: 10 bases, 20 once circularised -- no window of 24 or 28
    assert set(vr.tolist()) == set(range(1, ac.N_SEQ)) - ({ac.IDX[b"short"]} if f.length > 20 else set())
    # the reference-class sequence is not circularised, the others are
    n_ref = int((vr == ac.IDX[b"reference"]).sum())
    assert n_ref == (len(ac.REFERENCE) - f.length + 1 if "reference_begin" in kw else len(ac.REFERENCE))
    assert int((vr == ac.IDX[b"poly_a"]).sum()) == 1 and kr[0] == 0


def test_own_filter_set_of_the_reference_table_equals_the_oracles():
    o = OracleArtifactFilter(artifact_config(build_edits=0), fasta("artifact_sequences.fa"))
    f = ra.Filter(ra.Config(build_edits=0), fasta("artifact_sequences.fa"))
    ko, vo = o.entries()
    kr, vr = f.entries()
    assert (f.n_seq, len(f.table), f.num_errors) == o.info()
    assert np.array_equal(kr, ko) and np.array_equal(vr, vo)


def test_tables_and_permutation_order():
    """the two tables as TwoBitSequence.cpp documents them, and __permuteBases' array order and sizes"""
    assert ra.RC_TABLE[0x00] == 0xff and ra.RC_TABLE[0x80] == 0xfd and ra.RC_TABLE[0xfe] == 0x40 and ra.RC_TABLE[0xff] == 0x00
    aaaa = [ra.compress_sequence(s)[0] for s in (b"CAAA", b"GAAA", b"TAAA", b"ACAA", b"AGAA", b"ATAA", b"AACA", b"AAGA", b"AATA", b"AAAC", b"AAAG", b"AAAT")]
    assert ra.PERMUTATIONS[0] == aaaa
    assert ra.PERMUTATIONS[0xff][:3] == [ra.compress_sequence(s)[0] for s in (b"ATTT", b"CTTT", b"GTTT")]
    k = ra.compress_sequence(b"ACGTACGTACGT")
    one, two = ra.permute_bases(k, 1), ra.permute_bases(k, 2)
    assert len(one) == 36 and len(set(one)) == 36 and len(two) == 36 + 9 * 66 and len(set(two)) == len(two)
    assert one[:3] == [ra.compress_sequence(s + b"CGTACGTACGT") for s in (b"C", b"G", b"T")]
    assert two[:3] == one[:3] and two[3:6] == [ra.compress_sequence(b"C" + s + b"GTACGTACGT") for s in (b"A", b"G", b"T")]
    assert ra.compress_sequence(b"acgtNn.R") == ra.compress_sequence(b"ACGTAAAA") and ra.compress_sequence(b"T") == b"\xc0"


@pytest.mark.parametrize("case_id", ac.ids())
def test_oracle_equals_the_reference(case_id):
    """all six arrays and the read set afterwards"""
    c = ac.CASES[case_id]
    b = c.batch()
    res, after = ac.reference(case_id)
    o = OracleArtifactFilter(artifact_config(**c.kw), c.fasta)
    rb = ReadBatch(b.seqs, b.quals)
    want = o.apply(rb, b.mate)
    for key in KEYS:
        bad = np.nonzero(want[key] != res[key])[0]
        assert bad.size == 0, (key, bad[:5], b.tags[bad[0]], b.seqs[bad[0]], b.quals[bad[0]], want[key][bad[:5]], res[key][bad[:5]])
    fr = apply_artifact_result(rb, want)
    assert [fr.seq(i) for i in range(fr.n)] == after[0] and [fr.qual(i) for i in range(fr.n)] == after[1]
    assert b.n <= 10000 and max(len(s) for s in b.seqs) <= (270 if c.family == "layout" else 160)          # the gather's 129 + 1 + 128
    if b.names:
        rem = [i for i in range(b.n) if res["remnant_len"][i]]
        assert after[2] == b.names + [b.names[i] for i in rem] and len(rem) >= 8


def changed(case_id, variant):
    a, v = ac.reference(case_id)[0], ac.reference(case_id, variant)[0]
    diff = np.zeros(a["value"].size, dtype=bool)
    for key in KEYS:
        diff |= a[key] != v[key]
    return int(diff.sum())


@pytest.mark.parametrize("variant", ra.VARIANTS)
def test_the_family_notices_the_deviation(variant):
    case_id = ac.SENSITIVE[variant]
    assert changed(case_id, variant) >= 8, (variant, case_id, changed(case_id, variant))


# what a family can produce: `sides`, `edits` ... hold hits in every read or nearly; only where a family cannot reach an action
# by its construction is it left out here
ACTIONS = {"runs": {0, 1, 2}, "quality": {0, 1, 2}, "windows": {0, 1, 2}, "sides": {1, 2}, "edits": {0, 1, 2}, "classes": {0, 1, 2},
           "pairs": {0, 1, 2}, "short": {0, 1, 2}, "characters": {0, 1, 2}, "layout": {0, 1, 2}}


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_family_has_every_action_and_past_buffer_stays_where_it_belongs(family):
    seen = set()
    for case_id in ac.ids(family):
        b = ac.CASES[case_id].batch()
        res, _ = ac.reference(case_id)
        seen |= set(np.unique(res["action"]).tolist())
        past = np.nonzero(res["past_buffer"])[0]
        for i in past:          # only where the hop clamp fires on a read of 20 bases or fewer with minPass < 4
            assert len(b.seqs[i]) <= 20 and res["screens"][i]["pass0"][0] < 4, (case_id, i)
        if family == "short":
            assert past.size >= 100
        elif family == "layout":          # its filler and empty reads are short reads: nothing else
            assert all(b.tags[i] == "filler" for i in past)
        else:
            assert past.size == 0, (case_id, past[:5])
    assert seen >= ACTIONS[family], (family, seen)


def _screens(case_id):
    return ac.CASES[case_id].batch(), ac.reference(case_id)[0]


def test_runs_hold_the_ties_the_remnants_and_the_f32_product():
    b, res = _screens("runs-mrl0.4")
    assert b.n == sum(1 << L for L in range(13)) + b.tags.count("pin-best") + b.tags.count("pin-best-end") + b.tags.count("pin-second")
    ties = sum(1 for s in res["screens"] if s["pass0"][1] - s["pass0"][0] == s["second"][1] - s["second"][0] > 0)
    assert ties >= 500
    assert (res["remnant_len"] > 0).sum() >= 50 and len(set(res["remnant_off"].tolist())) >= 20
    # a run of exactly L * 0.40 passes in f32 (5 * 0.4f rounds to 2.0f) and would not in f64 (0.4f is a little above 0.4)
    exact = [i for i in range(b.n) if b.tags[i] == "pin-best" and len(b.seqs[i]) % 5 == 0 and res["max_pass"][i] * 5 == 2 * len(b.seqs[i])]
    assert len(exact) >= 25 and all(res["action"][i] == 1 for i in exact)
    assert changed("runs-mrl0.85", "f64_product") >= 8
    # length <= 1: a run of one base is nothing to keep, at any minimum length
    b0, res0 = _screens("runs-mrl0")
    one = [i for i in range(b0.n) if res0["value"][i] and res0["max_pass"][i] - res0["min_pass"][i] == 1]
    assert len(one) >= 100 and all(res0["action"][i] == 2 for i in one)


def test_quality_bytes_sit_on_the_threshold():
    for case_id in ac.ids("quality"):
        c = ac.CASES[case_id]
        thr = (c.kw["fastq_start_char"] + c.kw["min_quality"]) & 0xff
        b, res = _screens(case_id)
        low = lambda x: (x - 256 if x >= 128 else x) < (thr - 256 if thr >= 128 else thr)
        for i in range(b.n):
            if b.tags[i] == "one":
                at = [j for j, x in enumerate(b.quals[i]) if x != 0x7e]
                assert len(at) == 1
                assert (res["value"][i] != 0) == low(b.quals[i][at[0]]), (case_id, i)
        assert changed(case_id, "unsigned_qual") >= 8 and changed(case_id, "min_qual_plus1") >= 8


def test_windows_take_every_residue_and_the_pointer_quirk_books_shifted():
    for case_id in ac.ids("windows"):
        b, res = _screens(case_id)
        scr = res["screens"]
        assert {s["pass0"][0] % 4 for s in scr if s["hits"]} == {0, 1, 2, 3} and {s["pass0"][1] % 4 for s in scr if s["hits"]} == {0, 1, 2, 3}
        assert {len(x) % 4 for x in b.seqs} == {0, 1, 2, 3}
        M = ac.CASES[case_id].kw.get("match_length", 24)
        piece = (ac.AD_A + ac.AD_A)[3:3 + M]
        shifted = sum(1 for i, s in enumerate(scr) if s["hits"] == 1 and s["pass0"][0] >= 4 and s["affected"][0] != b.seqs[i].find(piece))
        assert shifted >= 50, (case_id, shifted)
    for v in ("no_odd_hop", "book_at_window", "pointer_at_min_pass"):
        assert changed("windows-m12", v) >= 8 and changed("windows-m28", v) >= 8


def test_sides_wrap_tie_and_cover():
    b, res = _screens("sides-exact")
    scr = res["screens"]
    hit = [s for s in scr if s["hits"]]
    assert sum(1 for s in hit if s["affected"][0] < s["pass0"][0]) >= 8          # minAffected - minPass wraps
    assert sum(1 for s in hit if s["affected"][1] > s["pass0"][1]) >= 8          # maxPass - maxAffected wraps
    assert sum(1 for s in hit if s["affected"][0] < s["pass0"][0] and s["affected"][1] > s["pass0"][1]) >= 1
    assert sum(1 for s in hit if s["pass0"][0] <= s["affected"][0] and s["affected"][1] <= s["pass0"][1]
               and s["affected"][0] - s["pass0"][0] == s["pass0"][1] - s["affected"][1]) >= 8          # left == right
    pl = (res["max_pass"].astype(np.int64) - res["min_pass"].astype(np.int64))
    assert (pl < 0).sum() >= 8 and (pl == 0).sum() >= 1 and ((res["action"] == 2) & (pl <= 0)).sum() == (pl <= 0).sum()


def test_edits_reach_what_they_should_and_miss_what_the_reference_misses():
    assert len(ac.strand_flips()) >= 20
    for case_id, ed in (("edits-query1", 1), ("edits-query2", 2)):
        b, res = _screens(case_id)
        v = {t: [int(res["value"][i]) for i in range(b.n) if b.tags[i] == t] for t in set(b.tags)}
        a = ac.IDX[b"adapter_a"]
        assert set(v["exact"] + v["exact-rc"]) == {a}
        x, n_one = b.seqs[0][4:28], 0
        for i in range(b.n):          # one substitution is found unless it flips the canonical strand
            if b.tags[i] in ("one", "one-rc") and ed == 1:
                piece, orig = b.seqs[i][4:28], (x if b.tags[i] == "one" else ac.revcomp(x))
                assert (res["value"][i] == a) == (ac._fwd_is_least(piece) == ac._fwd_is_least(orig)) and res["value"][i] in (0, a), (i, piece)
                n_one += res["value"][i] == a
        assert ed == 2 or n_one >= 120
        two = v["two"] + v["two-rc"]          # two substitutions: out of reach with one edit, found with two unless the strand flips
        assert set(two) == ({0} if ed == 1 else {0, a}) and (ed == 1 or two.count(a) >= 16) and set(v["three"] + v["three-rc"]) == {0}
        assert len(v["one"]) >= (72 if ed == 1 else 24) and len(v["two"]) == 16
        if ed == 1:          # one substitution that flips the canonical strand is out of reach without re-canonicalising
            assert len(v["flip"]) >= 20 and set(v["flip"]) == {0}
            flips = [i for i in range(b.n) if b.tags[i] == "flip"]
            rec = ac.reference(case_id, "recanonicalise")[0]
            assert all(rec["value"][i] != 0 for i in flips)
            # one substitution from adapter_a and one from adapter_b: the later key in permutation order names the value
            near = [i for i in range(b.n) if b.tags[i].startswith("near")]
            first = ac.reference(case_id, "first_hit")[0]
            assert len(near) >= 28 and sum(1 for i in near if res["screens"][i]["hits"] >= 2) >= 28          # (where a strand flips, one is missed)
            assert {int(res["value"][i]) for i in near} == {a, a + 1} and sum(1 for i in near if first["value"][i] != res["value"][i]) >= 20


def test_classes_hold_the_margins_and_the_overrides():
    b, res = _screens("classes-exact")
    scr = res["screens"]
    left = lambda s: s["affected"][0] - s["pass0"][0]
    right = lambda s: s["pass0"][1] - s["affected"][1]
    for m, forgiven in ((35, False), (36, True), (37, True)):
        for side, other in ((left, right), (right, left)):
            at = [i for i in range(b.n) if b.tags[i] == "margin" and side(scr[i]) == m and other(scr[i]) >= 36]
            assert len(at) >= 8, (m, len(at))
            assert all((not 6 <= res["value"][i] < 8) == forgiven for i in at)          # forgiven: 0, or nSeq where a quality trim remains
    by = lambda t: [i for i in range(b.n) if b.tags[i] == t]
    P, R, n = ac.CLASSES["phix_idx"], ac.CLASSES["reference_begin"], ac.N_SEQ
    assert all(res["value"][i] == 0 and res["action"][i] == 0 for i in by("adapter-then-repeat"))
    assert all(res["value"][i] == ac.IDX[b"adapter_c"] and res["action"][i] == 1 for i in by("repeat-then-adapter"))
    for t in ("phix-then-adapter", "phix-then-repeat", "repeat-then-phix"):
        assert all(res["value"][i] == P and res["action"][i] == 2 for i in by(t))
    assert all(res["value"][i] == R and res["action"][i] == 2 for i in by("reference"))
    assert all(res["value"][i] == 0 for i in by("reference-wrap") + by("short-sequence"))
    assert all(res["value"][i] == ac.IDX[b"adapter_c"] and res["action"][i] == 1 for i in by("adapter-wrap"))
    assert all(res["value"][i] == n and res["action"][i] == 1 for i in by("quality-only"))          # value == nSeq >= reference_begin: exempt


def test_pairs_hold_every_combination():
    b, res = _screens("pairs-mrl0.4")
    combos = {t for t in b.tags if not t.endswith("|")}
    singles = [t for t in b.tags if t.endswith("|")]
    assert combos == {x + "|" + y for x in ac.KINDS for y in ac.KINDS} and {t[:-1] for t in singles} == set(ac.KINDS) and (b.mate < 0).sum() == len(singles)
    alone = ac.reference_filter("pairs-mrl0.4").apply(b.seqs, b.quals)[0]
    P = ac.CLASSES["phix_idx"]
    for i in range(b.n):
        mine, mates = (b.tags[i].split("|") + [""])[:2]
        if "phix" in (mine, mates):
            assert res["action"][i] == 2
        elif mates == "reference" and mine in ("quality", "adapter"):
            assert res["action"][i] == 2 and alone["action"][i] == 1          # trimmed on its own, discarded for its mate's reference hit
        elif mine in ("clean", "repeat"):
            assert res["action"][i] == 0
        assert res["value"][i] == alone["value"][i] and (res["value"][i] == P) == (mine == "phix")


def test_short_reads_and_their_neighbours():
    for case_id, ed in (("short-query0", 0), ("short-query1", 1), ("short-query2", 2)):
        b, res = _screens(case_id)
        a = ac.IDX[b"poly_a"]
        for i in range(b.n):
            s = res["screens"][i]
            L, tag = len(b.seqs[i]), b.tags[i]
            if tag.startswith("poly-a") and L <= 20:          # the zeros behind the read complete the all-A sequence
                edits = {"poly-a": 0, "poly-a-1": 1, "poly-a-2": 2}[tag]
                looked = s["pass0"][0] < 4
                assert (s["hits"] > 0) == (looked and edits <= ed), (case_id, i, b.seqs[i], b.quals[i])
                assert not s["hits"] or res["value"][i] == a
                assert s["past_buffer"] == looked
            if tag == "between":          # what lies behind it in the array would complete a window of adapter_c; the zeros do not
                c = ac.IDX[b"adapter_c"]
                assert res["value"][i] != c and b.tags[i + 1] == "after", (case_id, i)
                seen = ac.reference_filter(case_id).screen(b.seqs[i] + b.seqs[i + 1][:24 - L], b"I" * 24)
                assert seen["value"] == c
        assert {len(x) for x in b.seqs} >= set(range(25)) and {s["pass0"][0] for s in res["screens"]} >= set(range(6))
    assert changed("short-query1", "past_nonzero") >= 8


def test_characters_pack_as_a():
    b, res = _screens("characters-exact")
    a = ac.IDX[b"adapter_a"]
    for i in range(b.n):
        t = b.tags[i]
        if t.startswith(("lower", "half")) or t in ("in-A", "outside"):
            assert res["screens"][i]["hits"] and res["value"][i] == a, (i, t, b.seqs[i])
        elif t == "in-other":          # an A where adapter_b has one makes it adapter_b's window
            assert res["value"][i] in (0, a + 1)
        elif t in ("all-N", "all-dot"):
            assert res["value"][i] == ac.IDX[b"poly_a"]
    assert b.tags.count("in-A") >= 8 and sum(1 for i in range(b.n) if b.tags[i] == "in-other" and res["value"][i] == 0) >= 40
    b1, res1 = _screens("characters-built1")
    assert all(res1["value"][i] in (a, a + 1) for i in range(b1.n) if b1.tags[i] == "in-other")


def test_layout_meets_every_residue_and_border():
    starts = {}
    for f in range(8):
        b, res = _screens("layout-filler%d" % f)
        off = np.concatenate([[0], np.cumsum([len(s) for s in b.seqs])])
        assert len(b.seqs[0]) == f and b.n >= 100
        for i in range(1, b.n):
            starts.setdefault(i, set()).add(int(off[i]) % 8)
        trims = {(int(off[i]) + int(res["min_pass"][i])) % 8 for i in range(b.n) if res["action"][i] == 1}
        rems = {(int(off[i]) + int(res["remnant_off"][i])) % 8 for i in range(b.n) if res["remnant_len"][i]}
        assert trims == set(range(8)) and rems == set(range(8))
    assert all(v == set(range(8)) for v in starts.values())
    assert [ac.CASES["layout-count%d" % n].batch().n for n in (255, 256, 257)] == [255, 256, 257]
    b = ac.CASES["layout-count257"].batch()
    assert [len(b.seqs[i]) for i in (0, 128, 256)] == [0, 0, 0] and len(ac.CASES["layout-count256"].batch().seqs[-1]) > 0
    b, res = _screens("layout-gather0")
    kept = set((res["max_pass"] - res["min_pass"])[res["action"] == 1].tolist()) | set(res["remnant_len"][res["remnant_len"] > 0].tolist())
    assert kept >= {63, 64, 65, 127, 128, 129}
    assert b.tags.count("gather-right") == 12 and all(res["min_pass"][i] > 0 and res["value"][i] == ac.IDX[b"adapter_c"] for i in range(b.n) if b.tags[i] == "gather-right")
    b = ac.CASES["layout-names0"].batch()
    assert len(set(b.names)) == b.n and b.fastq().count(b"\n") == 4 * b.n
