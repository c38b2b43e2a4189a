"""The directed cases of the duplicate-fragment collapse (tests/dedupcases.py) against the restatement (tests/refdedup.py) on the
CPU: every case changes under each deviation it is written to notice, every deviation refdedup can switch on is noticed by a named
family, and every family reaches the edge it is aimed at -- conditions on the inputs, so the device comparison of
tests/test_gpu_dedup_edges.py cannot pass on cases that miss their line.  Without a deviation refdedup is what it was: the hand
cases and the reference's consensus fixtures of tests/test_dedup_restatement.py stay as they are and are run there."""
import functools

import pytest

import dedupcases as dc
import refdedup

# which family is answerable for which deviation (test_every_deviation_has_a_family holds the list complete)
ANSWERS = {
    "key_window_shifted": "G", "x_before_window_ignored": "G", "n_is_its_own_code": "G", "last_key_word_ignored": "K",
    "canonical_first_word_only": "K", "canonical_tie_takes_reverse": "K", "members_not_in_pair_order": "K", "flip_sides_not_swapped": "F",
    "name_of_unflipped_first_read": "F", "low_quality_skips": "S", "no_floor": "Q", "ref_qual_not_one": "Q", "count_is_int": "W",
    "copy_does_not_raise_top": "D", "set_top_not_strict": "D", "tree_not_strict": "D", "get_ignores_best": "D", "qual_rounds": "Q",
    "forty_from_0_9999_off": "Q", "name_cut_at_blank_only": "F", "count_digits_fixed": "F", "groups_in_key_order": "K", "cutoff_three": "P",
    "pair_short_counted_twice": "P",
}


@functools.lru_cache(maxsize=None)
def base(family, index):
    return dc.run(dc.family(family)[index])


def _cases():
    return [(f, i) for f in dc.FAMILIES for i in range(len(dc.family(f)))]


@pytest.mark.parametrize("family,index", _cases(), ids=[c[0] for f in dc.FAMILIES for c in dc.family(f)])
def test_the_case_notices_its_deviations(family, index):
    case = dc.family(family)[index]
    want = dc.signature(base(family, index))
    for d in case[5]:
        assert dc.signature(dc.run(case, d)) != want, (case[0], d)


def test_every_deviation_has_a_family():
    assert set(ANSWERS) == set(refdedup.DEVIATIONS) and len(refdedup.DEVIATIONS) == 24
    for d, f in ANSWERS.items():
        assert any(d in c[5] for c in dc.family(f)), (d, f)
    for f in dc.FAMILIES:          # labels are what the device test's ids are made of
        labels = [c[0] for c in dc.family(f)]
        assert len(set(labels)) == len(labels) and all(l.startswith(f + "-") for l in labels)


def test_a_set_of_deviations_and_an_unknown_name():
    case = dc.family("P")[0]
    both = dc.signature(dc.run(case, {"cutoff_three", "pair_short_counted_twice"}))
    assert both != dc.signature(dc.run(case, "cutoff_three")) and both != dc.signature(dc.run(case, "pair_short_counted_twice"))
    with pytest.raises(AssertionError):
        dc.run(case, "no_such_rule")


# ---- reach
def _out_quals(family, min_q):
    seen = set()
    for i, c in enumerate(dc.family(family)):
        if c[4]["min_quality_score"] == min_q:
            for r in base(family, i):
                seen |= {ord(ch) - c[4]["fastq_start_char"] for _, _, q in r.consensus for ch in q}
    return seen


def test_q_and_d_produce_every_output_quality():
    """0 and 3 .. 40 under the default minimum, 1 under minimum 0.  2 cannot come out of integer input qualities: it needs a value
    in [step(2), 1 - 10^-0.3).  What getQualChar is handed is a sum or `top`, a sum that was the largest once.  A sum that wins
    holds at least one observation's probability: with a second observed base in it, it is at least 0.2501 + (1 - 0.2501) / 3 > 0.5;
    alone it is 1 - 10^(-q/10), which for q = 2 lies just below the step (the restatement answers 1) and for q = 3 is the upper end,
    or the floor 0.2501 (quality 1).  Nothing falls between."""
    default = _out_quals("Q", 3) | _out_quals("D", 3)
    assert default == {0} | set(range(3, 41)), sorted(default ^ ({0} | set(range(3, 41))))
    assert _out_quals("Q", 0) >= {1} and _out_quals("Q", 1) >= {1}
    assert 2 not in default | _out_quals("Q", 0) | _out_quals("Q", 1) | _out_quals("Q", 10)
    assert refdedup.get_qual_char(1.0 - 10 ** -0.2, 0) == 1 and refdedup.get_qual_char(0.2501, 0) == 1 and refdedup.get_qual_char(1.0 - 10 ** -0.3, 0) == 3


def test_q_sits_on_the_steps():
    """the restatement answers q - 1 at the qualities whose probability falls just below its step, q elsewhere, 40 from Q40 on"""
    below = {2, 5, 11, 13, 14, 17, 20, 21, 22, 23, 25, 28, 29, 30, 34, 36, 38, 39}
    for i, c in enumerate(dc.family("Q")):
        min_q, start = c[4]["min_quality_score"], c[4]["fastq_start_char"]
        qb = dc.Q_bytes(min_q, start)
        assert {start + 41, start + 42, 102, 103, 126, 127, 255} <= set(qb) and qb[0] == start + min_q
        (res,) = base("Q", i)
        (name, bases, quals), = res.consensus
        assert name == "C2-" and bases == "ACGTACGT" + "A" * len(qb) and res.groups == [(0, 2)]
        for byte, ch in zip(qb, quals[8:]):
            q, got = byte - start, ord(ch) - start
            want = 40 if (q >= 40 or byte >= 103) else (1 if q < 2 else (q - 1 if q in below else q))
            assert got == want, (c[0], byte, got, want)


def test_d_holds_every_pair_of_qualities_and_every_tie():
    grid, ties = dc.family("D")
    for q1 in dc.D_QUALS:
        r1 = [r for r in grid[1] if r[0] == "d%d-0/1" % (q1 - 3)][0]
        r2 = [r for r in grid[1] if r[0] == "d%d-1/1" % (q1 - 3)][0]
        assert r1[1][8:] == "A" * 39 and r2[1][8:] == "C" * 39 and r1[2][8:] == chr(33 + q1) * 39 and r2[2][8:] == "".join(chr(33 + q) for q in dc.D_QUALS)
    res, = base("D", 0)
    assert len(res.groups) == 39 + 6 and [m for _, m in res.groups] == [2] * 39 + [3] * 6
    # the tie tree keeps the later letter: of two members at equal quality the consensus shows the larger base, whoever came first
    res, = base("D", 1)
    pairs = [(a, b) for a in "ACGT" for b in "ACGT" if a != b]
    shown = res.consensus[0][1][8:]
    assert len(shown) == 3 * len(pairs) + 2 and all(shown[i] == max(pairs[i % 12]) for i in range(36)) and shown[36:] == "TT"
    assert res.consensus[0][2][-2:] == "!!"
    # three members: p + o + o, o + p + o and o + o + p are one number only where the rounding allows (Q3 and Q40 here); at Q20 the
    # order of the additions decides the base, which the device has to repeat
    triples = [(a, b, c) for a in "ACGT" for b in "ACGT" for c in "ACGT" if len({a, b, c}) == 3]
    shown = res.consensus[2][1][8:]
    assert len(shown) == 3 * 24 and all(shown[i] in triples[i % 24] for i in range(72))
    assert all(shown[i] == max(triples[i % 24]) for i in list(range(24)) + list(range(48, 72)))
    assert sum(1 for i in range(24, 48) if shown[i] != max(triples[i % 24])) >= 8
    assert len(res.consensus[4][1][8:]) == 12 and set(res.consensus[4][1][8:11]) != {"T"}


def test_g_has_a_group_a_neighbour_and_a_short_record_everywhere():
    cases = dc.family("G")
    assert len(cases) == 16 * 4 * 2 and {(c[3]["dedup_length"], c[3]["start_offset"], c[3]["dedup_mode"]) for c in cases} == {(L, so, m) for L in dc.LENGTHS for so in dc.OFFSETS for m in (1, 2)}
    for i, c in enumerate(cases):
        n_records = len(dc.pair_list(c))
        assert 40 <= n_records <= 60
        for res in base("G", i):
            members = sum(m for _, m in res.groups)
            candidates = n_records - sum(res.skipped)
            assert res.groups and max(m for _, m in res.groups) >= 5, c[0]          # the kept group
            assert candidates - members >= 3, c[0]                                # neighbours with keys of their own
            assert res.skipped[1] >= (5 if c[3]["start_offset"] else 3) and res.skipped[2] > 0 and res.skipped[0] == res.skipped[3] == 0, c[0]
        paired = base("G", i)[0]
        assert paired.flipped > 0 if c[3]["dedup_mode"] == 2 else paired.flipped == 0


def _words(key_str):
    b = refdedup.key_bytes(refdedup.two_bit(key_str))
    return [b[i:i + 8] for i in range(0, len(b), 8)]


def test_k_really_ties_in_the_stated_words():
    for L in dc.K_LENGTHS:
        ties = dc.K_ties(L)
        assert {w for w, _, _ in ties} == ({0} if L == 20 else {0, 1})          # agreement over half the key is equality
        for w, forward_less, key in ties:
            assert len(key) == 2 * L
            f, r = _words(key), _words(dc.revcomp(key))
            assert f[:w] == r[:w] and f[w] != r[w] and (f[w] < r[w]) == forward_less, (L, w)
        mode2 = [c for c in dc.family("K") if c[3]["dedup_length"] == L and c[3]["dedup_mode"] == 2][0]
        res = dc.run(mode2)[0]
        by_first = {mode2[1][2 * pos][0]: m for pos, m in res.groups}
        # every tie fragment given as (A, B) and (B, A) is one group of two; the palindrome is one and nobody in it is flipped
        assert sum(1 for name, m in by_first.items() if "-tie" in name and m == 2) == len(ties)
        pal = [(pos, m) for pos, m in res.groups if "-pal/" in mode2[1][2 * pos][0]]
        assert len(pal) == 1
        a, b = mode2[1][2 * pal[0][0]][1][:L], mode2[1][2 * pal[0][0] + 1][1][:L]
        assert dc.key_of(a, b, L) == dc.revcomp(dc.key_of(a, b, L))
        # one-base neighbours at both ends of every word are groups of their own, in mode 1 too
        W = (2 * L + 31) // 32
        assert sum(1 for name in by_first if "-w" in name) == 2 * W and sum(1 for name in by_first if "-inter" in name) == 4
        firsts = [pos for pos, _ in res.groups]
        assert firsts == sorted(firsts) and firsts[:4] == [0, 1, 2, 3]


def test_w_gives_the_three_qualities():
    for i, c in enumerate(dc.family("W")):
        res, = base("W", i)
        m = len(c[1]) // 2
        assert res.groups == [(0, m)] and res.affected == 2 * m
        want = "I" if c[0].endswith("early-A") else dc.W_QUALS[m]
        assert res.consensus[0] == ("C%d-w0/1" % m, "ACGTA", "IIII" + want) and res.consensus[1] == ("C%d-w0/2" % m, "TTGCA", "IIIII")
    assert dc.W_QUALS == {32767: "$", 32768: ";", 65537: "$"}


def test_s_has_a_position_nobody_observes():
    named, chars = dc.family("S")
    res, = base("S", 0)
    by_name = {n: (b, q) for n, b, q in res.consensus}
    assert by_name["C3-dark0/1"] == ("GATTACTTTTTT", "IIIIII!!!!!!")          # all four sums 0: T at quality 0
    assert by_name["C3-dark0/2"] == ("T" * 10, "!" * 10)
    b, q = by_name["C8-len0/1"]
    assert len(b) == 200 and len(by_name["C8-len0/2"][0]) == 200
    assert sorted(len(r[1]) for r in named[1] if r[0].startswith("len") and r[0].endswith("/1")) == sorted(dc.S_LENGTHS)
    stops = {r[2].find("#") for r in named[1] if r[0].startswith("stop") and r[0].endswith("/1")}
    assert stops == {0, 63, 64, 65, 129, -1}
    res, = base("S", 1)
    assert res.groups == [(0, 6)] and res.skipped == [0, 1, 0, 0]          # lower case and N inside the window group; an x inside it ends the read, one behind it does not


def test_f_reaches_flips_names_and_digits():
    flips = dc.family("F")[0]
    res, = base("F", 0)
    assert len(res.groups) == 4 and res.flipped == 8
    first_flipped = [dc.signature(dc.run(flips, "name_of_unflipped_first_read"))[0][4][2 * g][0] != res.consensus[2 * g][0] for g in range(4)]
    assert any(first_flipped) and not all(first_flipped)
    for i in (1, 2):
        c = dc.family("F")[i]
        paired, single = base("F", i)
        assert [n for n, _, _ in paired.consensus] == ["C2-cas0", "C2-cas0"]
        names = [n for n, _, _ in single.consensus]
        sc = c[3]["store_comment"]
        assert names[:4] == ["C2-b%d" % sc, "C2-t%d" % sc, "C2-bt%d" % sc, "C2-tb%d" % sc]
        assert [len(n) - 3 for n in names[4:]] == list(dc.F_NAME_LENGTHS)
    res, = base("F", 3)
    assert [m for _, m in res.groups] == list(dc.F_SIZES)
    res, = base("F", 4)
    assert [n for n, _, _ in res.consensus] == ["C3-"]


def test_p_counts_each_skip_once():
    for i in (0, 1):
        paired, single = base("P", i)
        assert paired.skipped == [5, 3, 9, 0] and paired.groups == [(0, 4)]
        # the single pass: the pairs are not its business; the discarded half pair and the short one are counted, three groups form
        assert single.skipped == [1, 1, 12, 0] and [m for _, m in single.groups] == [3, 2, 2]
        pl = dc.pair_list(dc.family("P")[i])
        assert sum(1 for a, b in pl if a == dc.NONE) == 3 and sum(1 for a, b in pl if b == dc.NONE) == 6


def test_m_holds_more_tasks_than_two_grids():
    for c, sides in zip(dc.family("M"), (2, 1)):
        res, = dc.run(c)
        tasks = len(res.groups) * sides
        assert tasks > 2 * 8 * 256 * 4 and len(res.groups) == dc.M_groups(256, sides) and all(m == 2 for _, m in res.groups)
    assert dc.M_groups(304, 1) <= 65536          # the keys of 8 bases suffice for any CU count in sight
