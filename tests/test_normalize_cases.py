"""The restatement of coverage normalization (tests/refnormalize.py) and its directed batches (tests/normalizecases.py) on the
CPU: Philox4x32-10 against known answers, every family of batches against the restatement with one rule changed, batching
invariance, and the sanity of the stream of draws."""
import os
import subprocess

import numpy as np

import normalizecases as nc
from helpers import GOLDEN, ROOT
from refnormalize import Normalizer, draw, file_name, pair_list, philox4x32_10


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox4x32-10 (zeros, ones, digits of pi)"""
    f = 0xffffffff
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox4x32_10((f, f, f, f), (f, f)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    assert draw(0, 0) == 0x6627e8d5 and draw(2 ** 64 - 1, 2 ** 64 - 1) != draw(0, 0)
    # g above 2^32 reaches the second counter word
    assert draw(5, 1 << 32) == philox4x32_10((0, 1, 0, 0), (5, 0))[0] != draw(5, 0)


class Exclusive(Normalizer):
    def draw_keeps(self, choice, target):
        return choice < target


class PerReadOrder(Normalizer):
    def order(self, picks):
        return sorted(x for p in picks for x in p if x >= 0)


class NoBothPassQuirk(Normalizer):
    def both_pass_skips(self, s1, s2):
        return False


class Rounding(Normalizer):
    def score_long(self, score):
        return int(np.floor(float(np.float32(score)) + 0.5))


class GOfRead1(Normalizer):
    def g_of_pair(self, a, b):
        return a if a >= 0 else b


FAMILIES = [
    (lambda: nc.single_reads_over(600), Exclusive),
    (lambda: nc.blocks(70), PerReadOrder),
    (lambda: nc.both_pass_halves(), NoBothPassQuirk),
    (lambda: nc.truncation(), Rounding),
    (lambda: nc.reversed_pairs(), GOfRead1),
    (lambda: nc.interleaved(129), Rounding),
]


def test_every_family_notices_its_deviation():
    for k, (make, mutant) in enumerate(FAMILIES):
        b = make()
        want, got = b.expect(), b.expect(mutant)
        print("%d %-70s %s: %d picks against %d" % (k, b.purpose, mutant.__name__, want["info"]["n_picks"], got["info"]["n_picks"]))
        assert want["text"] != got["text"], (b.purpose, mutant.__name__)
    # interleaved pairs with read1 < read2 are in read order already: the one family the order cannot change
    b = nc.interleaved(129)
    assert b.expect()["text"] == b.expect(PerReadOrder)["text"]


def test_witnesses_of_the_families():
    b = nc.single_reads_over(600)
    e = b.expect()
    kept = set(e["reads"])
    assert all(i in kept for i in b.witness["at_T"]) and not any(i in kept for i in b.witness["at_T_plus_1"])
    assert e["info"] == dict(n_picks=len(kept), n_candidates=b.witness["drawing"], n_draws=b.witness["drawing"]) and b.witness["drawing"] > 590
    b = nc.blocks(70)
    e = b.expect()
    m = 70
    picks = set(e["picks"])
    w = b.witness
    # a reversed pair prints its R2 read first; pairs with a discarded or failed mate are picked whole
    assert any((m + i, i) in picks for i in w["reversed"])
    rd = e["reads"]
    i = next(i for i in w["reversed"] if (m + i, i) in picks)
    assert rd.index(m + i) + 1 == rd.index(i)
    assert any((i, m + i) in picks or (m + i, i) in picks for i in w["discarded_mate"]) and any((i, m + i) in picks or (m + i, i) in picks for i in w["failed_mate"])
    assert any((i, -1) in picks for i in w["half1"]) and any((-1, m + i) in picks for i in w["half2"])
    assert any((x, -1) in picks for x in range(2 * m, b.n))          # an unlisted read
    assert all(t[1] > 0 for t in e["table"])                          # every input takes records
    assert e["info"]["n_draws"] > 20 and e["info"]["n_picks"] < e["info"]["n_candidates"]
    b = nc.both_pass_halves()
    e = b.expect()
    assert not any(e["read_segment"][i] >= 0 for i in b.witness["halves"]) and e["info"]["n_picks"] > 0
    assert all(b.expect(NoBothPassQuirk)["read_segment"][i] >= 0 for i in b.witness["halves"])
    b = nc.truncation()
    e = b.expect()
    assert not any(e["read_segment"][i] >= 0 for i in b.witness["zero"]) and e["info"]["n_draws"] == 0 and e["info"]["n_picks"] == 30
    b = nc.by_read_full_pairs()
    e = b.expect()
    assert any(a < 0 for a, c in e["picks"]) and any(c < 0 for a, c in e["picks"]) and any(a > c >= 0 for a, c in e["picks"])
    b = nc.interleaved(129)
    e = b.expect()
    assert e["read_segment"][128] >= 0 or b.sc[128] > nc.T      # the unlisted last read is a half pair
    assert any(b.disc[i] and e["read_segment"][i] >= 0 for i in range(b.n))      # a discarded mate prints beside its passing mate


def test_batching_invariance_of_the_restatement():
    for b, cut in ((nc.interleaved(129), 64), (nc.single_reads_over(600), 301), (nc.by_read_full_pairs(), 100)):
        whole = b.expect()
        lo, hi = b.half(0, cut), b.half(cut, b.n)
        a, c = lo.expect(), hi.expect()
        assert a["text"] + c["text"] == whole["text"]
        assert [x for x in a["reads"]] + [x + cut for x in c["reads"]] == whole["reads"]
        assert {k: a["info"][k] + c["info"][k] for k in a["info"]} == whole["info"]
    # another seed is another subset
    b = nc.single_reads_over(600)
    assert b.expect()["reads"] != b.expect(seed=8)["reads"]


def test_sanity_of_the_stream():
    """20 000 single reads of score 100 with T = 9 and seed 1: each is kept with probability 10 / 100, so 2 000 are expected with a
    binomial standard deviation of 42; the bound is about 6 of them.  The count is deterministic (2 003 as computed on the CPU when
    the bound was written); the check guards against a stream that is correlated with the index."""
    n = 20000
    kept = [draw(1, g) % 100 <= 9 for g in range(n)]
    total = sum(kept)
    print("kept %d of %d" % (total, n))
    assert 1750 <= total <= 2250
    # and no drift along the index: every fifth of the range holds its share (400 expected, sd 19)
    fifths = [sum(kept[k * 4000:(k + 1) * 4000]) for k in range(5)]
    print("per fifth", fifths)
    assert all(290 <= f <= 510 for f in fifths)


def test_file_names_and_pair_list():
    assert file_name("out", 2, 30, "lib1") == "out-MinDepth2-MaxDepth30-lib1.fastq"
    assert file_name("out", 2, 30, "lib1", fasta=True) == "out-MinDepth2-MaxDepth30-lib1.fasta"
    assert file_name("out", 2, 30, "lib1", separate_outputs=False) == "out"
    assert pair_list(4, [2], [0]) == [(2, 0), (1, -1), (3, -1)] and pair_list(2) == [(0, -1), (1, -1)]


def build_cpp_demo(tmp_path):
    """tests/cpp/normalize_demo.cpp: ReadSelector::selectReadsNormalized of include/kmernator_amd.hpp against the library, warnings as errors"""
    exe = str(tmp_path / "normalize_demo")
    lib_dir = os.path.join(ROOT, "kmernator_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "normalize_demo.cpp"), "-L" + lib_dir, "-lkmernator_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_normalize_demo_compiles_and_links(tmp_path):
    exe = build_cpp_demo(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
