"""The directed dump images of tests/dumpcases.py, on the CPU: tests/refdump.py (the two texts restated from the reference's
source) against the oracle's dump on every case, the restatement tied to the reference's own mercount / mergraph files, every
coverage condition of dumpcases asserted on the expected text and offsets alone (so that tests/test_gpu_dump_edges.py tests
the borders it says it does), and every deliberate deviation of refdump.WRONG shown to change some family's expected text."""
import collections
import functools
import os

import pytest

import dumpcases as dc
import refdump as rd
import refimage as ri
from helpers import GOLDEN, KMR_MAP_WEAK, KMR_VALUE_EXT, OracleSpectrum, default_config, read_fastq

DEPTHS = (0, 1, 3, 70000, 0xFFFFFFFF)
TILE = dc.TILE


def oracle(k, kind):
    return OracleSpectrum(default_config(k, value_kind=KMR_VALUE_EXT if kind == "weak_ext" else 0))


def oracle_dump(o, path, min_depth, graph):
    if os.path.exists(path):
        os.remove(path)          # the oracle appends, as the reference does
    o.dump(path, min_depth, graph)
    with open(path, "rb") as f:
        return f.read()


def loaded(image, k, kind):
    import numpy as np
    o = oracle(k, kind)
    o.load_image(KMR_MAP_WEAK, np.frombuffer(image, dtype=np.uint8))
    return o


# ---------------------------------------------------------------------------------------------------------------------- oracle == restatement
@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("k", dc.KS)
def test_oracle_equals_restatement(tmp_path, k, kind, family):
    """The oracle loads the image as the device will hold it (every bucket sorted) and dumps refdump.text, byte for byte, at every
    min depth; it loads the image as stored (shuffled) too and dumps in stored order, as the reference's iterator would"""
    path = str(tmp_path / "dump")
    kb = dc.kb_of(k)
    for case in dc.cases(family, k, kind):
        for image, depths in ((case.sorted_image, DEPTHS), (case.image, (1,))):
            o = loaded(image, k, kind)
            parsed = ri.parse(image, kb, kind)
            for graph in dc.texts_of(case):
                for min_depth in depths:
                    assert oracle_dump(o, path, min_depth, graph) == rd.text(parsed, k, kind, min_depth, graph), (case.name, graph, min_depth)
            o.close()


def test_restatement_reproduces_the_reference_files(tmp_path):
    """1000.fastq at k = 21 with MeraculousCounter's settings, built by the oracle: the sorted lines of refdump.text over its stored
    map are the reference's own phix.mercount.m21 and phix.mergraph.m21.D2; the oracle's dump of the map it just stored (every
    bucket sorted) is refdump.text byte for byte"""
    rb = read_fastq(os.path.join(GOLDEN, "1000.fastq"))
    o = OracleSpectrum(default_config(21, value_kind=KMR_VALUE_EXT, fastq_start_char=64, estimated_raw_kmers=56000, min_weight=0.0, min_quality_score=2))
    o.add_reads(rb)
    o.finalize(2)
    parsed = ri.parse(o.image(KMR_MAP_WEAK).tobytes(), dc.kb_of(21), "weak_ext")
    for graph, gold in ((False, "phix.mercount.m21"), (True, "phix.mergraph.m21.D2")):
        text = rd.text(parsed, 21, "weak_ext", 2, graph)
        with open(os.path.join(GOLDEN, gold)) as f:
            assert sorted(text.decode().splitlines()) == sorted(f.read().splitlines())
        assert text.count(b"\n") == 2 * 5401
        assert oracle_dump(o, str(tmp_path / "dump"), 2, graph) == text


# ---------------------------------------------------------------------------------------------------------------------- coverage
def entries_of(case):
    return [kv for b in case.parsed[2] for kv in b]


def border_entries(off):
    """(border, entry) for every tile border inside the text: the entry e with off[e] <= border < off[e + 1]"""
    out, e = [], 0
    for border in range(TILE, off[-1], TILE):
        while off[e + 1] <= border:
            e += 1
        out.append((border, e))
    return out


@pytest.mark.parametrize("k", dc.KS)
def test_widths_cover_every_number(k):
    case = dc.widths(k, "weak_ext")
    entries = entries_of(case)
    assert len(entries) == dc.widths_entries(k) <= 3000
    assert {v[0] for _, v in entries} == set(dc.COUNTS) and len(dc.VALS) == 20 and {len(str(v)) for v in dc.VALS} == set(range(1, 11))
    for j in range(12):
        assert {v[3][j] for _, v in entries} == set(dc.VALS), j
    assert all(len(set(v[3])) == 12 for _, v in entries)
    n_zero = [v for _, v in entries if not all(v[3][j] for j in dc.N_COLUMNS)]
    assert len(n_zero) == 2          # each N column's own turn at 0
    for kind in dc.KINDS:
        case = dc.widths(k, kind)
        text = rd.text(case.parsed, k, kind, 0, False)
        assert len(text) > 3 * TILE
        assert {len(line.split(b"\t")[1]) for line in text.splitlines()} == {1, 2, 3, 4, 5}
        assert case.nb == 1 and [key for key, _ in case.buckets[0]] != sorted(key for key, _ in case.buckets[0])
    graph = rd.text(dc.widths(k, "weak_ext").parsed, k, "weak_ext", 0, True).splitlines()
    for line in (0, 1):          # in the forward and in the reverse line every column shows every width, 4294967295 and 0 among them
        cols = [row.split(b"\t")[1].split(b" ") for row in graph[line::2]]
        for j in range(12):
            assert {row[j] for row in cols} == {str(v).encode() for v in dc.VALS}, (line, j)
        assert all(len(row) == 13 and row[12] == b"0" for row in cols)
    # the pair to merge: shared keys, and sums that pass 2^16 and 2^32
    for kind in dc.KINDS:
        a, b = (dict(entries_of(dc.widths(k, kind, second))) for second in (False, True))
        shared = set(a) & set(b)
        assert shared and set(b) - set(a) and set(a) - set(b)
        assert any(a[key][0] + b[key][0] > 65535 for key in shared)
        if kind == "weak_ext":
            assert any(x + y > 0xffffffff for key in shared for x, y in zip(a[key][3], b[key][3]))


@pytest.mark.parametrize("k", dc.KS)
def test_keys_cover_the_special_kmers(k):
    case = dc.keys(k, "weak_ext")
    held = {key for key, _ in entries_of(case)}
    marks = case.marks
    assert all(set(g) <= held for g in marks.values())
    assert [rd.fasta(key, k) for key in marks["zero"]] == ["A" * k]
    m = (k & 3) or 1
    assert marks["t_tail"] and all(rd.fasta(key, k).endswith("T" * m) for key in marks["t_tail"])
    assert ("palindrome" in marks) == (k % 2 == 0) and ("ones" in marks) == (k >= 64)
    if k % 2 == 0:
        seq = rd.fasta(marks["palindrome"][0], k)
        assert rd.reverse_complement(seq) == seq
        lines = rd.text(case.parsed, k, "weak_ext", 0, False).splitlines()
        assert any(lines[i] == lines[i + 1] for i in range(0, len(lines), 2))
    if k >= 64:
        assert rd.fasta(marks["ones"][0], k) == "T" * 32 + "A" * (k - 32)
    groups = collections.Counter(rd.fasta(key, k)[:-1] for key in marks["last_base"])
    assert len(groups) == 3 and min(groups.values()) >= 2
    for key in held:          # canonical, by refdump's own reverse complement
        seq = rd.fasta(key, k)
        assert seq <= rd.reverse_complement(seq)
    assert dc.keys(k, "weak").marks == marks


def char_class(line, q, k, graph):
    if q < k:
        return "key"
    if q == k:
        return "tab"
    if q == len(line) - 1:
        return "newline"
    if graph and q == len(line) - 2:
        return "final 0"
    return {True: "digit", False: "blank"}[line[q:q + 1].isdigit()]


@pytest.mark.parametrize("graph", (False, True))
def test_borders_lie_everywhere(graph):
    """over the family a tile border lies at every even offset of an entry of the most common length (offset 0: exactly between two
    entries); every character class of both lines is the last byte of a tile or the first of the next (a reverse line's newline
    lies at an odd offset, so it can only be a tile's last byte); lines start at every residue mod 4 they can: an entry's text is
    even, so a forward line starts at 0 or 2 only"""
    kind = "weak_ext"
    classes, starts = set(), set()
    for k in dc.BORDER_KS:
        L = dc.common_len(k, graph)
        at, lengths = set(), collections.Counter()
        family = dc.borders(k, kind, graph)
        assert len(family) == L // 2
        for case in family:
            assert len(entries_of(case)) <= 3000
            text, off = rd.text(case.parsed, k, kind, 0, graph), rd.offsets(case.parsed, k, kind, 0, graph)
            assert all((y - x) % 2 == 0 and y > x for x, y in zip(off, off[1:]))
            lengths.update(y - x for x, y in zip(off, off[1:]))
            hits = border_entries(off)
            assert len(hits) == 1          # two tiles: with two tiles a block the second learns its first entry from the first
            for border, e in hits:
                if off[e + 1] - off[e] == L:
                    at.add(border - off[e])
                for p in (border - 1, border):          # the last byte of a tile and the first of the next
                    e = max(i for i in range(len(off) - 1) if off[i] <= p)
                    half = (off[e + 1] - off[e]) // 2
                    rev = p - off[e] >= half
                    start = off[e] + (half if rev else 0)
                    classes.add((rev, char_class(text[start:start + half], p - start, k, graph)))
            starts |= {(False, x % 4) for x in off[:-1]} | {(True, (x + (y - x) // 2) % 4) for x, y in zip(off, off[1:])}
        assert lengths.most_common(1)[0][0] == L
        assert at == set(range(0, L, 2)), (k, sorted(set(range(0, L, 2)) - at))
    names = ("key", "tab", "digit", "newline") + (("blank", "final 0") if graph else ())
    assert classes == {(rev, name) for rev in (False, True) for name in names}
    assert starts == {(False, 0), (False, 2)} | {(True, r) for r in range(4)}


@pytest.mark.parametrize("kind,graph", (("weak", False), ("weak_ext", False), ("weak_ext", True)))
@pytest.mark.parametrize("k", dc.KS)
def test_gaps_put_runs_at_borders(k, kind, graph):
    family = dc.gaps(k, kind, graph)
    assert [c.marks["run"] for c in family] == list(dc.RUNS) == [1, 2, 63, 64, 65, 600]
    for case in family:
        entries = entries_of(case)
        n, r = len(entries), case.marks["run"]
        assert n <= 3100
        off = rd.offsets(case.parsed, k, kind, dc.GAP_DEPTH, graph)
        head, at_start, inside, tail = case.marks["runs"]
        dropped = {i for a, b in case.marks["runs"] for i in range(a, b)}
        assert all((off[i + 1] == off[i]) == (i in dropped) for i in range(n))
        assert {entries[i][1][0] for i in dropped} == {1, 2} and min(v[0] for i, (_, v) in enumerate(entries) if i not in dropped) >= 3
        assert head[0] == 0 and tail[1] == n and at_start[1] - at_start[0] == r == inside[1] - inside[0]
        # the first border exactly at the start of the kept entry behind the run, the second inside the kept entry behind the run
        assert off[at_start[0]] == off[at_start[1]] == TILE < off[at_start[1] + 1]
        assert off[inside[0]] == off[inside[1]] < 2 * TILE < off[inside[1] + 1]
        assert 2 * TILE < off[-1] <= 3 * TILE
        for a, b in case.marks["runs"]:          # a range in which nothing is kept
            assert rd.text(case.parsed, k, kind, dc.GAP_DEPTH, graph, a, b) == b""


@pytest.mark.parametrize("kind,graph", (("weak", False), ("weak_ext", False), ("weak_ext", True)))
@pytest.mark.parametrize("k", dc.KS)
def test_exact_totals(k, kind, graph):
    one, two, plus, single = dc.exact(k, kind, graph)
    shortest = dc.entry_len(k, graph, 12 if graph else 1)
    off = {c.name: rd.offsets(c.parsed, k, kind, dc.GAP_DEPTH, graph) for c in (one, two, plus, single)}
    assert off[one.name][-1] == TILE
    o = off[two.name]
    (a, b), = two.marks["runs"]
    assert o[-1] == o[a] == 2 * TILE and b == len(o) - 1 and b - a == 7 and o[a - 1] < 2 * TILE
    assert TILE in o          # and a border between two entries
    o = off[plus.name]
    assert o[-1] == TILE + shortest and o[-2] == TILE
    assert len(off[single.name]) == 2 and 16 <= shortest <= off[single.name][-1]
    assert all(len(entries_of(c)) <= 3000 for c in (one, two, plus, single))
    # no entry can be shorter than `shortest`: one digit a number
    assert shortest == 2 * len(("A" * k + "\t" + ("0 " * 12 + "0" if graph else "0") + "\n"))


@pytest.mark.parametrize("k", dc.KS)
def test_buckets_pin_bucket_major_order(k):
    for kind in dc.KINDS:
        for case in dc.buckets(k, kind):
            nb, _, buckets = case.parsed
            filled = [b for b in buckets if b]
            assert nb > 1 and len(filled) >= 2 and len(filled) < nb
            flat = [key for b in buckets for key, _ in b]
            assert flat != sorted(flat) and all([key for key, _ in b] == sorted(key for key, _ in b) for b in buckets)


# ---------------------------------------------------------------------------------------------------------------------- deviations
# the families whose expected text changes under each deviation, at k = 14 with tallies, over DEPTHS.  In borders, gaps, exact and
# keys the N tallies are 0 as in a map built from reads, so only widths and buckets see the N columns; only buckets has more than
# one bucket; only widths holds count 0, and only widths and gaps hold a count of DEPTHS by design (the others may by chance).
NOTICED_BY = {
    "rc_tallies_unpermuted": set(dc.FAMILIES), "rc_sides_not_swapped": set(dc.FAMILIES), "rc_n_x_swapped": set(dc.FAMILIES),
    "rc_left_n_only": {"widths", "buckets"}, "rc_not_complemented": set(dc.FAMILIES), "rc_not_reversed": set(dc.FAMILIES),
    "strict_min_depth": {"widths", "gaps"}, "unsigned_min_depth": set(dc.FAMILIES), "count_is_direction_bias": set(dc.FAMILIES),
    "stored_order_ignored": {"buckets"}, "no_trailing_zero": set(dc.FAMILIES),
}


@functools.lru_cache(maxsize=None)
def expected_texts(case_id, wrong, depths):
    family, k, kind, i = case_id
    case = dc.cases(family, k, kind)[i]
    parsed = parsed_of(case_id)
    return [rd.text(parsed, k, kind, d, graph, wrong=wrong) for graph in dc.texts_of(case) for d in depths]


@functools.lru_cache(maxsize=None)
def parsed_of(case_id):
    family, k, kind, i = case_id
    return dc.cases(family, k, kind)[i].parsed


def changed(case_id, wrong, depths=None):
    """over every min depth for a deviation of the keep test, at min depth 0 for the others"""
    depths = depths or (DEPTHS if "min_depth" in wrong else (0,))
    return expected_texts(case_id, wrong, depths) != expected_texts(case_id, None, depths)


def test_every_deviation_is_noticed():
    assert set(NOTICED_BY) == set(rd.WRONG)
    noticed = {wrong: set() for wrong in rd.WRONG}
    for family in dc.FAMILIES:
        n = len(dc.cases(family, 14, "weak_ext"))
        ids = [(family, 14, "weak_ext", i) for i in sorted({0, max(0, n - 2)})]          # (the images of a family differ in their layout, not in their kind of content)
        for wrong in rd.WRONG:
            if any(changed(c, wrong) for c in ids):
                noticed[wrong].add(family)
        # count 0 at min depth 0 (kept; a strict test drops it) occurs in widths alone
        assert any(changed(c, "strict_min_depth", (0,)) for c in ids) == (family == "widths"), family
        # the left N column alone misplaced: seen where that column is nonzero, and by nothing built from reads
        if family not in ("widths", "buckets"):
            assert all(not v[3][j] for c in ids for b in parsed_of(c)[2] for _, v in b for j in dc.N_COLUMNS)
    chance = noticed.pop("strict_min_depth")
    assert chance >= NOTICED_BY["strict_min_depth"]
    assert noticed == {w: f for w, f in NOTICED_BY.items() if w != "strict_min_depth"}
    # what a family alone catches: bucket-major order needs more than one bucket
    assert [w for w, f in NOTICED_BY.items() if f == {"buckets"}] == ["stored_order_ignored"]
    # the plain value kind sees the deviations of the mercount line
    for wrong in ("rc_not_complemented", "rc_not_reversed", "strict_min_depth", "unsigned_min_depth", "count_is_direction_bias"):
        assert changed(("widths", 31, "weak", 0), wrong), wrong
