"""kmr_dump_text, kmr_dump_text_size, kmr_text_info, kmr_dump_mercount and kmr_dump_mergraph on the directed images of
tests/dumpcases.py, held to tests/refdump.py byte for byte (tests/test_dump_cases.py holds the oracle to the same restatement and
asserts on the expected text that every border named below is there).  Every case uses a fresh handle of its k and value kind,
loads its image and builds nothing; the largest image holds about three thousand entries.

What runs where in kmr_dump.hpp (a tile is 32 KiB of the text; kmr_tune "dump_tiles_per_block" = t):
  bisection               t = 0 and t = 1: every block finds its first entry by bisection over the offsets (the default gives one
                          tile a block up to 128 MiB of text)
  tile-to-tile hand-off   t = 2, 3 and t above the number of tiles (one block walks the whole text): every later tile of a block learns
                          its first entry from the lane that met the entry across the border (s_first[par ^ 1]); asserted from
                          kmr_build_info "dump_blocks" < tiles wherever the text has more than one tile
  put_dec's `hi` half     `widths`: every tally column takes 99999999 .. 4294967295 (8 to 10 digits and the separator), at every byte
                          phase of the line
  both N columns          `widths` and `buckets`: nonzero N tallies, so the reverse line's whole permutation is seen
  count 0                 `widths` at min depth 0 and 0xFFFFFFFF
  borders everywhere      `borders`: the first tile border at every even offset of an entry (0: between two entries), of both lines
  not-kept runs           `gaps` at min depth 3: a border at the start of, and inside, a kept entry behind 1, 2, 63, 64, 65 and 600
                          entries without bytes (o1 == o0), runs at the head and the end of the map, ranges with nothing kept
  exact-tile totals       `exact`: the `pos < total` guard and the 16-byte pad at a text of exactly one and two tiles
An entry's text is even (two lines of one length), so no border lies at an odd offset of an entry."""
import numpy as np
import pytest

import dumpcases as dc
import kmernator_amd as ka
import refdump as rd
import refimage as ri
from helpers import KMR_MAP_WEAK, KMR_VALUE_EXT

pytestmark = pytest.mark.gpu

TILE = dc.TILE
ALL_TILES = 1000          # more tiles a block than any text here has
TILES_PER_BLOCK = (0, 1, 2, 3, ALL_TILES)
DEPTHS = {"widths": (0, 1, 3, 70000, 0xFFFFFFFF), "keys": (0, 0xFFFFFFFF), "borders": (0,), "gaps": (dc.GAP_DEPTH, 0), "exact": (dc.GAP_DEPTH,),
          "buckets": (0, 3, 1000)}
SHAPES = [(k, kind, graph) for k in dc.KS for kind in dc.KINDS for graph in dc.graphs_of(kind)]


def handle(k, kind):
    return ka.KmerSpectrum(ka.default_config(k, device=0, value_kind=KMR_VALUE_EXT if kind == "weak_ext" else 0))


def as_array(image):
    return np.frombuffer(bytes(image), dtype=np.uint8)


def loaded(case):
    sp = handle(case.k, case.kind)
    sp.load_image(KMR_MAP_WEAK, as_array(case.image))
    return sp


def device_text(sp, min_depth, graph, lo=0, hi=None):
    """the text through kmr_dump_text, with kmr_dump_text_size == kmr_text_info == the real length checked on the way"""
    kept, nbytes = sp.dumpTextSize("mergraph" if graph else "mercount", min_depth, lo, hi)
    with (sp.dumpGraphsText if graph else sp.dumpCountsText)(min_depth, lo, hi) as t:
        assert (t.kept, t.bytes) == (kept, nbytes)
        text = t.numpy().tobytes()
    assert len(text) == nbytes
    return text, kept


def tiles_of(nbytes):
    return -(-nbytes // TILE)


def check_text(sp, parts, min_depth, graph, what, lo=0, hi=None, tiles_per_block=TILES_PER_BLOCK):
    """the text of the entries [lo, hi) under every setting of the knob; parts = refdump.pieces of the whole map (an entry's text
    does not depend on the range it is asked in).  Returns the text"""
    parts = parts[lo:hi]
    want = b"".join(parts)
    for t in tiles_per_block:
        sp.tune(dump_tiles_per_block=t)
        got, kept = device_text(sp, min_depth, graph, lo, hi)
        assert got == want, (what, graph, min_depth, lo, hi, t)
        assert kept == sum(1 for p in parts if p), (what, graph, min_depth, lo, hi, t)
        if want:
            tiles, per_block = tiles_of(len(want)), t or 1
            assert int(sp.build_info("dump_tiles_per_block")) == per_block and int(sp.build_info("dump_blocks")) == -(-tiles // per_block)
            if t >= 2 and tiles >= 2:
                assert int(sp.build_info("dump_blocks")) < tiles          # the hand-off ran
    sp.tune(dump_tiles_per_block=0)
    return want


def check_case(case, depths):
    sp, parsed = loaded(case), case.parsed
    for graph in dc.texts_of(case):
        for min_depth in depths:
            check_text(sp, rd.pieces(parsed, case.k, case.kind, min_depth, graph), min_depth, graph, case.name)
    return sp, parsed


# ---------------------------------------------------------------------------------------------------------------------- whole texts
@pytest.mark.parametrize("family", ("widths", "keys", "buckets"))
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("k", dc.KS)
def test_whole_text(k, kind, family):
    for case in dc.cases(family, k, kind):
        sp, parsed = check_case(case, DEPTHS[family])
        if family == "widths":          # three borders or more: one block of three tiles and a rest, two of two, one of all
            assert tiles_of(len(rd.text(parsed, k, kind, 0, False))) >= 4
        sp.close()


@pytest.mark.parametrize("k,kind,graph", SHAPES)
def test_exact_totals(k, kind, graph):
    for case in dc.exact(k, kind, graph):
        check_case(case, DEPTHS["exact"])[0].close()


def cuts_next_to_borders(off):
    """the entries next to every tile border of the text with these offsets: the entry the border lies in or in front of, and the
    one behind it"""
    out, e = set(), 0
    for border in range(TILE, off[-1], TILE):
        while off[e + 1] <= border:
            e += 1
        out |= {e, e + 1}
    return out


def check_ranges(sp, parsed, k, kind, min_depth, graph, cuts, what):
    """every cut of the map into two ranges at an entry of `cuts`, and that entry as a range of its own; the pieces concatenate to
    the whole text.  Both ranges under every setting of the knob (a range's text starts at its first entry, so its borders lie
    elsewhere than the whole text's); the single entry is less than a tile"""
    parts = rd.pieces(parsed, k, kind, min_depth, graph)
    n, whole = len(parts), b"".join(parts)
    assert whole == rd.text(parsed, k, kind, min_depth, graph)
    for c in sorted(x for x in cuts if 0 <= x <= n):
        head = check_text(sp, parts, min_depth, graph, what, 0, c)
        tail = check_text(sp, parts, min_depth, graph, what, c, None)
        assert head + tail == whole
        if c < n:
            one = check_text(sp, parts, min_depth, graph, what, c, c + 1, (0,))
            assert tail.startswith(one)


@pytest.mark.parametrize("k,kind,graph", [s for s in SHAPES if s[0] in dc.BORDER_KS])
def test_borders(k, kind, graph):
    """the first border at every even offset of an entry: whole texts under every setting of the knob, and the cuts next to the
    border"""
    for case in dc.borders(k, kind, graph):
        sp, parsed = check_case(case, DEPTHS["borders"])
        off = rd.offsets(parsed, k, kind, 0, graph)
        assert tiles_of(off[-1]) == 2
        check_ranges(sp, parsed, k, kind, 0, graph, cuts_next_to_borders(off), case.name)
        sp.close()


@pytest.mark.parametrize("k,kind,graph", SHAPES)
def test_gaps(k, kind, graph):
    """runs of entries that are not kept in front of a border: whole texts, the cuts next to every border and at both ends of every
    run, and every run as a range in which nothing is kept"""
    for case in dc.gaps(k, kind, graph):
        sp, parsed = check_case(case, DEPTHS["gaps"])
        off = rd.offsets(parsed, k, kind, dc.GAP_DEPTH, graph)
        assert tiles_of(off[-1]) == 3
        cuts = cuts_next_to_borders(off) | {x for run in case.marks["runs"] for x in run}
        check_ranges(sp, parsed, k, kind, dc.GAP_DEPTH, graph, cuts, case.name)
        for a, b in case.marks["runs"]:
            assert device_text(sp, dc.GAP_DEPTH, graph, a, b) == (b"", 0)
        sp.close()


# ---------------------------------------------------------------------------------------------------------------------- merged maps
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("k", dc.KS)
def test_merged_widths(k, kind):
    """merge_image of two `widths` maps that share half of their keys: tallies wrap at 2^32 and counts at 2^16 (refimage.merge_add;
    tests/test_dump_cases.py asserts that such sums occur), and the merged map's texts are refdump's over the merged image"""
    a, b = dc.widths(k, kind), dc.widths(k, kind, True)
    kb = dc.kb_of(k)
    sp = loaded(a)
    sp.merge_image(KMR_MAP_WEAK, as_array(b.image))
    merged = ri.canonical(ri.merge_add(a.image, b.image, kb, kind), kb, kind)
    assert sp.image(KMR_MAP_WEAK).tobytes() == merged
    parsed = ri.parse(merged, kb, kind)
    for graph in dc.graphs_of(kind):
        for min_depth in (0, 3, 0xFFFFFFFF):
            check_text(sp, rd.pieces(parsed, k, kind, min_depth, graph), min_depth, graph, "merged")
    sp.close()


# ---------------------------------------------------------------------------------------------------------------------- files
@pytest.mark.parametrize("k,kind", ((13, "weak"), (32, "weak_ext"), (65, "weak_ext"), (127, "weak_ext")))
def test_file_forms(tmp_path, k, kind):
    """kmr_dump_mercount / kmr_dump_mergraph on `widths` with a staging bound of one byte (one entry a piece), 600 bytes (a few
    entries, fewer where the numbers could be wide) and the default (one piece)"""
    case = dc.widths(k, kind)
    sp, parsed = loaded(case), case.parsed
    for graph in dc.graphs_of(kind):
        want = rd.text(parsed, k, kind, 1, graph)
        for piece in (1, 600, 0):
            sp.tune(dump_piece_bytes=piece)
            path = str(tmp_path / ("dump.%d.%d" % (graph, piece)))
            (sp.dumpGraphs if graph else sp.dumpCounts)(path, 1)
            with open(path, "rb") as f:
                assert f.read() == want, (graph, piece)
    sp.close()
