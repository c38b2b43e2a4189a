"""Directed weak-map images for the mercount / mergraph writer: tests/test_dump_cases.py (CPU: the oracle's dump against
tests/refdump.py, and every coverage condition named here asserted on the expected text) and tests/test_gpu_dump_edges.py
(kmr_dump_text and kin on maps that kmr_load_image left).  No reads and no spectrum build.  Everything is drawn from seeded
generators, so a case id names one image for good.  Keys are made canonical by a plain least-complement in Python.

All families but `buckets` use nb = 1 (mask 0): the map's order is then the key order, whatever the hash, and the image is stored
shuffled so that the load has to sort it.  A case lists its entries in map order; `Case.image` is the stored (shuffled) form,
`Case.sorted_image` what a map that loaded it holds.

An entry's text is two lines of equal length, so it is always even: a tile border can lie at even offsets of an entry only, and
never at an odd offset of a forward line.  A text shorter than 16 bytes cannot exist either: the shortest entry (k = 13, mercount,
a one-digit count) has 2 (13 + 1 + 1 + 1) = 32 bytes.

Families, each for one thing that can go wrong:
  widths   every tally column takes every value of VALS (both sides of every step of the digit count up to 4294967295: put_dec's
           `hi` half is used from 8 digits on), every count of COUNTS; the twelve tallies of an entry differ pairwise and both N
           columns are nonzero except where they take their own turn at 0; the mercount text crosses three tile borders or more
  keys     A^k, keys that end in T^(k & 3) (T for k & 3 = 0), for even k a palindrome (both lines equal), for k >= 64
           T^32 A^(k-32), groups that differ in their last base only
  borders  small k: images that differ in the widths of their first entries, so that over the family the first tile border lies
           at every even offset of an entry of the common length
  gaps     counts 1 and 2 among counts >= 3, for a dump at min depth 3: a tile border exactly at the start of a kept entry that
           follows RUNS entries that are not kept, a border inside a kept entry that follows such a run, a run at the head of the
           map and one at its end
  exact    a text of exactly one tile; of exactly two tiles with only entries that are not kept behind; one tile and one
           shortest entry; one entry
  buckets  imagecases.fills and imagecases.sparse: many buckets, some empty (the oracle's hash deals the keys there)
In borders, gaps and exact the N tallies are 0, as in any map built from reads; the images directed at one text (`graph` False:
mercount, True: mergraph) are laid out by that text's entry lengths."""
import collections
import functools

import numpy as np

import imagecases as ic
import refimage as ri

TILE = 32768
KS = (13, 14, 15, 16, 31, 32, 33, 64, 65, 96, 97, 127)
BORDER_KS = (13, 14, 15, 16)
KINDS = ("weak", "weak_ext")
FAMILIES = ("widths", "keys", "borders", "gaps", "exact", "buckets")
VALS = (0,) + tuple(v for i in range(1, 10) for v in (10 ** i - 1, 10 ** i)) + (4294967295,)
COUNTS = (0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 32767, 32768, 65535)
RUNS = (1, 2, 63, 64, 65, 600)
GAP_DEPTH = 3          # the min depth the gaps and exact families are laid out for
N_COLUMNS = (4, 10)
MAX_DIGITS = {False: 5, True: 102}      # of an entry's numbers: a count; ten tallies of up to ten digits and the two N columns' "0"
COMMON_DIGITS = {False: 1, True: 20}

Case = collections.namedtuple("Case", "name k kind graph nb buckets marks")
Case.image = property(lambda c: ri.pack(c.nb, c.buckets, kb_of(c.k), c.kind))
Case.sorted_image = property(lambda c: ri.canonical(c.image, kb_of(c.k), c.kind))
Case.parsed = property(lambda c: ri.parse(c.sorted_image, kb_of(c.k), c.kind))


def kb_of(k):
    return (k + 3) // 4


def _rng(*what):
    return np.random.default_rng([ord(c) for c in "dump/" + "/".join(str(w) for w in what)])


# ------------------------------------------------------------------------------------------------------------------ keys
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
_CODES = str.maketrans("ACGT", "0123")
_BASES = bytes.maketrans(b"\0\1\2\3", b"ACGT")


def least_complement(seq):
    rc = seq.translate(_COMPLEMENT)[::-1]
    return min(seq, rc)


def pack_key(seq):
    k = len(seq)
    return (int(seq.translate(_CODES), 4) << (2 * (4 * kb_of(k) - k))).to_bytes(kb_of(k), "big")


def sorted_keys(rng, k, n, must=()):
    """n distinct canonical k-mers that include `must`, as packed keys in key order (memcmp order is the order of the bases)"""
    seen = set(must)
    assert all(least_complement(s) == s and len(s) == k for s in seen)
    while len(seen) < n:
        for row in rng.integers(0, 4, size=(n - len(seen), k), dtype=np.uint8):
            seen.add(least_complement(row.tobytes().translate(_BASES).decode()))
    return [pack_key(s) for s in sorted(seen)]


# ------------------------------------------------------------------------------------------------------------------ values
def digits(v):
    return len(str(v))


def entry_len(k, graph, d):
    """bytes of an entry whose numbers have d digits in all: two lines of k bases, a tab, the numbers, and a newline (mercount)
    or twelve blanks, "0" and a newline (mergraph)"""
    return 2 * (k + (15 if graph else 2) + d)


def number_of_width(rng, d):
    return int(rng.integers(0 if d == 1 else 10 ** (d - 1), min(10 ** d - 1, 4294967295) + 1))


def split_digits(rng, d):
    """the digit counts of twelve tallies that have d digits in all, the N columns one (their value is 0)"""
    w = [1] * 12
    free = [j for j in range(12) if j not in N_COLUMNS]
    assert 12 <= d <= MAX_DIGITS[True]
    for _ in range(d - 12):
        j = free[int(rng.integers(0, len(free)))]
        w[j] += 1
        if w[j] == 10:
            free.remove(j)
    return w


def directed_value(rng, kind, graph, keep, d):
    """a weak value whose text for `graph` has d digits; not kept at GAP_DEPTH unless `keep`"""
    if graph:
        count = int(rng.integers(GAP_DEPTH, 65536)) if keep else int(rng.integers(1, GAP_DEPTH))
        tallies = tuple(0 if j in N_COLUMNS else number_of_width(rng, w) for j, w in enumerate(split_digits(rng, d if keep else 12 + int(rng.integers(0, 60)))))
    else:
        count = int(rng.integers(max(GAP_DEPTH, 10 ** (d - 1)), min(10 ** d - 1, 65535) + 1)) if keep else int(rng.integers(1, GAP_DEPTH))
        assert digits(count) == d
        tallies = tuple(0 if j in N_COLUMNS else number_of_width(rng, int(rng.integers(1, 11))) for j in range(12)) if kind == "weak_ext" else ()
    return (count, ic.dyadic_bits(float(count)), int(rng.integers(0, 65536)), tallies, b"\0\0\0\0")


def fill(rng, nbytes, k, graph, d0):
    """digit counts of kept entries whose texts have exactly nbytes in all: as many entries of d0 digits as fit, the rest of the
    bytes dealt out as further digits"""
    assert nbytes % 2 == 0
    half, unit = nbytes // 2, k + (15 if graph else 2)
    n = half // (unit + d0)
    ds = [d0] * n
    rest = half - n * (unit + d0)
    open_ = list(range(n))
    while rest:
        assert open_, "no layout of %d bytes at k = %d" % (nbytes, k)
        i = open_[int(rng.integers(0, len(open_)))]
        ds[i] += 1
        rest -= 1
        if ds[i] == MAX_DIGITS[graph]:
            open_.remove(i)
    assert sum(entry_len(k, graph, d) for d in ds) == nbytes
    return ds


KEEP, DROP = True, False


def directed(name, k, kind, graph, layout, marks=None):
    """the case of a layout [(keep, digits)] in map order"""
    rng = _rng(name, k, kind, graph)
    keys = sorted_keys(rng, k, len(layout))
    entries = [(key, directed_value(rng, kind, graph, keep, d)) for key, (keep, d) in zip(keys, layout)]
    return shuffled(name, k, kind, graph, entries, rng, marks)


def shuffled(name, k, kind, graph, entries, rng, marks=None):
    assert [key for key, _ in entries] == sorted(key for key, _ in entries)
    stored = [entries[i] for i in rng.permutation(len(entries))]
    return Case(name, k, kind, graph, 1, [stored], marks or {})


def graphs_of(kind):
    return (False, True) if kind == "weak_ext" else (False,)


# ------------------------------------------------------------------------------------------------------------------ widths
def widths_entries(k):
    """enough entries for three tile borders in the mercount text (the counts of COUNTS have 3.15 digits on average)"""
    return min(3000, -(-13 * TILE // (4 * 2 * (k + 5))))


def widths_value(rng, kind, i):
    count = COUNTS[i % len(COUNTS)]
    tallies = ()
    if kind == "weak_ext":
        if i < len(VALS):          # column j takes VALS[(i + j) % 20]: every column every value, the N columns their 0 too
            tallies = tuple(VALS[(i + j) % len(VALS)] for j in range(12))
        else:
            while True:
                tallies = tuple(VALS[j] for j in rng.permutation(len(VALS))[:12])
                if all(tallies[j] for j in N_COLUMNS):
                    break
    return (count, ic.dyadic_bits(float(count)), int(rng.integers(0, 65536)), tallies, b"\0\0\0\0")


@functools.lru_cache(maxsize=None)
def _widths_pool(k):
    rng = _rng("widths-keys", k)
    n = widths_entries(k)
    keys = sorted_keys(rng, k, n + n // 4)
    return [keys[i] for i in rng.permutation(len(keys))]


@functools.lru_cache(maxsize=None)
def widths(k, kind, second=False):
    """second: the map to merge into the first -- it shares half of the first's keys and holds a quarter as many of its own; the
    value cycles are shifted, so that sums of tallies pass 2^32 and sums of counts 2^16"""
    rng = _rng("widths", k, kind, second)
    n, pool = widths_entries(k), _widths_pool(k)
    keys = sorted(pool[n // 2:] if second else pool[:n])
    entries = [(key, widths_value(rng, kind, i + (7 if second else 0))) for i, key in enumerate(keys)]
    return shuffled("widths-second" if second else "widths", k, kind, None, entries, rng)


# ------------------------------------------------------------------------------------------------------------------ keys
def special_keys(k):
    """name -> canonical k-mers"""
    rng = _rng("keys", k)

    def random_seq(n):
        return rng.integers(0, 4, size=n, dtype=np.uint8).tobytes().translate(_BASES).decode()

    out = {"zero": ["A" * k]}
    m = (k & 3) or 1
    out["t_tail"] = sorted({least_complement("A" * m + random_seq(k - 2 * m) + "T" * m) for _ in range(6)})      # its reverse complement has the same form
    if k % 2 == 0:
        half = "A" + random_seq(k // 2 - 1)
        out["palindrome"] = [half + half.translate(_COMPLEMENT)[::-1]]
    if k >= 64:
        out["ones"] = ["T" * 32 + "A" * (k - 32)]
    groups = []
    while len(groups) < 3:
        head = "A" + random_seq(k - 2)
        group = [head + b for b in "ACGT" if least_complement(head + b) == head + b]
        if len(group) >= 2:
            groups.append(group)
    out["last_base"] = [s for g in groups for s in g]
    out["last_base_groups"] = groups
    return out


@functools.lru_cache(maxsize=None)
def keys(k, kind):
    rng = _rng("keys-values", k, kind)
    sp = special_keys(k)
    must = {s for name, g in sp.items() if name != "last_base_groups" for s in g}
    ks = sorted_keys(rng, k, len(must) + 20, must)
    entries = []
    for key in ks:
        count = int(rng.integers(1, 65536))
        tallies = tuple(0 if j in N_COLUMNS else number_of_width(rng, int(rng.integers(1, 11))) for j in range(12)) if kind == "weak_ext" else ()
        entries.append((key, (count, ic.dyadic_bits(float(count)), int(rng.integers(0, 65536)), tallies, b"\0\0\0\0")))
    return shuffled("keys", k, kind, None, entries, rng, {name: [pack_key(s) for s in g] for name, g in sp.items() if name != "last_base_groups"})


# ------------------------------------------------------------------------------------------------------------------ borders
SHIFTERS = 6


def common_len(k, graph):
    return entry_len(k, graph, COMMON_DIGITS[graph])


@functools.lru_cache(maxsize=None)
def borders(k, kind, graph):
    """one image per even offset 2 s of the common entry length L: SHIFTERS first entries that hold s digits more than the common
    ones, then common entries to the end of the second tile's first entries.  The first border then lies at offset
    (TILE - SHIFTERS L - 2 s) mod L of a common entry: every even offset once"""
    if k not in BORDER_KS:
        return []
    L, d0 = common_len(k, graph), COMMON_DIGITS[graph]
    out = []
    for s in range(L // 2):
        extra = [s // SHIFTERS + (1 if i < s % SHIFTERS else 0) for i in range(SHIFTERS)]
        assert max(extra) + d0 <= MAX_DIGITS[graph]
        layout = [(KEEP, d0 + e) for e in extra] + [(KEEP, d0)] * (TILE // L + 8)
        out.append(directed("borders-%d" % s, k, kind, graph, layout, {"shift": s}))
    return out


# ------------------------------------------------------------------------------------------------------------------ gaps
@functools.lru_cache(maxsize=None)
def gaps(k, kind, graph):
    """one image per run length r: three entries that are not kept; kept entries of exactly one tile; r not kept; kept entries that
    end half an entry before the second border; r not kept; a kept entry, which the second border cuts; five kept; five not
    kept.  marks["runs"]: the four runs [first, end) of entries that are not kept, in map order"""
    d0 = 20 if graph else 3
    half = entry_len(k, graph, d0) // 4 * 2
    out = []
    for r in RUNS:
        rng = _rng("gaps-layout", k, kind, graph, r)
        first, second = fill(rng, TILE, k, graph, d0), fill(rng, TILE - half, k, graph, d0)
        layout, runs = [], []
        for part in ([(DROP, 1)] * 3, [(KEEP, d) for d in first], [(DROP, 1)] * r, [(KEEP, d) for d in second], [(DROP, 1)] * r,
                     [(KEEP, d0)] * 6, [(DROP, 1)] * 5):
            if part[0][0] == DROP:
                runs.append((len(layout), len(layout) + len(part)))
            layout += part
        out.append(directed("gaps-%d" % r, k, kind, graph, layout, {"runs": runs, "run": r}))
    return out


# ------------------------------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def exact(k, kind, graph):
    d0 = 20 if graph else 2
    shortest = 12 if graph else 1
    rng = _rng("exact-layout", k, kind, graph)
    one, two = fill(rng, TILE, k, graph, d0), fill(rng, TILE, k, graph, d0) + fill(rng, TILE, k, graph, d0)      # (a border between two entries, too)
    return [directed("exact-one_tile", k, kind, graph, [(KEEP, d) for d in one]),
            directed("exact-two_tiles", k, kind, graph, [(KEEP, d) for d in two] + [(DROP, 1)] * 7, {"runs": [(len(two), len(two) + 7)]}),
            directed("exact-tile_and_shortest", k, kind, graph, [(KEEP, d) for d in one] + [(KEEP, shortest)]),
            directed("exact-one_entry", k, kind, graph, [(KEEP, d0)])]


# ------------------------------------------------------------------------------------------------------------------ buckets
@functools.lru_cache(maxsize=None)
def buckets(k, kind):
    return [Case("buckets-fills", k, kind, None, *ic.fills(k, kind), {}), Case("buckets-sparse", k, kind, None, *ic.sparse(k, kind), {})]


def cases(family, k, kind):
    """every case of a family at this k and value kind"""
    if family == "widths":
        return [widths(k, kind)]
    if family == "keys":
        return [keys(k, kind)]
    if family == "buckets":
        return buckets(k, kind)
    return [c for graph in graphs_of(kind) for c in {"borders": borders, "gaps": gaps, "exact": exact}[family](k, kind, graph)]


def texts_of(case):
    """the texts a case is compared in: the one it was laid out for, or both"""
    return graphs_of(case.kind) if case.graph is None else (case.graph,)
