"""ContigExtender on the CPU: the restatement (tests/refextend.py) on miniature cases worked out by hand, getNewName and
getMinMaxKmerSize through the library's host entry points against the restatement, the driver's lists and log text, and every family
of tests/extendcases.py against the restatement with the one rule it is written for changed: the family must notice."""
import pytest

import extendcases as ec
import kmernator_amd as ka
import refextend as rx
from helpers import default_config
from kmernator_amd import _lib


def extender_of(c, cls=rx.Extender, k=None):
    return cls(default_config(c["k"] if k is None else k, **c["cfg"]), **c["options"])


def run(c, cls=rx.Extender):
    return extender_of(c, cls).extend(c["contigs"], [ec.pool_of(c, i) for i in range(len(c["contigs"]))], c["active"])


def figures(res):
    """what the device is held to: sequences, totals, stop reasons and the bits of the stop values"""
    return [(s, l, r, tuple((st[0], tuple(rx.bits(v) for v in st[1])) for st in stops)) for s, l, r, stops in res]


# ------------------------------------------------------------------------------------------------------------- miniatures by hand
K = 21
G = ec.R(200, 4242)
CONTIG = G[60:120]


def flat(reads):
    return [(s, b"I" * len(s)) for s in reads]


def test_miniature_grows_right_by_the_reads_bases():
    """five copies of a read that ends three bases past the right edge: three steps, then the edge k-mer is the read's last and has no
    extension; nothing holds the left edge"""
    e = rx.Extender(default_config(K))
    seq, l, r, (sl, sr) = e.extend_one(CONTIG, flat([G[80:123]] * 5))
    assert (seq, l, r) == (G[60:123], 0, 3)
    assert sl == (rx.STOP_NO_EDGE, [0.0] * 6)
    assert sr[0] == rx.STOP_COVERAGE and sr[1][1:] == [0.0] * 5
    assert 4.9 < sr[1][0] < 5.0      # five sightings of weight 0.9999 ** 21


def test_miniature_counts_and_singletons():
    e = rx.Extender(default_config(K), use_weights=False, max_extend=1)
    nxt = G[120:121]
    alt = ec.other(nxt)
    pool = flat([G[90:121]] * 5 + [G[90:120] + alt])
    seq, l, r, (_, sr) = e.extend_one(CONTIG, pool)
    vals = [0.0] * 4
    vals[b"ACGT".index(nxt)] = 5.0
    assert (seq, r) == (G[60:121], 1) and sr == (rx.STOP_LIMIT, [6.0] + vals + [5.0])      # the sixth read's last k-mer is a singleton: not seen
    e = rx.Extender(default_config(K, separate_singletons=0), use_weights=False, max_extend=1)
    seq, l, r, (_, sr) = e.extend_one(CONTIG, pool)
    vals[b"ACGT".index(alt)] = 1.0
    assert (seq, r) == (CONTIG, 0) and sr == (rx.STOP_AMBIGUOUS, [6.0] + vals + [6.0])      # 5 / 6 < 0.85


def test_miniature_short_and_empty():
    e = rx.Extender(default_config(K))
    zero = (rx.STOP_SHORT, [0.0] * 6)
    assert e.extend_one(G[:K - 1], flat([G[:60]] * 6))[1:] == (0, 0, (zero, zero))
    assert e.extend_one(G[:K], flat([G[:60]] * 6))[1:] == (0, 0, (zero, zero))
    assert e.extend_one(CONTIG, [])[1:] == (0, 0, ((rx.STOP_NO_EDGE, [0.0] * 6),) * 2)
    assert rx.Extender(default_config(K), max_extend=0).extend_one(G[:K - 1], [])[3] == ((rx.STOP_LIMIT, [0.0] * 6),) * 2


def test_miniature_fasta_and_pack():
    e = rx.Extender(default_config(K))
    assert e.fasta(b"acgtNn.xACGT") == b"ACGTNnNxACGT"
    assert e.pack(b"acgtNn.xACGT") == b"ACGTAAAAACGT"


# ------------------------------------------------------------------------------------------------------------------ names, k range
WANT_NAMES = {(b"c1", 1, 2): b"c1-l1r2", (b"c1-l3r4", 1, 2): b"c1-l4r6", (b"cell-1", 1, 0): b"cell-1-l1r0", (b"ctgl", 0, 2): b"ctgl-l0r2", (b"x-l2", 1, 1): b"x-l2-l1r1",
              (b"a-l1r2-l3r4", 10, 20): b"a-l1r2-l13r24", (b"c1", 0, 0): b"c1", (b"c1-l3r4", 0, 0): b"c1-l3r4"}


def test_new_name_by_hand():
    for (old, l, r), want in WANT_NAMES.items():
        assert rx.new_name(old, l, r) == want


@pytest.mark.parametrize("old", ec.NAMES)
def test_new_name_of_the_library_equals_the_restatement(old):
    for l, r in ((0, 0), (1, 0), (0, 1), (3, 4), (50, 50), (12345, 678)):
        assert ka.ContigExtender.getNewName(old, l, r) == rx.new_name(old, l, r)


def test_new_name_capacity():
    lib = _lib.load()
    import ctypes as C
    buf = C.create_string_buffer(8)
    assert lib.kmr_extend_new_name(b"c1", 1, 2, buf, 8) == 0 and buf.value == b"c1-l1r2"
    assert lib.kmr_extend_new_name(b"c1", 1, 2, buf, 7) == -6      # KMR_ERR_CAPACITY


def test_min_max_kmer_size():
    assert rx.min_max_kmer_size(31, 150, 15000, 100) == (31, 142, 18)      # by hand: min(142, 149) = 142; 111 / 6 = 18
    assert rx.min_max_kmer_size(21, 100, 7000, 100) == (21, 66, 8)        # mean length 70: 66; 45 / 6 = 7, made even
    for args in ((31, 150, 15000, 100), (21, 100, 7000, 100), (51, 40, 4000, 100), (21, 101, 10100, 100, 3), (21, 0, 0, 5), (21, 36, 3600, 100, 1), (127, 250, 25000, 100)):
        assert ka.ContigExtender.getMinMaxKmerSize(*args) == rx.min_max_kmer_size(*args), args


def test_exports_and_config_defaults():
    import ctypes as C
    lib = _lib.load()
    for name in ("kmr_extend_config_init", "kmr_extend_contigs", "kmr_extend_contigs_dev", "kmr_extend_info", "kmr_extend_copy", "kmr_extend_reads", "kmr_extend_free",
                 "kmr_extend_new_name", "kmr_extend_min_max_kmer_size"):
        assert name in _lib.EXPORTS and getattr(lib, name)
    cfg = _lib.KmrExtendConfig()
    assert lib.kmr_extend_config_init(C.byref(cfg)) == 0
    assert (cfg.struct_size, cfg.max_extend, cfg.minimum_consensus, cfg.minimum_coverage, cfg.maximum_delta_ratio, cfg.use_weights) == (C.sizeof(cfg), 50, 85.0, 4.8, 0.33, 1)
    assert C.sizeof(_lib.KmrExtendStop) == 56 == ka.EXTEND_STOP_DTYPE.itemsize


# ------------------------------------------------------------------------------------------------------------------------- the driver
def driver(c, cls=rx.Extender, minimum_coverage=4.8):
    pools = [ec.pool_of(c, i) for i in range(len(c["contigs"]))]
    return rx.extend_with_contig_extender(lambda k: extender_of(c, cls, k), c["contigs"], c["names"], pools, c["k"], c["k"] + 2, 2, minimum_coverage)


@pytest.mark.parametrize("k", ec.KS)
def test_driver_lists_and_log(k):
    c = ec.driver_case(k)
    changed, final, log = driver(c)
    lines = log.split(b"\n")
    assert lines[0] == b"" and len(lines) == 5
    assert lines[1] == b"Did not extend c1 with 4 reads in the pool"                                  # 4 > 4.8 is false
    g = min(3, ec.READ - (k + 2))      # the bases the reads hold past the edge, or max_extend
    n1, n2 = len(c["contigs"][1]) + g, len(c["contigs"][2]) + g
    assert lines[2] == b"Kmer Extended c1-l3r4 %d bases to %d: c1-l3r%d with 5 reads in the pool K %d" % (g, n1, 4 + g, k)
    assert lines[3] == b"Kmer Extended cell-1 %d bases to %d: cell-1-l0r%d with 6 reads in the pool K %d" % (g, n2, g, k + 2)      # a repeat at k, none at k + 2
    assert lines[4] == b"Did not extend ctgl with 6 reads in the pool"
    assert [n for n, _ in changed] == [b"c1-l3r%d" % (4 + g), b"cell-1-l0r%d" % g] and [n for n, _ in final] == [b"c1", b"ctgl"]
    assert final[0][1] == c["contigs"][0] and changed[0][1][:-g] == c["contigs"][1]
    # pool size against the coverage as a double: 5 > 5.0 is false
    assert [n for n, _ in driver(c, minimum_coverage=5.0)[1]] == [b"c1", b"c1-l3r4", b"ctgl"]
    keep, fin = rx.finish_long_contigs(len(changed[0][1]), changed, final)
    assert [n for n, _ in keep] == [nm for nm, s in changed if len(s) < len(changed[0][1])] and fin[:2] == final and len(keep) + len(fin) == 4
    assert ka.finishLongContigs(len(changed[0][1]), changed, final) == (keep, fin)


# ---------------------------------------------------------------------------------------------------------------- one rule changed each
class NoLimitCheck(rx.Extender):
    """the iteration limit off by one"""
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.max_extend += 1


class CoverageStrict(rx.Extender):
    def goes_on(self, total, edge):
        return total > self.minimum_coverage and rx._div(total, edge) > self.maximum_delta_ratio


class DeltaNotStrict(rx.Extender):
    def goes_on(self, total, edge):
        return total >= self.minimum_coverage and rx._div(total, edge) >= self.maximum_delta_ratio


class ConsensusStrict(rx.Extender):
    def pick(self, values, total):
        for i, v in enumerate(values):
            if rx._div(v, total) > self.minimum_consensus:
                return i
        return None


class OrderReversed(rx.Extender):
    def pick(self, values, total):
        for i in reversed(range(4)):
            if rx._div(values[i], total) >= self.minimum_consensus:
                return i
        return None


class NoExclusion(rx.Extender):
    def excluded(self, key, solid):
        return False


class NoRecord(rx.Extender):
    def record(self, solid, fasta, to_right):
        pass


class FailureEndsBoth(rx.Extender):
    def ends_both(self):
        return True


class SingletonsOtherWay(rx.Extender):
    """the pool's spectrum with the singleton map the other way round"""
    def __init__(self, cfg, **kw):
        super().__init__(default_config(cfg.k, separate_singletons=0 if cfg.separate_singletons else 1), **kw)


class WeightsOtherWay(rx.Extender):
    def __init__(self, cfg, **kw):
        kw["use_weights"] = not kw.get("use_weights", True)
        super().__init__(cfg, **kw)


class MarkupsCount(rx.Extender):
    """an N of a read read as an A, a low quality as a high one"""
    def pool_spectrum(self, pool):
        return super().pool_spectrum([(s.replace(b"N", b"A"), bytes(max(q, 63) for q in qq)) for s, qq in pool])


class PackAsC(rx.Extender):
    """a non-ACGT base packed as C, and given back as it was packed"""
    def pack(self, seq):
        return bytes(b"ACGT"[rx._CODE.get(c, 1)] for c in bytes(seq))

    def fasta(self, seq):
        return self.pack(seq)


class LengthNotStrict(rx.Extender):
    def long_enough(self, fasta):
        return len(fasta) >= self.k


class PoolsShifted(rx.Extender):
    """every contig with its neighbour's pool"""
    def extend(self, contigs, pools, active=None):
        return super().extend(contigs, pools[1:] + pools[:1], active)


class ActiveIgnored(rx.Extender):
    def extend(self, contigs, pools, active=None):
        return super().extend(contigs, pools, None)


class SumReversed(rx.Extender):
    """the pool's sightings added in the opposite order"""
    def pool_spectrum(self, pool):
        return super().pool_spectrum(pool[::-1])


CHANGED = {"limit": NoLimitCheck, "coverage": CoverageStrict, "delta": DeltaNotStrict, "consensus": ConsensusStrict, "order": OrderReversed, "exclude": NoExclusion,
           "record": NoRecord, "other-side": FailureEndsBoth, "singleton": SingletonsOtherWay, "weights": WeightsOtherWay, "read-markup": MarkupsCount, "pack": PackAsC,
           "length": LengthNotStrict, "pool": PoolsShifted, "active": ActiveIgnored, "sum-order": SumReversed}
FAMILY_K = [(f, k) for f in ec.FAMILIES for k in ec.KS]


@pytest.mark.parametrize("family,k", FAMILY_K, ids=["%s-k%d" % (f.__name__, k) for f, k in FAMILY_K])
def test_family_notices_its_rule(family, k):
    """some case of the family gives another result once the family's rule is changed (the several-cut case differs in a tuning knob
    alone); and every case runs under the unchanged rules"""
    cases = family(k)
    rules = {c["rule"] for c in cases}
    assert len(rules) == 1 and rules <= set(CHANGED)
    cls = CHANGED[rules.pop()]
    assert any(figures(run(c)) != figures(run(c, cls)) for c in cases), [c["name"] for c in cases]


def test_recorded_keys_stop_both_sides():
    """the circular family: both sides end on a repeat, the left first, each on a k-mer the other side recorded in this call -- not one
    of the contig's own"""
    for k in ec.KS:
        c = ec.repeat_recorded(k)[0]
        (seq, l, r, stops), = run(c)
        assert (stops[0][0], stops[1][0]) == (rx.STOP_REPEAT, rx.STOP_REPEAT) and 0 < l <= r <= l + 1 < 200
        assert len(c["contigs"][0]) + 16 < len(seq) < len(c["contigs"][0]) + 400

        class OwnOnly(rx.Extender):
            def record(self, solid, fasta, to_right):
                pass
        (_, l2, r2, stops2), = run(c, OwnOnly)
        assert l2 > l and r2 > r
