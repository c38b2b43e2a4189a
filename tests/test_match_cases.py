"""KmerMatch on the CPU: the restatement's instance map (tests/refmatch.py) against the oracle's spectrum, every family of
tests/matchcases.py against the restatement with its one rule changed, the independence of the batch cuts, and the new symbols of the
library."""
import ctypes as C

import numpy as np
import pytest

import kmernator_amd as ka
import matchcases as mc
from helpers import default_config
from kmernator_amd import _lib
from refcompare import oracle_set_map
from refmatch import Matcher, same_result
from refnormalize import M32


def matcher_of(c, cls=Matcher, **kw):
    s = dict(min_depth=c["min_depth"], max_positions_from_edge=c["edge"], max_read_matches=c["max_read_matches"], include_mate=c["include_mate"], seed=c["seed"])
    s.update(kw)
    return cls(default_config(c["k"]), **s)


def run(c, cls=Matcher, cuts=(), **kw):
    return matcher_of(c, cls, **kw).match(c["contigs"], mc.batches_of(c, cuts))


@pytest.mark.parametrize("min_depth", [1, 2, 3])
@pytest.mark.parametrize("k", [21, 22, 65])
def test_instance_map_equals_oracle_spectrum(k, min_depth):
    """the keys, and the counts as instance counts, of what purgeMinDepth leaves"""
    c = mc.mixed(k, dup=True)
    live = [r for r, d in zip(c["reads"], c["discarded"]) if not d]
    m = Matcher(default_config(k), min_depth=min_depth)
    spec = m.spectrum(mc.batches_of(c))
    assert {key: len(v) for key, v in spec.items()} == oracle_set_map(default_config(k), live, min_depth=min_depth)
    assert all(len(set(v)) == len(v) for v in spec.values())


# ---------------------------------------------------------------------------------------------------------------- one rule changed each
class SymmetricEdges(Matcher):
    def considered(self, n):
        M = self.max_kmers_from_edge()
        return [j for j in range(n) if M < 0 or j < M or j >= n - M]


class UnsignedPositions(Matcher):
    """M held in an unsigned before the subtraction is undone: below zero it is nothing instead of everything"""
    def considered(self, n):
        M = max(self.max_kmers_from_edge(), 0)
        upper = n - M if n > M else 0
        return [j for j in range(n) if j <= M or j >= upper]


class ZeroedN(Matcher):
    def contig_keys(self, seq):
        keys = Matcher.contig_keys(self, seq)
        return [None if any(ch not in b"ACGTacgt" for ch in bytes(seq)[j:j + self.k]) else key for j, key in enumerate(keys)]


class NoWeightTest(Matcher):
    def passes(self, w):
        return True


class NoDepthPurge(Matcher):
    def holds(self, instances):
        return True


class MatesBeforeSampling(Matcher):
    def sample_then_mates(self, contig, hits, mate):
        both = dict(hits)
        if self.include_mate:
            both.update({mate[r]: 1 for r in hits if r in mate})
        size = self.size(both)
        reads = sorted(both)
        kept = [r for r in reads if self.keeps(r, contig, size)] if self.is_sampled(size) else reads
        return size, kept, set(kept)


class DiscardedKept(Matcher):
    def drops(self, read, discarded):
        return False


class FractionInDouble(Matcher):
    def keeps(self, read, contig, size):
        return float(self.uniform(read, contig)) <= float(self.max_hits()) / float(size)


class HitMultiset(Matcher):
    def add_hits(self, hits, instances):
        for read, _ in instances:
            hits[read] = hits.get(read, 0) + 1

    def size(self, hits):
        return sum(hits.values())


DEVIATIONS = [
    ("symmetric_edges", SymmetricEdges, lambda: mc.shapes(21)),
    ("unsigned_positions", UnsignedPositions, lambda: mc.edge_settings(21)[0]),
    ("unsigned_positions_k_minus_2", UnsignedPositions, lambda: mc.edge_settings(33)[1]),
    ("zeroed_n", ZeroedN, lambda: mc.mixed(21)),
    ("no_weight_test", NoWeightTest, lambda: mc.mixed(21)),
    ("no_depth_purge", NoDepthPurge, lambda: mc.mixed(22, min_depth=2)),
    ("mates_before_sampling", MatesBeforeSampling, lambda: mc.many(21, 300, max_read_matches=100)),
    ("discarded_kept", DiscardedKept, lambda: mc.mixed(33)),
    ("fraction_in_double", FractionInDouble, lambda: mc.f32_edge()),
    ("hit_multiset", HitMultiset, lambda: mc.many(21, 70, max_read_matches=35)),
]


@pytest.mark.parametrize("name,deviant,make", DEVIATIONS, ids=[d[0] for d in DEVIATIONS])
def test_every_family_notices_its_deviation(name, deviant, make):
    c = make()
    assert not same_result(run(c), run(c, deviant))


# ------------------------------------------------------------------------------------------------------------- what the families mean
def sets_of(res):
    return [[int(x) for x in res["reads"][int(res["offsets"][i]):int(res["offsets"][i + 1])]] for i in range(len(res["offsets"]) - 1)]


def test_mixed_family_means_what_it_says():
    c = mc.mixed(22)
    s = sets_of(run(c))
    # (12 fails the weight test and 9 holds no k-mer, but both are mates of hits; 3 and 10 are discarded)
    assert s[0] == [0, 1, 2] and s[1] == [0, 1, 12, 13, 14, 15] and s[2] == [6, 7] and s[3] == [8, 9] and s[4] == [] and s[5] == [16, 17]
    assert sets_of(run(c, include_mate=False)) == [[0, 2], [0, 13, 14], [6], [8], [], [16]]
    # under min_depth 2 only the keys seen twice are left: X (twice in read 6) and read 13's and 14's
    assert sets_of(run(mc.mixed(22, min_depth=2), include_mate=False)) == [[], [13, 14], [6], [], [], []]


def test_shapes_and_edge_settings_mean_what_they_say():
    k, M = 21, 4
    c = mc.shapes(k, M)
    res = run(c)
    ns = (0, 1, M, M + 1, 2 * M, 2 * M + 1, 2 * M + 2)
    assert [int(x) for x in res["size_before_sampling"]] == [0, 1, M, M + 1, 2 * M, 2 * M + 1, 2 * M + 1]
    first = sum(ns[:-1])                                            # the reads of the longest contig, one per k-mer
    last = sets_of(res)[-1]
    assert first + M in last and first + M + 1 not in last and first + ns[-1] - M - 1 not in last and first + ns[-1] - M in last
    sizes = [int(run(e)["size_before_sampling"][0]) for e in mc.edge_settings(k)]
    assert sizes == [12, 12, 1, 12]


def test_sampling_threshold_seeds_and_mates():
    at, above = run(mc.many(21, 70, max_read_matches=35)), run(mc.many(21, 71, max_read_matches=35))
    assert at["n_sampled_contigs"] == 0 and int(at["size_after_sampling"][0]) == 70 and len(at["reads"]) == 140
    assert above["n_sampled_contigs"] == 1 and int(above["size_before_sampling"][0]) == 71 and 40 < int(above["size_after_sampling"][0]) <= 71
    a, b = run(mc.many(21, 300, max_read_matches=100)), run(mc.many(21, 300, max_read_matches=100, seed=12345))
    assert not same_result(a, b) and 150 < int(a["size_after_sampling"][0]) < 250 and 150 < int(b["size_after_sampling"][0]) < 250
    assert len(a["reads"]) == 2 * int(a["size_after_sampling"][0])      # the mates of the reads that stayed, and no others
    none = run(mc.many(21, 300, max_read_matches=0))
    assert none["n_sampled_contigs"] == 0 and int(none["size_after_sampling"][0]) == 300
    # the same reads under other global indices draw other numbers
    shifted = run(mc.many(21, 300, max_read_matches=100, first=(1 << 32) + 12345))
    assert not np.array_equal(shifted["reads"] - np.uint64((1 << 32) + 12345), a["reads"])


def test_f32_edge_read_sits_on_the_bound():
    c = mc.f32_edge()
    m = matcher_of(c)
    assert m.uniform(mc.F32_EDGE_READ, 0) == m.fraction(7) and float(m.fraction(7)) > 6.0 / 7.0
    assert mc.F32_EDGE_READ in sets_of(run(c))[0] and mc.F32_EDGE_READ > M32


@pytest.mark.parametrize("make", [lambda: mc.mixed(21), lambda: mc.mixed(65, dup=True, min_depth=2), lambda: mc.shapes(22), lambda: mc.many(21, 71, max_read_matches=35),
                                  lambda: mc.f32_edge()], ids=["mixed", "mixed_dup", "shapes", "many", "f32_edge"])
def test_result_does_not_depend_on_the_batch_cuts(make):
    c = make()
    whole = run(c)
    layouts = mc.cut_layouts(c)
    assert len(layouts) >= 2
    for cuts in layouts:
        assert same_result(whole, run(c, cuts=cuts)), cuts


# ----------------------------------------------------------------------------------------------------------------- the library's side
def test_symbols_are_exported_and_the_config_has_the_defaults():
    lib = ka.load()
    for name in ("kmr_match_config_init", "kmr_match_create", "kmr_match_edge_info", "kmr_match_add_read_batch", "kmr_match_finish", "kmr_match_info", "kmr_match_copy",
                 "kmr_match_device_ptrs", "kmr_match_free"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    cfg = _lib.KmrMatchConfig()
    assert C.sizeof(cfg) == 24
    assert lib.kmr_match_config_init(C.byref(cfg)) == 0
    assert (cfg.struct_size, cfg.max_positions_from_edge, cfg.max_read_matches, cfg.include_mate, cfg.seed) == (24, 500, 450, 1, 0)
    assert lib.kmr_match_config_init(None) == -1
    # no handle can exist without a device, and no entry point invents one
    m = C.c_void_p()
    assert lib.kmr_match_create(None, None, C.byref(cfg), C.byref(m)) == -1 and not m.value
    assert lib.kmr_match_add_read_batch(None, None, 0, None, None) == -1
    assert lib.kmr_match_finish(None) == -1 and lib.kmr_match_info(None, None, None, None) == -1
    assert lib.kmr_match_copy(None, None, None, None, None) == -1 and lib.kmr_match_edge_info(None, None, None, None, None) == -1
    lib.kmr_match_free(None)
    assert hasattr(ka, "KmerMatch") and hasattr(ka, "MatchResults")
