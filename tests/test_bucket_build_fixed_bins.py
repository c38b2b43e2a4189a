"""The default build's bucket build with bins of one capacity (kmr_buckets.hpp: no histogram passes, nothing between the count pass
and the end of the group kernel waits for the host): the finalized weak map must be the serial oracle's and, byte for byte, what
the same build makes with measured bins (kmr_tune bb_fixed_bins = 0) -- in one-level and two-level geometries, over one-word and
two-word keys, with flat and noisy qualities, with holes in the count pass's slabs (min-depth 2 and 3), on a map so small that a
first-level bin is a single tile, when a bin or a group overflows its capacity (the build is made again with measured bins),
twice on one handle (also behind a build that overflowed), behind an early count of half the lists, and with the singleton map kept."""
import functools

import numpy as np
import pytest

from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, OracleSpectrum, default_config, synth_reads
from test_gpu_parity import add, compare_weak_images, product

pytestmark = pytest.mark.gpu

READ_LEN = 100
FIXED, MEASURED = 2.0, 1.0      # kmr_build_info "bb_path"


@functools.lru_cache(maxsize=None)
def reads(n, genome, seed, quality):
    return synth_reads(n, read_len=READ_LEN, genome_len=genome, seed=seed, err=0.01, quality=quality)


def config(k, n, nbw):
    return default_config(k, estimated_raw_kmers=n * (READ_LEN - k + 1), num_buckets_weak=nbw, num_buckets_singleton=nbw)


@functools.lru_cache(maxsize=None)
def oracle(k, n, genome, seed, quality, nbw, min_depth):
    """the serial oracle's weak image and statistics of one case: made once, shared, read only"""
    o = OracleSpectrum(config(k, n, nbw))
    o.add_reads(reads(n, genome, seed, quality))
    o.finalize(min_depth)
    img = o.image(KMR_MAP_WEAK)
    img.setflags(write=False)
    return img, o.stats()


def build(k, n, genome, seed, quality, nbw, min_depth, **tune):
    tune.setdefault("binned_buckets_min", 0)
    p = product(config(k, n, nbw), 3, **tune)
    add(p, reads(n, genome, seed, quality))
    p.finalize(min_depth)
    return p


def check(case, path=FIXED, fallback=0.0, **tune):
    """one build of `case` under `tune`: the oracle's map, the bytes of the build with measured bins, the path it says it took"""
    img_o, stats_o = oracle(*case)
    p = build(*case, **tune)
    assert p.stats() == stats_o
    assert p.build_info("bb_path") == path and p.build_info("bb_fallback") == fallback
    img_p = p.image(KMR_MAP_WEAK)
    assert compare_weak_images(img_o, img_p, p.kb, False) == stats_o["weak_entries"]
    q = build(*case, bb_fixed_bins=0)
    assert q.build_info("bb_path") == MEASURED and q.build_info("bb_fallback") == 0.0
    assert np.array_equal(img_p, q.image(KMR_MAP_WEAK))
    p.sync()      # the handle's error state is clean
    return p, stats_o


# (k, reads, genome length, seed, quality, weak buckets, min depth).  ~2.9 * 10^5 weak entries at k = 31: 2^16 buckets leave 9 bits to
# resolve (one level, 512 groups of ~560), 2^19 buckets leave 11 (two levels of 6 and 5 bits: 64 bins of ~4500, 2048 groups of ~140)
ONE_LEVEL = [(31, 40000, 280000, 11, "flat", 1 << 16, 2), (31, 40000, 280000, 12, "noisy", 1 << 16, 3)]
TWO_LEVELS = [(31, 40000, 280000, 11, "flat", 1 << 19, 2), (31, 40000, 280000, 12, "noisy", 1 << 19, 2), (31, 40000, 280000, 11, "flat", 1 << 19, 3),
              (51, 40000, 280000, 13, "flat", 1 << 19, 2), (51, 40000, 280000, 14, "noisy", 1 << 19, 2)]


@pytest.mark.parametrize("case", ONE_LEVEL + TWO_LEVELS, ids=lambda c: "k%d-%s-2^%d-d%d" % (c[0], c[4], c[5].bit_length() - 1, c[6]))
def test_fixed_bins_equal_oracle_and_measured_bins(case):
    _, stats_o = check(case)
    assert stats_o["weak_entries"] > 200000


def test_tiny_map_one_tile_per_bin():
    """~1300 weak entries over 2^19 buckets, just above a binned_buckets_min of 1000: 64 first-level bins of ~20 entries, each one
    tile of capacity, 2048 groups of less than one entry on average"""
    case = (31, 400, 1200, 15, "flat", 1 << 19, 2)
    _, stats_o = check(case, binned_buckets_min=1000)
    assert 1000 <= stats_o["weak_entries"] < 1500


@pytest.mark.parametrize("case,knob", [(TWO_LEVELS[0], "bb_slack_bins"), (TWO_LEVELS[0], "bb_slack_groups"), (ONE_LEVEL[0], "bb_slack_groups"), (TWO_LEVELS[3], "bb_slack_groups")],
                         ids=["level1", "level2", "one-level", "k51-level2"])
def test_overflow_falls_back_to_measured_bins(case, knob):
    """no room above the mean (slack 0): the bins of that level hold fewer entries together than there are, so one of them overflows.
    Nothing is stored past a bin, the levels behind it do nothing, and the build is made again with measured bins: same map, and
    kmr_build_info says so"""
    check(case, path=MEASURED, fallback=1.0, **{knob: 0})


def test_two_builds_on_one_handle():
    """kmr_reset between two builds: the partition's buffers are reused, fill counts and the overflow word start from zero"""
    first, second = TWO_LEVELS[0], (31, 40000, 160000, 16, "flat", 1 << 19, 2)
    p = build(*first)
    img_o, stats_o = oracle(*first)
    assert p.build_info("bb_path") == FIXED and p.build_info("bb_fallback") == 0.0
    assert compare_weak_images(img_o, p.image(KMR_MAP_WEAK), p.kb, False) == stats_o["weak_entries"]
    p.reset()
    add(p, reads(*second[1:5]))
    p.finalize(second[6])
    img_o, stats_o = oracle(*second)
    assert p.stats()["weak_entries"] == stats_o["weak_entries"]
    assert p.build_info("bb_path") == FIXED and p.build_info("bb_fallback") == 0.0
    assert compare_weak_images(img_o, p.image(KMR_MAP_WEAK), p.kb, False) == stats_o["weak_entries"]


@pytest.mark.parametrize("knob", ["bb_slack_bins", "bb_slack_groups"])
def test_build_after_an_overflowed_one_on_the_same_handle(knob):
    """the first build overflows a level and is made again with measured bins; after kmr_reset and with the slack back at its
    default, the same handle builds other reads with bins of one capacity: the overflow word, the fill counts and "bb_fallback"
    are those of the second build alone"""
    first, second = TWO_LEVELS[0], (31, 40000, 160000, 16, "flat", 1 << 19, 2)
    p = build(*first, **{knob: 0})
    assert p.build_info("bb_path") == MEASURED and p.build_info("bb_fallback") == 1.0
    assert p.stats() == oracle(*first)[1]      # (its map: test_overflow_falls_back_to_measured_bins)
    p.sync()
    p.reset()
    p.tune(**{knob: 1})
    add(p, reads(*second[1:5]))
    p.finalize(second[6])
    img_o, stats_o = oracle(*second)
    assert p.stats() == stats_o
    assert p.build_info("bb_path") == FIXED and p.build_info("bb_fallback") == 0.0
    assert compare_weak_images(img_o, p.image(KMR_MAP_WEAK), p.kb, False) == stats_o["weak_entries"]
    p.sync()


@pytest.mark.parametrize("knob", [None, "bb_slack_bins"], ids=["fits", "overflow"])
def test_early_count_then_fixed_bins(knob):
    """kmr_count_lists_prefix counts the lower half of the lists ahead of kmr_finalize, which takes those entries over behind its own
    before the partition -- and, when a bin overflows, a second time behind the entries of the repeated count pass"""
    case = TWO_LEVELS[0]
    img_o, stats_o = oracle(*case)
    k, n, nbw = case[0], case[1], case[5]
    tune = {"binned_buckets_min": 0}
    if knob:
        tune[knob] = 0
    p = product(config(k, n, nbw), 3, **tune)
    add(p, reads(*case[1:5]))
    nl = int(p.build_info("lists"))
    assert nl > 64
    p.count_lists_prefix(case[6], nl // 2)
    p.finalize(case[6])
    assert p.build_info("early_lists") == nl // 2 and 0 < p.build_info("early_entries") < stats_o["weak_entries"]
    assert p.stats() == stats_o
    assert p.build_info("bb_path") == (MEASURED if knob else FIXED) and p.build_info("bb_fallback") == (1.0 if knob else 0.0)
    assert compare_weak_images(img_o, p.image(KMR_MAP_WEAK), p.kb, False) == stats_o["weak_entries"]
    p.sync()


def test_singleton_map_kept_behind_fixed_bins():
    """min-depth 1 keeps the singleton map: its bucket starts are scanned on the stream behind the partition, and both maps are,
    byte for byte, those of the build with measured bins"""
    case = (31, 40000, 280000, 11, "flat", 1 << 19, 1)
    p, q = build(*case), build(*case, bb_fixed_bins=0)
    assert p.build_info("bb_path") == FIXED and q.build_info("bb_path") == MEASURED and p.build_info("bb_fallback") == 0.0
    assert p.stats() == q.stats() and p.stats()["singleton_entries"] > 0
    assert np.array_equal(p.image(KMR_MAP_WEAK), q.image(KMR_MAP_WEAK)) and np.array_equal(p.image(KMR_MAP_SINGLETON), q.image(KMR_MAP_SINGLETON))
    img_o, stats_o = oracle(*case)
    assert p.stats() == stats_o
    assert compare_weak_images(img_o, p.image(KMR_MAP_WEAK), p.kb, False) == stats_o["weak_entries"]
    p.sync()
