"""The instances of the count pass over super-k-mer lists (sk_count_kernel), each held to the serial oracle at the smallest shapes
where it can go wrong.  What a launch used to say with null pointers is a template argument now -- the pass over work items of long
lists into the merge table, the form of the weak entries -- and the rarely read arguments wait in device memory: a mistake there
shows as a wrong or missing entry on the path that reads it, so every path is taken with every form:

  form    one quality character -> the one-weight form; noisy qualities -> the general form (build_info "uniform_count")
  k       31 (one key word with pad bits), 32 (one word, none), 51 (two words)
  rules   min_depth 1, 2, 3 with and without a separate singleton map
  path    plain lists | long_list_chunks = 2: nearly every list goes through the item instance and the merge table
  table   an honest estimate | estimated_raw_kmers = 1000: a handful of lists that overflow the LDS table and are redone in sub-passes
          | low coverage with 2 % errors: nearly every k-mer distinct, sub-passes on an input that is mostly singletons
"""
import functools

import numpy as np
import pytest

from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, OracleSpectrum, default_config, synth_reads
from test_gpu_parity import add, compare_weak_images, product

pytestmark = pytest.mark.gpu

FORMS = {"flat": 1.0, "noisy": 0.0}      # quality of synth_reads -> build_info("uniform_count")
PATHS = {"lists": {}, "items": {"long_list_chunks": 2}}      # kmr_tune knobs of the path


@functools.lru_cache(maxsize=None)
def _reads(shape, quality, k):
    if shape == "covered":      # 10 x coverage: lists of a few chunks, most k-mers seen several times
        return synth_reads(6000, read_len=150, genome_len=90000, seed=900 + k, quality=quality)
    return synth_reads(30000, read_len=150, genome_len=40_000_000, seed=78 + k, err=0.02, quality=quality)


def _config(k, est, separate_singletons):
    return default_config(k, estimated_raw_kmers=est, num_buckets_weak=4096, num_buckets_singleton=16384, separate_singletons=separate_singletons)


@functools.lru_cache(maxsize=None)
def _oracle(shape, quality, k, est, separate_singletons, min_depth):
    """(statistics, weak image, singleton image) of the serial oracle: computed once, shared by the paths compared with it"""
    o = OracleSpectrum(_config(k, est, separate_singletons))
    o.add_reads(_reads(shape, quality, k))
    o.finalize(min_depth)
    res = (o.stats(), o.image(KMR_MAP_WEAK).copy(), o.image(KMR_MAP_SINGLETON).copy())
    o.close()
    return res


def _build(shape, quality, k, est, separate_singletons, min_depth, **tune):
    p = product(_config(k, est, separate_singletons), 3, **tune)
    add(p, _reads(shape, quality, k))
    p.finalize(min_depth)
    return p


def _check(shape, quality, k, est, separate_singletons, min_depth, path, against=("oracle", "general")):
    """against "oracle": statistics and images are the serial oracle's; "general" (one-weight builds): the general form over the same
    lists (kmr_tune uniform_count = 0) gives the same bytes"""
    tune = PATHS[path]
    kept = bool(separate_singletons) and min_depth == 1
    p = _build(shape, quality, k, est, separate_singletons, min_depth, **tune)
    assert p.build_info("uniform_count") == FORMS[quality]
    stats = p.stats()
    if "oracle" in against:
        stats, weak, sing = _oracle(shape, quality, k, est, separate_singletons, min_depth)
        assert p.stats() == stats, (tune, stats, p.stats())
        assert compare_weak_images(weak, p.image(KMR_MAP_WEAK), p.kb, False) == stats["weak_entries"]
        if kept:
            assert np.array_equal(sing, p.image(KMR_MAP_SINGLETON))
    if "general" in against and quality == "flat":
        g = _build(shape, quality, k, est, separate_singletons, min_depth, uniform_count=0, **tune)
        assert g.build_info("uniform_count") == 0.0
        assert g.stats() == p.stats()
        assert np.array_equal(g.image(KMR_MAP_WEAK), p.image(KMR_MAP_WEAK))
        if kept:
            assert np.array_equal(g.image(KMR_MAP_SINGLETON), p.image(KMR_MAP_SINGLETON))
    return stats


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("separate_singletons", [1, 0])
@pytest.mark.parametrize("k", [31, 32, 51])
@pytest.mark.parametrize("quality", sorted(FORMS))
def test_count_instances_fit_and_overflow(quality, k, separate_singletons, path):
    """lists that fit the table, and (estimated_raw_kmers = 1000) lists that overflow it and run as sub-passes: every rule of
    min_depth, through the list instance and through the item instance with its merge table"""
    n_kmers = 6000 * (150 - k + 1)
    for est in (n_kmers, 1000):
        for min_depth in (1, 2, 3):
            stats = _check("covered", quality, k, est, separate_singletons, min_depth, path)
            assert stats["weak_entries"] > 18000      # (a fifth of the genome's 90 000 k-mers at the least, whatever the qualities discard)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("k", [31, 51])
@pytest.mark.parametrize("quality,against", [("flat", "oracle"), ("flat", "general"), ("noisy", "oracle")])
def test_count_instances_mostly_distinct_kmers(quality, against, k, path):
    """low coverage at 2 % errors with an estimate a third of the truth: lists of nearly all distinct k-mers overflow the table, and
    what is kept is mostly the singleton map (a case per comparison: the input is 3.6 million k-mers, and the first case of a
    (quality, k) pays for the serial oracle over them, ~5 s, which the others share)"""
    stats = _check("sparse", quality, k, 30000 * (150 - k + 1) // 3, 1, 1, path, against=(against,))
    assert stats["singleton_entries"] > 4 * stats["weak_entries"] > 0
