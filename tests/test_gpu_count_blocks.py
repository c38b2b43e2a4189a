"""The two instances of the one-weight, one-word count pass over super-k-mer lists -- compiled for four and for five blocks per
compute unit, kmr_tune "count_blocks" -- give the same bytes, and those of the serial oracle.  What differs between them is what a
mistake would show in: the register allocation of the same source (a value spilled and reloaded at the wrong place), the grid (a
quarter more blocks drawing batches of lists from the one work counter) and the entry buffers' slack (a quarter more wavefronts, each
leaving the tail of an output slab unused).  Shapes, reads and oracles are those of test_gpu_count_instances.py (its caches are shared).

  shape   "covered": 6 000 reads over 90 kb, lists of a few chunks | "sparse": 30 000 reads at 2 % errors, mostly singletons,
          an estimate a third of the truth: lists overflow the LDS table
  k       31 (pad bits in the key word), 32 (none)
  rule    min_depth 2 | min_depth 1 with a separate singleton map (the singleton slabs as well)
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK
from test_gpu_count_instances import _build, _config, _oracle, _reads
from test_gpu_parity import add, compare_weak_images, product

pytestmark = pytest.mark.gpu

# (separate_singletons, min_depth); min_depth 2 with the singletons apart as well: the serial oracle of the sparse shape takes 5 s so,
# and 45 s with its three million singletons in the weak map until the purge
RULES = {"depth2": (1, 2), "singletons": (1, 1)}


def _est(shape, k):
    return 6000 * (150 - k + 1) if shape == "covered" else 30000 * (150 - k + 1) // 3


def _same(a, b, kept):
    assert a.stats() == b.stats(), (a.stats(), b.stats())
    assert np.array_equal(a.image(KMR_MAP_WEAK), b.image(KMR_MAP_WEAK))
    if kept:
        assert np.array_equal(a.image(KMR_MAP_SINGLETON), b.image(KMR_MAP_SINGLETON))


def _is_oracle(p, shape, quality, k, est, sep, min_depth):
    stats, weak, sing = _oracle(shape, quality, k, est, sep, min_depth)
    assert p.stats() == stats, (stats, p.stats())
    assert compare_weak_images(weak, p.image(KMR_MAP_WEAK), p.kb, False) == stats["weak_entries"]
    if sep and min_depth == 1:
        assert np.array_equal(sing, p.image(KMR_MAP_SINGLETON))
    return stats


def _four_and_five(shape, k, est, rule, **tune):
    """the build with each instance: both report what was asked for, agree byte for byte, and are the oracle's"""
    sep, min_depth = RULES[rule]
    built = {}
    for blocks in (4, 5):
        p = _build(shape, "flat", k, est, sep, min_depth, count_blocks=blocks, **tune)
        assert p.build_info("count_blocks") == blocks
        assert p.build_info("uniform_count") == 1.0
        built[blocks] = p
    _same(built[4], built[5], sep and min_depth == 1)
    stats = _is_oracle(built[5], shape, "flat", k, est, sep, min_depth)
    return built, stats


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("shape", ["covered", "sparse"])
def test_four_and_five_blocks_agree(shape, k, rule):
    built, stats = _four_and_five(shape, k, _est(shape, k), rule)
    assert stats["weak_entries"] > 0
    assert built[5].build_info("count_attempts") == 1      # the slack covers the slab tails of the wavefronts launched: no retry on an honest estimate


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("k", [31, 32])
def test_sub_passes_with_five_blocks(k, rule):
    """estimated_raw_kmers = 1000: a handful of lists overflow the LDS table and are redone in sub-passes (the cold copy of the insert
    pass and the stack of (bits, value) that every wavefront reads alike)"""
    _, stats = _four_and_five("covered", k, 1000, rule)
    assert stats["weak_entries"] > 18000


@pytest.mark.parametrize("rule", sorted(RULES))
def test_entry_buffers_grow_with_five_blocks(rule):
    """an entry share of next to nothing: the pass overflows its buffers, runs again with doubled ones, and ends with the plain build's bytes"""
    sep, min_depth = RULES[rule]
    k, est = 31, _est("covered", 31)
    plain = _build("covered", "flat", k, est, sep, min_depth, count_blocks=5)
    small = _build("covered", "flat", k, est, sep, min_depth, count_blocks=5, entry_share=0.00001)
    assert plain.build_info("count_attempts") == 1 and small.build_info("count_attempts") > 1
    assert small.build_info("count_blocks") == 5
    _same(plain, small, sep and min_depth == 1)


def test_general_instance_is_not_touched():
    """noisy qualities take the general form, which has no five-block instance: the knob is ignored and the figure says so"""
    p = _build("covered", "noisy", 31, _est("covered", 31), 1, 1, count_blocks=5)
    assert p.build_info("uniform_count") == 0.0 and p.build_info("count_blocks") == 4
    _is_oracle(p, "covered", "noisy", 31, _est("covered", 31), 1, 1)


def test_count_blocks_takes_0_4_5_only_and_0_is_five():
    p = product(_config(31, 1000, 1), 3)
    for bad in (1, 3, 6, 4.5, -1):
        with pytest.raises(Exception):
            p.tune(count_blocks=bad)
    p.tune(count_blocks=0)
    d = _build("covered", "flat", 31, _est("covered", 31), 1, 2)      # no knob: the default choice
    assert d.build_info("count_blocks") == 5 and d.build_info("uniform_count") == 1.0
    _same(d, _build("covered", "flat", 31, _est("covered", 31), 1, 2, count_blocks=4), False)


def test_long_lists_beside_five_blocks():
    """long_list_chunks = 2: nearly every list is left to the pass over work items (the item instance, four blocks as before); the
    five-block launch over the lists skips them and counts the rest"""
    built, _ = _four_and_five("covered", 31, _est("covered", 31), "depth2", long_list_chunks=2)
    plain = _build("covered", "flat", 31, _est("covered", 31), 1, 2, count_blocks=5)
    _same(plain, built[5], False)


def test_early_count_with_five_blocks():
    """kmr_count_lists_prefix as the two-step exchange drives it (build_partitioned_superkmers with list_steps = 2 and early_min_depth,
    here in a job of one rank): the lower half of the lists is counted early by the five-block instance, kmr_finalize counts the rest
    and takes the early entries over"""
    from kmernator_amd.distributed import build_partitioned_superkmers
    k, est = 31, _est("covered", 31)
    rb = _reads("covered", "flat", k)
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(np.concatenate([rb.bases, np.zeros(64, np.uint8)])).to(dev)
    tq = torch.from_numpy(np.concatenate([rb.quals, np.zeros(64, np.uint8)])).to(dev)
    to = torch.from_numpy(rb.offsets.astype(np.int64)).to(dev)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        built = {}
        for blocks in (4, 5):
            sp = product(_config(k, est, 0), 3, count_blocks=blocks)
            build_partitioned_superkmers(sp, tb, tq, to, first_read_idx=0, list_steps=2, early_min_depth=2)
            assert sp.build_info("count_blocks") == blocks      # the early launch
            sp.finalize(2)
            assert sp.build_info("early_lists") == int(sp.build_info("lists")) // 2 and sp.build_info("early_overflowed") == 0
            assert sp.build_info("count_blocks") == blocks and sp.build_info("uniform_count") == 1.0
            built[blocks] = sp
    finally:
        dist.destroy_process_group()
    _same(built[4], built[5], False)
    plain = _build("covered", "flat", k, est, 0, 2, count_blocks=5)
    _same(plain, built[5], False)
    _is_oracle(built[5], "covered", "flat", k, est, 0, 2)
