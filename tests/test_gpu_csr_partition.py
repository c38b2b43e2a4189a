"""The chunk CSR of a build on super-k-mer lists (build_csr: where every list's chunks lie) made by the radix partition of the
(list, chunk) pairs -- csr_bin_hist / _scan / _scatter / _place, kmr_tune "csr_partition" = 1, the default -- and by the path it
replaces, one device atomic per chunk (csr_partition = 0); and the feed's pre-pass, which learns the longest read of a call from
the pass over its qualities and cuts work units only for a batch that holds a read longer than a tile.

Every build is held to the serial oracle's statistics and images, never to the other path: a CSR that loses, doubles or misfiles
a chunk loses, doubles or misfiles its k-mers.  kmr_build_info "csr_path" says which path the last build_csr took, "csr_chunks"
how many chunks it looked at (a tile of the partition is 8192 chunks), "unit_batches" how many batches were cut into units.

Shapes: 2 000 reads get 192 lists, a bin each, so the ragged last bin comes from kmr_tune list_aim (2 560 lists in bins of three).
40 000 reads look at 8 x 10^4 chunks, ten tiles.  A tile of the extraction holds 9 824 bases, so a 1 000-base read is still one work
unit: the batch is kept and a 12 000-base read beside it is the one that has to be cut.  The strided lists of several ranks on one
GPU need a process per rank (tests/test_gpu_two_ranks.py, which runs on the default path); here the early count of the lower lists
(kmr_count_lists_prefix) is taken on one handle.
"""
import functools

import numpy as np
import pytest

from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, OracleSpectrum, ReadBatch, default_config, synth_reads
from test_gpu_parity import _pack_twobit, add, compare_weak_images, product

pytestmark = pytest.mark.gpu

TILE = 8192           # chunks per tile of the partition (CSRP_TILE)
BINS = 1024           # most bins (CSRP_BINS)
PATHS = [1, 0]        # kmr_tune csr_partition -> kmr_build_info csr_path


def _with_poly_a(rb, n):
    """rb and n reads of 150 A behind it: one k-mer, one list, thousands of sightings"""
    bases = np.concatenate([rb.bases, np.full(150 * n, ord("A"), np.uint8)])
    quals = np.concatenate([rb.quals, np.full(150 * n, ord("I"), np.uint8)])
    offsets = np.concatenate([rb.offsets, rb.offsets[-1] + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(150)])
    return ReadBatch.from_arrays(bases, quals, offsets)


def _with_long_read(rb, length, seed):
    """rb with one read of `length` random bases in its middle (qualities: 'I')"""
    rng = np.random.default_rng(seed)
    long_read = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)]
    seqs = [rb.seq(i) for i in range(rb.n)]
    quals = [rb.qual(i) for i in range(rb.n)]
    seqs.insert(rb.n // 2, long_read.tobytes())
    quals.insert(rb.n // 2, b"I" * length)
    return ReadBatch(seqs, quals)


@functools.lru_cache(maxsize=None)
def _reads(name):
    if name == "small":
        return synth_reads(2000, read_len=150, seed=5, quality="flat")
    if name in ("flat", "noisy"):
        return synth_reads(40000, read_len=150, seed=6, quality=name)
    if name == "poly_a":
        return _with_poly_a(_reads("flat"), 5000)
    if name == "k51":
        return synth_reads(20000, read_len=150, seed=7, quality="noisy")
    if name == "long1000":      # the issue's batch: one 1 000-base read among 150-base reads
        return _with_long_read(synth_reads(3000, read_len=150, seed=8, quality="flat"), 1000, 80)
    if name == "long12000":     # ... and one that is longer than a tile of the extraction (9 824 bases): cut into two work units
        return _with_long_read(synth_reads(3000, read_len=150, seed=8, quality="flat"), 12000, 81)
    raise KeyError(name)


def _config(name, k):
    rb = _reads(name)
    return default_config(k, estimated_raw_kmers=int(rb.offsets[-1]) - rb.n * (k - 1), num_buckets_weak=4096, num_buckets_singleton=16384)


@functools.lru_cache(maxsize=None)
def _oracle(name, k, min_depth):
    """(statistics, weak image, singleton image) of the serial oracle over the batch: computed once, shared by both paths"""
    o = OracleSpectrum(_config(name, k))
    o.add_reads(_reads(name))
    o.finalize(min_depth)
    res = (o.stats(), o.image(KMR_MAP_WEAK).copy(), o.image(KMR_MAP_SINGLETON).copy())
    o.close()
    return res


def _assert_oracle(p, name, k, min_depth, path, saturated=False):
    stats, weak, sing = _oracle(name, k, min_depth)
    assert p.build_info("csr_path") == path
    assert p.stats() == stats, (name, path, stats, p.stats())
    assert compare_weak_images(weak, p.image(KMR_MAP_WEAK), p.kb, False, saturated_dir_free=saturated) == stats["weak_entries"]
    if min_depth == 1:
        assert np.array_equal(sing, p.image(KMR_MAP_SINGLETON))


def _build(name, k, min_depth, path, **tune):
    p = product(_config(name, k), 3, csr_partition=path, **tune)
    add(p, _reads(name))
    p.finalize(min_depth)
    return p


@pytest.mark.parametrize("path", PATHS)
def test_fewer_chunks_than_a_tile_and_a_ragged_last_bin(path):
    """2 000 reads: one partial tile.  Left alone the batch gets 192 lists, a bin each; list_aim = 94 k-mers per list gives it 2 560 (list
    counts are multiples of 64): bins of three lists, and a last bin that holds one"""
    p = _build("small", 31, 1, path, list_aim=94)
    nl = int(p.build_info("lists"))
    width = (nl + BINS - 1) // BINS
    print("lists %d width %d chunks %d" % (nl, width, p.build_info("csr_chunks")))
    assert nl == 2560 and nl % width == 1 and nl <= p.build_info("csr_chunks")
    _assert_oracle(p, "small", 31, 1, path)
    p = _build("small", 31, 1, path)      # ... and as it comes: fewer lists than bins
    assert int(p.build_info("lists")) < BINS and 0 < p.build_info("csr_chunks") < TILE
    _assert_oracle(p, "small", 31, 1, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("quality", ["flat", "noisy"])
def test_several_tiles_every_bin_populated(quality, path):
    """40 000 reads: more than two tiles of chunks, every bin holds chunks of many lists"""
    p = _build(quality, 31, 2, path)
    print("lists %d chunks %d" % (p.build_info("lists"), p.build_info("csr_chunks")))
    assert p.build_info("csr_chunks") > 2 * TILE
    _assert_oracle(p, quality, 31, 2, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("long_list_chunks", [0, 16])
def test_one_list_owns_most_of_a_bin(long_list_chunks, path):
    """the same reads and 5 000 poly-A reads: one list with hundreds of chunks in a bin of short ones; long_list_chunks = 16 sends it (and
    more) through the count pass's work items, which read the CSR by chunk ranges"""
    tune = {"long_list_chunks": long_list_chunks} if long_list_chunks else {}
    p = _build("poly_a", 31, 2, path, **tune)
    assert p.build_info("csr_chunks") > 2 * TILE
    _assert_oracle(p, "poly_a", 31, 2, path, saturated=True)


@pytest.mark.parametrize("path", PATHS)
def test_two_word_keys(path):
    p = _build("k51", 51, 2, path)
    assert p.build_info("csr_chunks") > TILE
    _assert_oracle(p, "k51", 51, 2, path)


@pytest.mark.parametrize("path", PATHS)
def test_empty_call_reuse_after_reset_and_three_calls(path):
    """an empty call and a finalize of nothing; then, on the same handle after reset (the finalize arena is reused), the build fed in
    three calls"""
    rb = _reads("k51")
    p = product(_config("k51", 31), 3, csr_partition=path)
    add(p, rb.slice(0, 0))
    p.finalize(2)
    assert p.build_info("csr_path") == path and p.build_info("csr_chunks") == 0
    assert p.stats()["weak_entries"] == 0 and p.stats()["raw_kmers"] == 0
    for _ in range(2):      # (the second round runs in the arena the first one sized)
        p.reset()
        for lo, hi in ((0, 7000), (7000, 7001), (7001, rb.n)):
            add(p, rb.slice(lo, hi), first=lo)
        p.finalize(2)
        _assert_oracle(p, "k51", 31, 2, path)


@pytest.mark.parametrize("path", PATHS)
def test_lists_counted_early_then_the_rest(path):
    """kmr_count_lists_prefix on one handle: the CSR of the early count over the lower half of the lists, and the CSR of the finalize
    that takes its entries over.  (The strided lists of two ranks on one GPU are test_gpu_two_ranks', which take the default path.)"""
    p = product(_config("k51", 31), 3, csr_partition=path)
    add(p, _reads("k51"))
    nl = int(p.build_info("lists"))
    p.count_lists_prefix(2, nl // 2)
    assert p.build_info("csr_path") == path and p.build_info("csr_chunks") > TILE
    p.finalize(2)
    assert p.build_info("early_lists") == nl // 2 or p.build_info("early_overflowed") == 1.0
    _assert_oracle(p, "k51", 31, 2, path)


@pytest.mark.parametrize("name,units", [("long1000", 0), ("long12000", 1)])
def test_long_read_through_the_fused_pre_pass(name, units):
    """one long read among 150-base reads of one quality character: the pass over the qualities brings the longest read along.  1 000
    bases fit a tile (no units); 12 000 do not, and the batch must be cut into units although nothing counted units beforehand"""
    p = _build(name, 31, 1, 1)
    assert p.build_info("unit_batches") == units and p.build_info("uniform_count") == 1.0
    _assert_oracle(p, name, 31, 1, 1)


@pytest.mark.parametrize("name,units", [("long1000", 0), ("long12000", 1)])
def test_long_read_with_the_quality_hinted(name, units):
    """the same batches handed over packed with uniform_quality: no quality pass, the longest read is learned by prepare_units itself"""
    rb = _reads(name)
    tw, to, mk = _pack_twobit(rb)
    p = product(_config(name, 31), 3)
    p.buildKmerSpectrumTwoBit(tw, to, rb.offsets, uniform_quality=ord("I"), markups=mk)
    p.finalize(1)
    assert p.build_info("unit_batches") == units
    _assert_oracle(p, name, 31, 1, 1)
