"""The six-block instance of the one-weight, one-word count pass over super-k-mer lists (kmr_tune "count_six"): table slots of 20
bytes, whose first-sighting word is 32 bits wide -- (stream ordinal - lowest ordinal of the build) << 1 | forward -- instead of the 64
bits of every other instance.  It has to give the bytes of the five-block instance and of the serial oracle, and what can go wrong is
what is new in it: which sighting of a k-mer counts as the first (the direction bias of a promoted key, the weight of its first
sighting) once ordinals are relative and cut to 31 bits, the strand bit at the word's other end, the rule that decides when the
instance may run at all, and a launch of half again as many blocks as the four-block one's.

Shapes, reads, oracle caches and rules are those of test_gpu_count_blocks.py:
  shape   "covered": 6 000 reads over 90 kb | "sparse": 30 000 reads at 2 % errors, an estimate a third of the truth
  k       31 (pad bits in the key word), 32 (none)
  rule    min_depth 2 | min_depth 1 with a separate singleton map
"count_six" 1 asks for the instance whatever the list count (the shapes here have a few hundred to a few thousand lists; the default
rule wants compute units x 6 x 24 of them, see test_default_rule_*).
"""
import functools

import numpy as np
import pytest
import torch
import torch.distributed as dist

from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, OracleSpectrum, ReadBatch
from test_gpu_count_blocks import RULES, _est, _is_oracle, _same
from test_gpu_count_instances import _build, _config, _oracle, _reads
from test_gpu_parity import add, compare_weak_images, product

pytestmark = pytest.mark.gpu


def _six_five_oracle(shape, k, est, rule, **tune):
    """the build with the six-block instance: it reports 6, has the bytes of the five-block build and is the oracle's"""
    sep, min_depth = RULES[rule]
    six = _build(shape, "flat", k, est, sep, min_depth, count_six=1, **tune)
    assert six.build_info("count_blocks") == 6 and six.build_info("uniform_count") == 1.0
    five = _build(shape, "flat", k, est, sep, min_depth, count_blocks=5, **tune)
    assert five.build_info("count_blocks") == 5
    _same(five, six, sep and min_depth == 1)
    stats = _is_oracle(six, shape, "flat", k, est, sep, min_depth)
    return six, five, stats


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("shape", ["covered", "sparse"])
def test_six_blocks_give_the_bytes_of_five_and_of_the_oracle(shape, k, rule):
    six, _, stats = _six_five_oracle(shape, k, _est(shape, k), rule)
    assert stats["weak_entries"] > 0
    assert six.build_info("count_attempts") == 1      # the slack covers the slab tails of six blocks per CU


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("k", [31, 32])
def test_sub_passes_with_six_blocks(k, rule):
    """estimated_raw_kmers = 1000: lists that overflow the LDS table are redone in sub-passes (the cold copy of the insert pass, the
    table cleared as a whole in between: the 32-bit words as well)"""
    _, _, stats = _six_five_oracle("covered", k, 1000, rule)
    assert stats["weak_entries"] > 18000


@pytest.mark.parametrize("rule", sorted(RULES))
def test_entry_buffers_grow_with_six_blocks(rule):
    """an entry share of next to nothing: more than one attempt, every one of them by the six-block instance"""
    sep, min_depth = RULES[rule]
    k, est = 31, _est("covered", 31)
    plain = _build("covered", "flat", k, est, sep, min_depth, count_blocks=5)
    small = _build("covered", "flat", k, est, sep, min_depth, count_six=1, entry_share=0.00001)
    assert small.build_info("count_attempts") > 1 and small.build_info("count_blocks") == 6
    _same(plain, small, sep and min_depth == 1)


def test_long_lists_beside_six_blocks():
    """long_list_chunks = 2: nearly every list is left to the pass over work items (four blocks, 64-bit words, the merge table); the
    six-block launch skips them and counts the rest"""
    six, _, _ = _six_five_oracle("covered", 31, _est("covered", 31), "depth2", long_list_chunks=2)
    plain = _build("covered", "flat", 31, _est("covered", 31), 1, 2, count_blocks=5)
    _same(plain, six, False)


def test_early_count_with_six_blocks():
    """kmr_count_lists_prefix (build_partitioned_superkmers with list_steps = 2, a job of one rank: nothing is adopted, every record
    is the handle's own): the lower half of the lists is counted early by the six-block instance, kmr_finalize counts the rest"""
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
        sp = product(_config(k, est, 0), 3, count_six=1)
        build_partitioned_superkmers(sp, tb, tq, to, first_read_idx=0, list_steps=2, early_min_depth=2)
        assert sp.build_info("count_blocks") == 6      # the early launch
        sp.finalize(2)
        assert sp.build_info("early_lists") == int(sp.build_info("lists")) // 2 and sp.build_info("early_overflowed") == 0
        assert sp.build_info("count_blocks") == 6 and sp.build_info("uniform_count") == 1.0
    finally:
        dist.destroy_process_group()
    _same(_build("covered", "flat", k, est, 0, 2, count_blocks=5), sp, False)
    _is_oracle(sp, "covered", "flat", k, est, 0, 2)


# ---- ordinals: the instance keeps (ordinal - lowest of the build) in 31 bits

def _fed(parts, origins, k, est, sep, min_depth, **tune):
    """a build fed one call per part, each from its own stream origin"""
    p = product(_config(k, est, sep), 3, **tune)
    for rb, origin in zip(parts, origins):
        p.set_stream_origin(origin)
        add(p, rb)
    p.finalize(min_depth)
    return p


def _halves(k):
    rb = _reads("covered", "flat", k)
    return rb.slice(0, rb.n // 2), rb.slice(rb.n // 2, rb.n)


@functools.lru_cache(maxsize=None)
def _oracle_second_half_first(k, est, sep, min_depth):
    """the serial oracle over the covered reads with the second half fed first"""
    a, b = _halves(k)
    o = OracleSpectrum(_config(k, est, sep))
    o.add_reads(b)
    o.add_reads(a, first_idx=b.n)
    o.finalize(min_depth)
    res = (o.stats(), o.image(KMR_MAP_WEAK).copy(), o.image(KMR_MAP_SINGLETON).copy())
    o.close()
    return res


@pytest.mark.parametrize("rule", sorted(RULES))
def test_origin_above_32_bits(rule):
    """one call from 2^33 + 12345: the base is not zero and does not fit 32 bits, the relative ordinals are those of a build from zero"""
    sep, min_depth = RULES[rule]
    k, est = 31, _est("covered", 31)
    p = _fed([_reads("covered", "flat", k)], [2**33 + 12345], k, est, sep, min_depth, count_six=1)
    assert p.build_info("count_blocks") == 6
    _is_oracle(p, "covered", "flat", k, est, sep, min_depth)
    _same(_fed([_reads("covered", "flat", k)], [2**33 + 12345], k, est, sep, min_depth, count_blocks=5), p, sep and min_depth == 1)


@pytest.mark.parametrize("rule", sorted(RULES))
def test_earliest_sighting_in_the_call_fed_later(rule):
    """two calls, the second from the lower origin: the build's lowest ordinal is only known after the first call's records are
    written, and the first sighting of a k-mer both halves hold lies in the call fed later -- the oracle is fed in ordinal order"""
    sep, min_depth = RULES[rule]
    k, est = 31, _est("covered", 31)
    a, b = _halves(k)
    p = _fed([a, b], [b.bases.size, 0], k, est, sep, min_depth, count_six=1)
    assert p.build_info("count_blocks") == 6 and p.build_info("uniform_count") == 1.0
    stats, weak, sing = _oracle_second_half_first(k, est, sep, min_depth)
    assert p.stats() == stats, (stats, p.stats())
    assert compare_weak_images(weak, p.image(KMR_MAP_WEAK), p.kb, False) == stats["weak_entries"]      # (dir_tol 0: the direction bias as well)
    if sep and min_depth == 1:
        assert np.array_equal(sing, p.image(KMR_MAP_SINGLETON))
    _same(_fed([a, b], [b.bases.size, 0], k, est, sep, min_depth, count_blocks=5), p, sep and min_depth == 1)
    # and the order of the halves matters to the bytes at all: fed in place, the other half's sightings come first
    _, weak0, _ = _oracle("covered", "flat", k, est, sep, min_depth)
    assert not np.array_equal(weak0, weak)


@pytest.mark.parametrize("span_is_2_31", [False, True])
def test_span_of_the_ordinals_decides(span_is_2_31):
    """origins 0 and 2^31 - (bases of the second call): the highest ordinal a base of the build can have is 2^31 - 1 above the lowest,
    the last span 31 bits hold: six blocks.  One base further on it is 2^31: the five-block instance, whatever "count_six" says.  The
    bytes are the oracle's either way."""
    k, est = 31, _est("covered", 31)
    a, b = _halves(k)
    second = 2**31 - int(b.bases.size) + (1 if span_is_2_31 else 0)
    p = _fed([a, b], [0, second], k, est, 1, 1, count_six=1)
    assert p.build_info("count_blocks") == (5 if span_is_2_31 else 6)
    _is_oracle(p, "covered", "flat", k, est, 1, 1)
    _same(_fed([a, b], [0, second], k, est, 1, 1, count_blocks=5), p, True)


@pytest.mark.parametrize("span_is_2_31", [False, True])
def test_span_with_absolute_offsets_in_the_second_call(span_is_2_31):
    """the same two spans fed as build_partitioned_superkmers feeds pieces: device calls over ONE offsets array, the second call's
    offsets absolute (they start at the first half's bases, not at zero) beside its stream origin -- its ordinals are origin + offset, so
    the highest lies the first half's bases above origin + the call's own bases, which only the offsets themselves tell"""
    k, est = 31, _est("covered", 31)
    rb = _reads("covered", "flat", k)
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(np.concatenate([rb.bases, np.zeros(64, np.uint8)])).to(dev)
    tq = torch.from_numpy(np.concatenate([rb.quals, np.zeros(64, np.uint8)])).to(dev)
    to = torch.from_numpy(rb.offsets.astype(np.int64)).to(dev)
    mid, total = rb.n // 2, int(rb.offsets[rb.n])
    first = int(rb.offsets[mid])
    origin = 2**31 - total + (1 if span_is_2_31 else 0)      # the last base of the second call: origin + total - 1
    p = product(_config(k, est, 1), 3, count_six=1)
    p.buildKmerSpectrumDevice(tb.data_ptr(), tq.data_ptr(), to.data_ptr(), mid, first, 0)
    p.set_stream_origin(origin)
    p.buildKmerSpectrumDevice(tb.data_ptr(), tq.data_ptr(), to.data_ptr() + 8 * mid, rb.n - mid, total - first, mid)
    p.finalize(1)
    assert p.build_info("count_blocks") == (5 if span_is_2_31 else 6)
    _is_oracle(p, "covered", "flat", k, est, 1, 1)


# ---- strands: bit 0 of the word

def _revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("k", [31, 32])
def test_first_sighting_on_either_strand(k, rule):
    """a few hand-made reads: every k-mer of s is seen first as s spells it and later from the other strand, every k-mer of u the
    other way round -- about half of each are forward at their first sighting and half reverse -- and the k-mers of v only once"""
    sep, min_depth = RULES[rule]
    rng = np.random.default_rng(5 + k)
    s, u, v = (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) for n in (97, 80, 64))
    seqs = [s, _revcomp(u), v, _revcomp(s), u, s]
    rb = ReadBatch(seqs, [b"I" * len(x) for x in seqs])
    est = sum(len(x) - k + 1 for x in seqs)
    o = OracleSpectrum(_config(k, est, sep))
    o.add_reads(rb)
    o.finalize(min_depth)
    built = {}
    for name, tune in (("six", {"count_six": 1}), ("five", {"count_blocks": 5})):
        p = product(_config(k, est, sep), 3, **tune)
        add(p, rb)
        p.finalize(min_depth)
        built[name] = p
    six = built["six"]
    assert six.build_info("count_blocks") == 6 and six.build_info("uniform_count") == 1.0
    assert six.stats() == o.stats(), (o.stats(), six.stats())
    assert o.stats()["weak_entries"] == (97 - k + 1) + (80 - k + 1)
    assert compare_weak_images(o.image(KMR_MAP_WEAK), six.image(KMR_MAP_WEAK), six.kb, False) == o.stats()["weak_entries"]
    if sep and min_depth == 1:
        assert np.array_equal(o.image(KMR_MAP_SINGLETON), six.image(KMR_MAP_SINGLETON))
    _same(built["five"], six, sep and min_depth == 1)
    # the batch does hold both cases: direction bias differs between keys (a promoted key loses its first sighting's direction)
    _, _, dirb, _, _ = o.entries()
    assert len(set(dirb.tolist())) > 1
    o.close()


# ---- the default rule

def test_default_rule_wants_lists_for_six_blocks_per_cu():
    """list_aim = 12: the covered reads cut into some 59 000 lists, more than compute units x 6 x 24 -- six blocks with no knob set, the
    bytes of the five-block instance over the same lists; "count_six" 2 keeps five.  (No CPU oracle at this list count.)"""
    k, est = 31, _est("covered", 31)
    need = torch.cuda.get_device_properties(0).multi_processor_count * 6 * 24
    d = _build("covered", "flat", k, est, 1, 1, list_aim=12)
    assert d.build_info("lists") >= need, (d.build_info("lists"), need)
    assert d.build_info("count_blocks") == 6 and d.build_info("uniform_count") == 1.0
    five = _build("covered", "flat", k, est, 1, 1, list_aim=12, count_blocks=5)
    assert five.build_info("count_blocks") == 5
    _same(five, d, True)
    never = _build("covered", "flat", k, est, 1, 1, list_aim=12, count_six=2)
    assert never.build_info("count_blocks") == 5
    _same(five, never, True)


def test_default_rule_keeps_small_builds_at_five():
    d = _build("covered", "flat", 31, _est("covered", 31), 1, 2)
    assert d.build_info("lists") < torch.cuda.get_device_properties(0).multi_processor_count * 6 * 24
    assert d.build_info("count_blocks") == 5


def test_count_six_takes_0_1_2_only_and_yields_to_count_blocks():
    p = product(_config(31, 1000, 1), 3)
    for bad in (3, -1, 0.5, 6):
        with pytest.raises(Exception):
            p.tune(count_six=bad)
    p.tune(count_six=0)
    for blocks in (4, 5):      # an explicit count_blocks means that instance
        q = _build("covered", "flat", 31, _est("covered", 31), 1, 2, count_six=1, count_blocks=blocks)
        assert q.build_info("count_blocks") == blocks


def test_general_form_ignores_count_six():
    """noisy qualities take the general form, which has one instance: four blocks, 64-bit words"""
    p = _build("covered", "noisy", 31, _est("covered", 31), 1, 1, count_six=1)
    assert p.build_info("uniform_count") == 0.0 and p.build_info("count_blocks") == 4
    _is_oracle(p, "covered", "noisy", 31, _est("covered", 31), 1, 1)
