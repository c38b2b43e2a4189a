"""CompareSpectrums on the device (kmr_compare_spectrums, kmr_compare_reads, kmr_reads_circularize; kmernator_amd/csrc/kmr_compare.hpp)
held to the restatement of tests/refcompare.py over the directed reads of tests/comparecases.py.  Every figure is an integer and
every comparison is for equality; no test builds a map with a saturated count, and saturated == 0 is asserted everywhere."""
import functools

import numpy as np
import pytest

import comparecases as cc
import kmernator_amd as ka
from helpers import default_config
from refcompare import FIELDS, HEADER, Comparer, evaluate, line, records_array

pytestmark = pytest.mark.gpu

KS = (21, 31, 33, 65, 97)          # one to four key words
TILE_SPAN = 9856 - 32              # kmr_kernels.hpp: the bases of one extraction tile
CAP = 256                          # kmr_compare.hpp: CMP_CAP


# ------------------------------------------------------------------------------------------------------------------- reference side
@functools.lru_cache(maxsize=None)
def comparer(k, min_weight=0.10):
    return Comparer(default_config(k, min_weight=min_weight))


@functools.lru_cache(maxsize=None)
def set2_map(k, min_weight=0.10, min_depth=1):
    m = comparer(k, min_weight).set_map(cc.set2())
    return {key: c for key, c in m.items() if c >= min_depth}


def pairs_of(fam):
    return [(s, q) for _, _, s, q in fam]


def want_records(k, fam, min_weight=0.10, min_depth=1):
    return records_array(comparer(k, min_weight).per_read(pairs_of(fam), set2_map(k, min_weight, min_depth)))


def same(got, want):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8], got[f][:8], want[f][:8])
    assert not got["saturated"].any()


# ---------------------------------------------------------------------------------------------------------------------- device side
def arrays_of(pairs):
    lens = np.array([len(s) for s, _ in pairs], dtype=np.uint64)
    off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    b = np.frombuffer(b"".join(s for s, _ in pairs) + b"\0", dtype=np.uint8)
    q = np.frombuffer(b"".join(q for _, q in pairs) + b"\0", dtype=np.uint8)
    return b, q, off


def read_set(sp, pairs):
    return ka.ReadSet.from_arrays(sp, *arrays_of(pairs))


def build(k, pairs, min_depth=1, sep=1, ext=False, min_weight=0.10, **cfg):
    sp = ka.KmerSpectrum(ka.default_config(k, device=0, separate_singletons=sep, value_kind=ka.KMR_VALUE_EXT if ext else ka.KMR_VALUE_COUNT_DIR, min_weight=min_weight,
                                           estimated_raw_kmers=max(4096, sum(len(s) for s, _ in pairs)), **cfg))
    if pairs:
        with read_set(sp, pairs) as rs:
            sp.buildKmerSpectrumFromReadSet(rs)
    sp.finalize(min_depth)
    return sp


class Handles:
    """set 2 built once per (k, variant) for the module's lifetime"""

    def __init__(self):
        self.sp = {}

    def set2(self, k, min_depth=1, sep=1, ext=False, min_weight=0.10):
        key = (k, min_depth, sep, ext, min_weight)
        if key not in self.sp:
            self.sp[key] = build(k, cc.set2(), min_depth, sep, ext, min_weight)
        return self.sp[key]

    def close(self):
        for sp in self.sp.values():
            sp.close()
        self.sp.clear()


@pytest.fixture(scope="module")
def dev():
    d = Handles()
    yield d
    d.close()


def compare(sp, pairs):
    with read_set(sp, pairs) as rs:
        return sp.compareReads(rs)


# ----------------------------------------------------------------------------------------------------------------------------- tests
VARIANTS = {"singletons_kept": dict(sep=1, min_depth=1), "one_map": dict(sep=0, min_depth=1), "ext_values": dict(sep=1, min_depth=1, ext=True),
            "min_depth_2": dict(sep=1, min_depth=2), "one_map_min_depth_2": dict(sep=0, min_depth=2)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("k", KS + (22,))
def test_families_per_read(dev, k, variant):
    v = VARIANTS[variant]
    fam = cc.families(k) + cc.batch_of(9, k)
    sp = dev.set2(k, **v)
    got = compare(sp, pairs_of(fam))
    same(got, want_records(k, fam, min_depth=v["min_depth"]))
    m2 = set2_map(k, 0.10, v["min_depth"])
    assert (got["size2"] == len(m2)).all() and (got["total_count2"] == sum(m2.values())).all()
    names = [f for f, _, _, _ in fam]
    a, b = [i for i, f in enumerate(names) if f == "strand"]
    assert got[a] == got[b]
    assert got[names.index("short")]["size1"] == 0 and got[names.index("exact")]["size1"] == 1 and got[names.index("kplus1")]["total_count1"] == 2
    if v["min_depth"] == 1:
        so = got[names.index("singleton_only")]
        assert so["common"] == so["size1"] == so["common_count2"] > 0


def test_weight_test_at_min_weight_zero(dev):
    k = 21
    fam = cc.families(k)
    lax, strict = compare(dev.set2(k, min_weight=0.0), pairs_of(fam)), compare(dev.set2(k), pairs_of(fam))
    same(lax, want_records(k, fam, min_weight=0.0))
    i = [f for f, _, _, _ in fam].index("low_quality")
    assert strict[i]["size1"] < lax[i]["size1"] == len(fam[i][2]) - k + 1


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_batch_sizes(dev, n):
    k = 31
    fam = cc.batch_of(n, k)
    got = compare(dev.set2(k), pairs_of(fam))
    assert got.shape == (n,)
    same(got, want_records(k, fam))


@functools.lru_cache(maxsize=None)
def cap_batch(k):
    return cc.cap_mix(k, CAP, TILE_SPAN) + cc.cap_mix(k, 8, 40)[:6] + cc.families(k)


SETTINGS = {"default": {}, "cap_8": dict(compare_lds_kmers=8), "cap_0": dict(compare_lds_kmers=0), "runs": dict(compare_stage_kmers=300),
            "runs_cap_8": dict(compare_stage_kmers=300, compare_lds_kmers=8), "runs_cap_0": dict(compare_stage_kmers=97, compare_lds_kmers=0)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("k", [31, 33, 65, 97])
def test_records_do_not_depend_on_cap_or_staging(dev, k, setting):
    """reads of CAP - 1, CAP and CAP + 1 k-mers and one of several tile spans; a staging budget that forces several runs and a lone
    oversize read.  One to four key words: the sorted path (cap_0) takes one sort pass per word and one more, and its order ends in
    a different buffer for an odd and an even count.  The families bring a read of one k-mer and an empty read"""
    fam = cap_batch(k)
    sp = dev.set2(k)
    try:
        sp.tune(**SETTINGS[setting])
        got = compare(sp, pairs_of(fam))
    finally:
        sp.tune(compare_lds_kmers=-1, compare_stage_kmers=0)
    same(got, want_records(k, fam))


WHOLE = {
    "overlapping": lambda k: pairs_of(cc.families(k)) + cc.set2()[:40],
    "identical": lambda k: cc.set2(),
    "disjoint": lambda k: [(cc.random_bases(300, 123), b"I" * 300)],
    "empty_set_1": lambda k: [],
}


@pytest.mark.parametrize("case", sorted(WHOLE))
@pytest.mark.parametrize("k", [21, 33, 65, 97])
def test_whole_form(dev, k, case):
    pairs = WHOLE[case](k)
    h2 = dev.set2(k)
    m1, m2 = comparer(k).set_map(pairs), set2_map(k)
    for cfg in (dict(sep=1), dict(sep=0), dict(sep=1, num_buckets_weak=64, num_buckets_singleton=16)):      # equal and different bucket counts
        with_h1 = build(k, pairs, 1, **cfg)
        try:
            assert with_h1.countCommonKmers(h2) == evaluate(m1, m2)
            assert h2.countCommonKmers(with_h1) == evaluate(m2, m1)      # (an empty set on either side)
        finally:
            with_h1.close()
    if case == "identical":
        assert h2.countCommonKmers(h2) == evaluate(m2, m2)
        r = h2.countCommonKmers(h2)
        assert r["common"] == r["size1"] == r["size2"] and r["common_count1"] == r["common_count2"] == r["total_count1"]


def test_whole_form_min_depth_2_and_value_kinds(dev):
    k = 31
    a, b = dev.set2(k, min_depth=2), dev.set2(k, ext=True)
    assert a.countCommonKmers(b) == evaluate(set2_map(k, 0.10, 2), set2_map(k))
    assert b.countCommonKmers(a) == evaluate(set2_map(k), set2_map(k, 0.10, 2))


@pytest.mark.parametrize("k", [31, 65])
def test_per_read_record_equals_whole_form_of_that_read(dev, k):
    fam = cc.families(k)
    h2 = dev.set2(k)
    got = compare(h2, pairs_of(fam))
    for i, (s, q) in enumerate(pairs_of(fam)):
        h1 = build(k, [(s, q)], 1, sep=i % 2)
        try:
            assert h1.countCommonKmers(h2) == {f: int(got[i][f]) for f in FIELDS}, fam[i][1]
        finally:
            h1.close()


@pytest.mark.parametrize("extra", [0, None, 10 ** 6])
def test_circularize(dev, extra):
    k = 31
    sp = dev.set2(k)
    pairs = pairs_of(cc.circular(k) + cc.families(k)[:4])
    want = comparer(k).circularize(pairs, extra)
    with read_set(sp, pairs) as rs, rs.circularize(extra) as circ:
        b, q, off, names = circ.arrays()
        wb, wq, woff = arrays_of(want)
        assert np.array_equal(off, woff) and np.array_equal(b, wb[:-1]) and np.array_equal(q, wq[:-1])
        assert circ.n == rs.n and circ.total_bases == int(woff[-1])
        same(sp.compareReads(circ), records_array(comparer(k).per_read(want, set2_map(k))))


def fastq_of(fam):
    return b"".join(b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n" for _, name, s, q in fam if s and q[0] != 0x7f)


def test_compare_spectrums_text(dev):
    """the tool's output: header and lines, per read with the reads' names and --circular-reference, and set against set"""
    k = 31
    sp = dev.set2(k)
    fam = [r for r in cc.families(k) + cc.circular(k) if r[2] and r[3][0] != 0x7f]
    with ka.ReadSet(sp, fastq_of(fam)) as rs:
        assert rs.n == len(fam)
        c = comparer(k)
        want = HEADER + b"".join(line(r, f[1]) for r, f in zip(c.per_read(pairs_of(fam), set2_map(k)), fam))
        assert ka.CompareSpectrums(sp, rs, per_read=True) == want
        circ = c.circularize(pairs_of(fam))
        want = HEADER + b"".join(line(r, f[1]) for r, f in zip(c.per_read(circ, set2_map(k)), fam))
        assert ka.CompareSpectrums(sp, rs, per_read=True, circular_reference=True) == want
        assert ka.CompareSpectrums(sp, rs) == HEADER + line(evaluate(c.set_map(pairs_of(fam)), set2_map(k)))
        assert ka.CompareSpectrums(sp, rs, circular_reference=True) == HEADER + line(evaluate(c.set_map(circ), set2_map(k)))


def test_device_records(dev):
    """kmr_compare_reads_dev: the records in device memory, written by work on the handle's stream"""
    import ctypes as C
    import torch
    k = 31
    sp = dev.set2(k)
    fam = cap_batch(k)
    with read_set(sp, pairs_of(fam)) as rs:
        out = torch.zeros(rs.n * 8, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        sp._call("compare_reads_dev", sp.h, rs.r, C.c_void_p(out.data_ptr()))
        sp.sync()
        got = out.cpu().numpy().view(np.uint64).view(ka.COMPARE_DTYPE).reshape(-1)
    same(got, want_records(k, fam))


def test_refusals(dev):
    k = 31
    h2 = dev.set2(k)
    pairs = pairs_of(cc.families(k)[:3])
    raw = ka.KmerSpectrum(ka.default_config(k, device=0, estimated_raw_kmers=4096))
    try:
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
            raw.countCommonKmers(h2)
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
            h2.countCommonKmers(raw)
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_STATE"):
            compare(raw, pairs)
    finally:
        raw.close()
    with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
        dev.set2(33).countCommonKmers(h2)
    other_hash = build(k, pairs, 1, hash_kind=1)
    try:
        with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_INVALID_ARG"):
            other_hash.countCommonKmers(h2)
    finally:
        other_hash.close()
    for part in (dict(world_size=2, rank=1), dict(num_parts=2, part_idx=1), dict(kmer_subsample=3)):
        sp = build(k, pairs, 1, **part)
        try:
            with pytest.raises(ka.KmerSpectrumError, match="KMR_ERR_UNSUPPORTED"):
                compare(sp, pairs)
        finally:
            sp.close()
