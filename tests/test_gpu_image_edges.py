"""kmr_load_image, kmr_merge_image and kmr_write_image, and what reads the maps they leave (lookups, both histograms), on the
directed images of tests/imagecases.py, held to tests/refimage.py byte for byte.  Every case uses a fresh handle of its k and value
kind and builds nothing; the largest image holds about two thousand entries.

What runs where (W = key words of k, VW = value words the bucket sort moves: 3 weak, 15 weak with extensions, 0 singleton):
  sort_buckets_kernel   the `fills` images hold buckets of 1, 2, 3, 63, 64 (shuffle rank sort), 65, 66, 128, 191, 255, 256 (four
                        entries per lane) and 257, 600 entries (heap sort): test_load[k-kind] runs all three paths at
                        (W, VW) = (words of k, words of kind), stored sorted, reversed and shuffled; the "cross" merges reach a
                        path only with the union of two maps
  multi-word order      `shared_words` in test_load (key_lt, the rank sorts, map_find's binary search)
  bucket of an entry    `sparse`, `empty`, `one_bucket` and the empty buckets of `fills` in test_load (image_entries_kernel,
                        image_unpack_kernel) and in test_merge's "b_empty" / "a_empty" (merge_copy_kernel)
  ref_histogram_kernel  test_histograms[k-kind] "values_wide" at zoom 1000: counts 512..1000 take the global-atomic branch
No image whose offsets or counts are out of range reaches a kernel: test_refusals asserts that the host refuses them."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import imagecases as ic
import kmernator_amd as ka
import refimage as ri
from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_EXT

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -7


def handle(k, kind):
    return ka.KmerSpectrum(ka.default_config(k, device=0, value_kind=KMR_VALUE_EXT if kind.endswith("ext") else 0))


def which_of(kind):
    return KMR_MAP_WEAK if ri.is_weak(kind) else KMR_MAP_SINGLETON


def as_array(image):
    return np.frombuffer(bytes(image), dtype=np.uint8)


def entries_stat(kind):
    return "weak_entries" if ri.is_weak(kind) else "singleton_entries"


def call(sp, name, which, image, shift=0):
    """kmr_load_image / kmr_merge_image on exactly len(image) bytes that stand `shift` bytes into a buffer: (status, message)"""
    buf = np.zeros(len(image) + shift + 1, dtype=np.uint8)
    buf[shift:shift + len(image)] = as_array(image)
    rc = getattr(sp.lib, "kmr_" + name)(sp.h, which, C.c_void_p(buf.ctypes.data + shift), len(image))
    return rc, (sp.lib.kmr_last_error(sp.h).decode() if rc else "")


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def check_lookups(sp, keys, weak, sing, what):
    """getCount(keys) and getCount(keys, useWeights=True) equal refimage.lookup, the weights by their f64 bits"""
    want = [ri.lookup(weak, sing, key) for key in keys]
    packed = np.frombuffer(b"".join(keys), dtype=np.uint8)
    assert [int(c) for c in sp.getCount(packed)] == [c for c, _ in want], what
    assert np.array_equal(bits(sp.getCount(packed, useWeights=True)), bits([w for _, w in want])), what


def check_device_lookups(sp, k, keys, weak, sing, what):
    """kmr_lookup_keys_dev (the weak map's count) and kmr_lookup_keys_weighted_dev (weak, then singleton) over key words on the
    device, through the lookup table and through the bucket search"""
    import torch
    dev = torch.device("cuda", 0)
    W, kb = ic.words_of(k), ic.kb_of(k)
    padded = np.zeros((len(keys), 8 * W), dtype=np.uint8)
    padded[:, :kb] = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), kb)
    words = torch.from_numpy(padded.view(">u8").astype(np.int64)).to(dev)
    for lut in (1, 0):
        sp.tune(lookup_table=lut)
        counts = torch.full((len(keys),), -1, dtype=torch.int32, device=dev)
        weights = torch.full((len(keys),), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        sp.lookup_keys(words, len(keys), counts)
        sp.lookup_keys_weighted(words, len(keys), weights)
        sp.sync()
        assert [int(c) for c in counts.cpu().numpy()] == [ri.lookup(weak, {}, key)[0] for key in keys], (what, lut)
        assert np.array_equal(bits(weights.cpu().numpy()), bits([ri.lookup(weak, sing, key)[1] for key in keys])), (what, lut)
    sp.tune(lookup_table=1)


@functools.lru_cache(maxsize=32)
def expected(image, k, kind):
    """(stored form, entries, weak table, singleton table, the keys to ask for) of the map of `image`, computed once"""
    kb = ic.kb_of(k)
    table = ri.table_of(image, kb, kind)
    weak, sing = (table, {}) if ri.is_weak(kind) else ({}, table)
    return ri.canonical(image, kb, kind), ri.entry_count(image, kb, kind), weak, sing, ic.stored_keys(image, k, kind) + ic.absent_keys(image, k, kind)


def check_map(sp, k, kind, image, what, device_lookups=True):
    """the handle's map of this kind is the map of `image`: its stored form, its entry count, every stored key and 64 absent ones"""
    stored, n, weak, sing, keys = expected(image, k, kind)
    assert sp.image(which_of(kind)).tobytes() == stored, what
    assert sp.stats()[entries_stat(kind)] == n, what
    check_lookups(sp, keys, weak, sing, what)
    if device_lookups:
        check_device_lookups(sp, k, keys, weak, sing, what)


# ---------------------------------------------------------------------------------------------------------------------- load
@pytest.mark.parametrize("kind", ri.KINDS)
@pytest.mark.parametrize("k", ic.KS)
def test_load(k, kind):
    for name, image in ic.load_cases(k, kind):
        sp = handle(k, kind)
        sp.load_image(which_of(kind), as_array(image))
        check_map(sp, k, kind, image, name)
        sp.close()


@pytest.mark.parametrize("ext", (False, True))
@pytest.mark.parametrize("k", ic.KS)
def test_weak_before_singleton(k, ext):
    """a weak and a singleton image in one handle: a key both hold answers from the weak map, the others from their own"""
    kb = ic.kb_of(k)
    wkind, skind = ("weak_ext", "sing_ext") if ext else ("weak", "sing")
    wimg, simg = ic.image_of(ic.values(k, wkind), k, wkind), ic.both_maps_singleton(k, skind)
    sp = handle(k, wkind)
    sp.load_image(KMR_MAP_WEAK, as_array(wimg))
    sp.load_image(KMR_MAP_SINGLETON, as_array(simg))
    weak, sing = ri.table_of(wimg, kb, wkind), ri.table_of(simg, kb, skind)
    keys = sorted(set(weak) | set(sing)) + ic.absent_keys(simg, k, skind)
    check_lookups(sp, keys, weak, sing, "both maps")
    check_device_lookups(sp, k, keys, weak, sing, "both maps")
    assert sp.image(KMR_MAP_WEAK).tobytes() == ri.canonical(wimg, kb, wkind)
    assert sp.image(KMR_MAP_SINGLETON).tobytes() == ri.canonical(simg, kb, skind)
    sp.close()


@pytest.mark.parametrize("k,kind", ((31, "sing"), (97, "sing_ext"), (31, "weak"), (97, "weak_ext")))
def test_the_map_not_loaded_is_stored_as_empty_buckets(k, kind):
    """a handle that loaded one map only stores the other as its bucket count of empty buckets (what a restore of one file and a
    store of both writes), from the host: no kernel is given the map that is not there"""
    image = ic.image_of(ic.values(k, kind), k, kind)
    sp = handle(k, kind)
    sp.load_image(which_of(kind), as_array(image))
    other = KMR_MAP_SINGLETON if ri.is_weak(kind) else KMR_MAP_WEAK
    other_kind = {"weak": "sing", "weak_ext": "sing_ext", "sing": "weak", "sing_ext": "weak_ext"}[kind]
    nb = sp.num_buckets(other)
    assert nb >= 1 and sp.image(other).tobytes() == ri.pack(nb, [[] for _ in range(nb)], ic.kb_of(k), other_kind)
    check_map(sp, k, kind, image, "the loaded map")
    sp.close()


# ---------------------------------------------------------------------------------------------------------------------- histograms
def check_weight_sums(got, terms, what):
    """visitedWeight of every bucket.  Where every term is a weak map's weight (a multiple of 2^-7 below 2^17) every order of
    addition is exact, so the sum is held to the bit.  A singleton's (w - 1) / 254 is not dyadic: there the device's sum of the
    n nonnegative terms, added in whatever order its atomics fall, is held to the standard bound of recursive summation against
    the exact sum (taken in rationals): |got - sum| <= (n - 1) 2^-53 sum"""
    rest = np.array(got, dtype=np.float64)
    rest[list(terms)] = 0.0
    assert not rest.any(), what
    for idx, recs in terms.items():
        exact = sum(Fraction(w) for _, w in recs)
        if all(w * 128 == int(w * 128) for _, w in recs):
            assert Fraction(float(got[idx])) == exact, (what, idx)
        else:
            assert abs(Fraction(float(got[idx])) - exact) <= (len(recs) - 1) * Fraction(1, 1 << 53) * exact, (what, idx, float(got[idx]), float(exact))


@pytest.mark.parametrize("kind", ("weak", "weak_ext"))
@pytest.mark.parametrize("k", (13, 33, 64, 127))
def test_histograms(k, kind):
    """getHistogram(256, 2.0), (15, 1.5) and (1000, 2.0) and histogram(n_bins) of loaded handles that hold a weak map and the
    `values` singleton map: visits and visitedCount exact, the weights as check_weight_sums says.  "values_wide" at zoom 1000 puts
    a hundred entries at indices 512..1000, which ref_histogram_kernel adds by global atomics (HIST_LDS = 512)"""
    kb = ic.kb_of(k)
    skind = "sing_ext" if kind == "weak_ext" else "sing"
    simg = ic.image_of(ic.values(k, skind), k, skind)
    sing = ri.table_of(simg, kb, skind)
    for name, wimg in ic.load_cases(k, kind) + [("values_wide", ic.image_of(ic.values(k, kind, True), k, kind))]:
        sp = handle(k, kind)
        sp.load_image(KMR_MAP_WEAK, as_array(wimg))
        sp.load_image(KMR_MAP_SINGLETON, as_array(simg))
        weak = ri.table_of(wimg, kb, kind)
        for zoom, base in ((256, 2.0), (15, 1.5), (1000, 2.0)):
            h = sp.getHistogram(zoom, base)
            visits, vcount, _ = ri.histogram(weak, sing, zoom, base)
            assert [int(x) for x in h.visits] == visits and [int(x) for x in h.visitedCount] == vcount, (name, zoom, base)
            terms = ri.histogram_terms(weak, sing, zoom, base)
            check_weight_sums(h.visitedWeight, terms, (name, zoom, base))
            if name == "values_wide" and zoom == 1000:
                assert sum(len(r) for i, r in terms.items() if i >= 512) >= 90
        for n_bins in (2, 64, 70000):
            counts, weights = sp.histogram(n_bins)
            rc, _ = ri.count_histogram(weak, n_bins)
            assert [int(x) for x in counts] == rc, (name, n_bins)
            terms = {}
            for v in weak.values():
                terms.setdefault(min(v[0], n_bins - 1), []).append((v[0], ri.f32_of_bits(v[1])))
            check_weight_sums(weights, terms, (name, n_bins))
        sp.close()


# ---------------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("kind", ("weak", "weak_ext"))
@pytest.mark.parametrize("k", ic.KS)
def test_merge(k, kind):
    """load A, merge_image(B) (and C, for the chain): the handle's map is canonical(merge_add(A, B)); a map of another bucket
    count is refused and leaves the handle as it was"""
    kb = ic.kb_of(k)
    for name in ic.MERGES:
        images = ic.merge_case(name, k, kind)
        sp = handle(k, kind)
        sp.load_image(KMR_MAP_WEAK, as_array(images[0]))
        want = images[0]
        for image in images[1:]:
            sp.merge_image(KMR_MAP_WEAK, as_array(image))
            want = ri.merge_add(want, image, kb, kind)
        check_map(sp, k, kind, want, name, device_lookups=name in ("half_shared", "cross_250_250_240"))
        sp.close()
    a, b = ic.merge_case("nb16_vs_32", k, kind)
    sp = handle(k, kind)
    sp.load_image(KMR_MAP_WEAK, as_array(a))
    before = sp.image(KMR_MAP_WEAK).tobytes()
    rc, message = call(sp, "merge_image", KMR_MAP_WEAK, b)
    assert rc == INVALID_ARG and "differing" in message
    assert sp.image(KMR_MAP_WEAK).tobytes() == before == ri.canonical(a, kb, kind)
    check_map(sp, k, kind, a, "after the refused merge", device_lookups=False)
    sp.close()


@pytest.mark.parametrize("kind", ("sing", "sing_ext"))
@pytest.mark.parametrize("k", ic.KS)
def test_merge_singletons(k, kind):
    """disjoint singleton maps merge; maps that share one key are refused (the key would have to move to the weak map) and the
    handle keeps its map"""
    kb = ic.kb_of(k)
    a, b = ic.merge_case("sing_disjoint", k, kind)
    sp = handle(k, kind)
    sp.load_image(KMR_MAP_SINGLETON, as_array(a))
    sp.merge_image(KMR_MAP_SINGLETON, as_array(b))
    check_map(sp, k, kind, ri.merge_add(a, b, kb, kind), "sing_disjoint")
    sp.close()
    a, b = ic.merge_case("sing_share_one", k, kind)
    with pytest.raises(ri.Refused, match="share"):
        ri.merge_add(a, b, kb, kind)
    sp = handle(k, kind)
    sp.load_image(KMR_MAP_SINGLETON, as_array(a))
    before = sp.image(KMR_MAP_SINGLETON).tobytes()
    rc, message = call(sp, "merge_image", KMR_MAP_SINGLETON, b)
    assert rc == UNSUPPORTED and "share" in message
    assert sp.image(KMR_MAP_SINGLETON).tobytes() == before == ri.canonical(a, kb, kind)
    check_map(sp, k, kind, a, "after the refused merge", device_lookups=False)
    sp.close()


# ---------------------------------------------------------------------------------------------------------------------- refusals
REFUSAL_SHAPES = ((13, "weak"), (31, "weak"), (31, "sing"), (33, "weak_ext"), (127, "sing_ext"))


@pytest.mark.parametrize("k,kind", REFUSAL_SHAPES)
def test_refusals_on_a_fresh_handle(k, kind):
    """every malformed image is refused with its message, from an even and from an odd address; the handle is as fresh as before:
    merging into it is still a state error, and a well-formed image loads"""
    sp = handle(k, kind)
    for name, image, message in ic.malformed(k, kind):
        for shift in (0, 1):
            rc, got = call(sp, "load_image", which_of(kind), image, shift)
            assert rc == INVALID_ARG and message in got, (name, shift, rc, got)
    rc, got = call(sp, "merge_image", which_of(kind), ic.image_of(ic.fills(k, kind), k, kind))
    assert rc == -5 and "before" in got
    good = ic.image_of(ic.fills(k, kind, "reversed"), k, kind)
    sp.load_image(which_of(kind), as_array(good))
    check_map(sp, k, kind, good, "a load after the refusals", device_lookups=False)
    sp.close()


@pytest.mark.parametrize("k,kind", REFUSAL_SHAPES)
def test_refused_load_keeps_the_map(k, kind):
    """a handle that holds map A refuses every malformed image, to load and to merge, and answers A afterwards: its stored form,
    its entry count and its lookups"""
    kb = ic.kb_of(k)
    a = ic.image_of(ic.fills(k, kind, "shuffled"), k, kind)
    sp = handle(k, kind)
    sp.load_image(which_of(kind), as_array(a))
    check_map(sp, k, kind, a, "before")
    for name, image, message in ic.malformed(k, kind):
        for fn in ("load_image", "merge_image"):
            rc, got = call(sp, fn, which_of(kind), image, 1)
            assert rc == INVALID_ARG and message in got, (name, fn, rc, got)
            check_map(sp, k, kind, a, (name, fn), device_lookups=False)
    check_map(sp, k, kind, a, "after")
    sp.close()
