"""The directed stored-map images of tests/imagecases.py, on the CPU: tests/refimage.py (the format and the merge restated plainly)
against the oracle on every well-formed image and every weak merge pair, each family shown to notice the rule it was written
for, and the generator held to its own quotas, so that tests/test_gpu_image_edges.py tests the shapes it says it does."""
import numpy as np
import pytest

import imagecases as ic
import refimage as ri
from helpers import KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_EXT, OracleSpectrum, default_config

KINDS = ri.KINDS


def oracle(k, kind):
    return OracleSpectrum(default_config(k, value_kind=KMR_VALUE_EXT if kind.endswith("ext") else 0))


def which_of(kind):
    return KMR_MAP_WEAK if ri.is_weak(kind) else KMR_MAP_SINGLETON


def as_array(image):
    return np.frombuffer(bytes(image), dtype=np.uint8)


def padding_zeroed(image, kb, kind):
    """the image with every weak value's struct padding zeroed and nothing else touched: the stored order stays"""
    nb, mask, buckets = ri.parse(image, kb, kind)
    return ri.pack(nb, [[(key, ri.zero_padding(v, kind)) for key, v in b] for b in buckets], kb, kind, mask)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ic.KS)
def test_pack_and_parse_are_inverse(k, kind):
    for name, image in ic.load_cases(k, kind):
        nb, buckets = ic.FAMILIES[name.split("-")[0]](k, kind, *name.split("-")[1:])
        assert ri.parse(image, ic.kb_of(k), kind) == (nb, nb - 1, buckets), name
        assert len(image) == 16 + 12 * nb + sum(len(b) for b in buckets) * (ic.kb_of(k) + ri.VBYTES[kind]), name
    for name in (ic.MERGES + ("nb16_vs_32",) if ri.is_weak(kind) else ic.SING_MERGES):
        for image in ic.merge_case(name, k, kind):
            nb, mask, buckets = ri.parse(image, ic.kb_of(k), kind)
            assert ri.pack(nb, buckets, ic.kb_of(k), kind, mask) == image, name


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ic.KS)
def test_oracle_restores_stores_and_looks_up(k, kind):
    """The oracle loads every well-formed image; what it stores again is canonical(image).  The oracle sorts every bucket before it
    stores (resort), so the stored order is compared too; it carries a weak value's struct padding along as the reference's memcpy
    of the struct does, where the device writes zeros, so the padding is zeroed on the oracle's side before the comparison and
    nothing else is.  Its counts of every stored key and of 64 absent ones equal refimage.lookup"""
    kb = ic.kb_of(k)
    for name, image in ic.load_cases(k, kind):
        o = oracle(k, kind)
        o.load_image(which_of(kind), as_array(image))
        back = o.image(which_of(kind)).tobytes()
        assert padding_zeroed(back, kb, kind) == ri.canonical(image, kb, kind), name
        assert o.stats()["weak_entries" if ri.is_weak(kind) else "singleton_entries"] == ri.entry_count(image, kb, kind)
        table = ri.table_of(image, kb, kind)
        weak, sing = (table, {}) if ri.is_weak(kind) else ({}, table)
        keys = ic.stored_keys(image, k, kind) + ic.absent_keys(image, k, kind)
        got = o.lookup(np.frombuffer(b"".join(keys), dtype=np.uint8))
        assert [int(c) for c in got] == [ri.lookup(weak, sing, key)[0] for key in keys], name
        o.close()


@pytest.mark.parametrize("k", ic.KS)
def test_weak_before_singleton(k):
    """a key both maps hold answers from the weak map (DataPointers::getCount): the singleton image holds the weak image's keys"""
    kb = ic.kb_of(k)
    wimg = ic.image_of(ic.values(k, "weak"), k, "weak")
    simg = ic.both_maps_singleton(k, "sing")
    o = oracle(k, "weak")
    o.load_image(KMR_MAP_WEAK, as_array(wimg))
    o.load_image(KMR_MAP_SINGLETON, as_array(simg))
    weak, sing = ri.table_of(wimg, kb, "weak"), ri.table_of(simg, kb, "sing")
    assert set(weak) & set(sing) and set(sing) - set(weak)
    keys = sorted(set(weak) | set(sing))
    got = o.lookup(np.frombuffer(b"".join(keys), dtype=np.uint8))
    assert [int(c) for c in got] == [ri.lookup(weak, sing, key)[0] for key in keys]


@pytest.mark.parametrize("kind", ("weak", "weak_ext"))
@pytest.mark.parametrize("k", ic.KS)
def test_oracle_merge_add(k, kind):
    """orc_merge_add (mergeAdd of the weak maps) against refimage.merge_add, byte for byte but for the struct padding, which the
    oracle carries along (zeroed on both sides); the chain merges its third map into the result of the first two"""
    kb = ic.kb_of(k)
    for name in ic.MERGES:
        images = ic.merge_case(name, k, kind)
        acc = oracle(k, kind)
        acc.load_image(KMR_MAP_WEAK, as_array(images[0]))
        want = images[0]
        for image in images[1:]:
            other = oracle(k, kind)
            other.load_image(KMR_MAP_WEAK, as_array(image))
            acc.merge_add(other)
            want = ri.merge_add(want, image, kb, kind)
            other.close()
        assert padding_zeroed(acc.image(KMR_MAP_WEAK).tobytes(), kb, kind) == ri.canonical(want, kb, kind), name
        acc.close()
    a, b = ic.merge_case("nb16_vs_32", k, kind)
    with pytest.raises(ri.Refused, match="differing"):
        ri.merge_add(a, b, kb, kind)
    o1, o2 = oracle(k, kind), oracle(k, kind)
    o1.load_image(KMR_MAP_WEAK, as_array(a))
    o2.load_image(KMR_MAP_WEAK, as_array(b))
    with pytest.raises(RuntimeError):
        o1.merge_add(o2)


@pytest.mark.parametrize("k", (31, 97))
def test_singleton_merges(k):
    a, b = ic.merge_case("sing_disjoint", k, "sing")
    merged = ri.parse(ri.merge_add(a, b, ic.kb_of(k), "sing"), ic.kb_of(k), "sing")
    assert sum(map(len, merged[2])) == ri.entry_count(a, ic.kb_of(k), "sing") + ri.entry_count(b, ic.kb_of(k), "sing")
    a, b = ic.merge_case("sing_share_one", k, "sing")
    assert len(set(ic.stored_keys(a, k, "sing")) & set(ic.stored_keys(b, k, "sing"))) == 1
    with pytest.raises(ri.Refused, match="share"):
        ri.merge_add(a, b, ic.kb_of(k), "sing")


HISTOGRAMS = ((256, 2.0), (15, 1.5), (1000, 2.0))


@pytest.mark.parametrize("kind", ("weak", "weak_ext"))
@pytest.mark.parametrize("k", (13, 33, 127))
def test_oracle_histograms(k, kind):
    """orc_histogram against refimage.histogram in visits and visitedCount, of a weak and a singleton map in one spectrum; the
    weights too, to the bit: the oracle adds in bucket order as refimage does, and every weak weight is dyadic"""
    kb = ic.kb_of(k)
    skind = "sing_ext" if kind == "weak_ext" else "sing"
    for name, wimg in ic.load_cases(k, kind) + [("values_wide", ic.image_of(ic.values(k, kind, True), k, kind))]:
        simg = ic.image_of(ic.values(k, skind), k, skind)
        o = oracle(k, kind)
        o.load_image(KMR_MAP_WEAK, as_array(wimg))
        o.load_image(KMR_MAP_SINGLETON, as_array(simg))
        weak, sing = ri.table_of(wimg, kb, kind), ri.table_of(simg, kb, skind)
        for zoom, base in HISTOGRAMS:
            v, c, w = o.ref_histogram(zoom, base)
            rv, rc, rw = ri.histogram(weak, sing, zoom, base)
            assert [int(x) for x in v] == rv and [int(x) for x in c] == rc, (name, zoom, base)
            assert np.array_equal(w.view(np.uint64), np.array(rw, np.float64).view(np.uint64)), (name, zoom, base)
        for n_bins in (2, 64, 70000):
            c, w = o.histogram(n_bins)
            rc, rw = ri.count_histogram(weak, n_bins)
            assert [int(x) for x in c] == rc and [float(x) for x in w] == rw, (name, n_bins)
        o.close()


# ---------------------------------------------------------------------------------------------------------------------- every family notices
@pytest.mark.parametrize("k", [k for k in ic.KS if ic.words_of(k) > 1])
def test_shared_words_notices_an_order_by_the_first_word(k):
    for kind in KINDS:
        image = ic.image_of(ic.shared_words(k, kind), k, kind)
        assert ri.canonical(image, ic.kb_of(k), kind, wrong="first_word_only") != ri.canonical(image, ic.kb_of(k), kind)


@pytest.mark.parametrize("k", ic.KS)
def test_families_notice_their_rules(k):
    kb = ic.kb_of(k)
    for kind in ("weak", "weak_ext"):
        a, b = ic.merge_case("equal", k, kind)
        assert ri.merge_add(a, b, kb, kind, wrong="saturating_count") != ri.merge_add(a, b, kb, kind)
        image = ic.image_of(ic.values(k, kind), k, kind)
        assert ri.canonical(image, kb, kind, wrong="padding_kept") != ri.canonical(image, kb, kind)
        wide = ri.table_of(ic.image_of(ic.values(k, kind, True), k, kind), kb, kind)
        assert ri.histogram(wide, {}, 1000, 2.0, wrong="clamp_511") != ri.histogram(wide, {}, 1000, 2.0)
        plain = ri.table_of(image, kb, kind)      # the plain `values` family alone would not: no index of its own reaches 512
        assert ri.histogram(plain, {}, 256, 2.0, wrong="clamp_511") == ri.histogram(plain, {}, 256, 2.0)
    for kind in KINDS:
        for name, image in ic.load_cases(k, kind):
            parsed = ri.parse(image, kb, kind)
            start, entries = ri.flatten(parsed)
            assert ri.unflatten(parsed[0], start, entries) == parsed[2], name
            wrong = ri.unflatten(parsed[0], start, entries, wrong="bucket_search") != parsed[2]
            if name in ("sparse", "fills-sorted", "fills-reversed", "fills-shuffled"):
                assert wrong, name
            if name in ("one_bucket", "empty"):
                assert not wrong, name


# ---------------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("k", ic.KS)
def test_every_quota_is_met(k):
    kb = ic.kb_of(k)
    for kind in KINDS:
        per_order = []
        for order in ic.ORDERS:
            nb, buckets = ic.fills(k, kind, order)
            assert nb == 16 and tuple(len(b) for b in buckets) == ic.FILLS
            keys = [[key for key, _ in b] for b in buckets]
            if order == "sorted":
                assert all(b == sorted(b) for b in keys)
            if order == "reversed":
                assert all(b == sorted(b)[::-1] for b in keys)
            if order == "shuffled":
                assert all(b != sorted(b) and b != sorted(b)[::-1] for b in keys if len(b) > 3)
            per_order.append([sorted(b) for b in buckets])
        assert per_order[0] == per_order[1] == per_order[2]
        assert ic.FILLS[0] == ic.FILLS[-1] == 0 and {0, 1, 2, 63, 64, 65, 128, 255, 256, 257, 600} <= set(ic.FILLS)
        nb, buckets = ic.one_bucket(k, kind)
        assert nb == 1 and len(buckets[0]) == 300
        nb, buckets = ic.sparse(k, kind)
        occupied = [b for b in range(nb) if buckets[b]]
        assert nb == 4096 and sum(map(len, buckets)) == 100 and occupied[0] >= 1024 and occupied[-1] < 3072 and set(occupied) <= ic.SPARSE_ELIGIBLE
        assert max(y - x for x, y in zip(occupied, occupied[1:])) >= 30
        nb, buckets = ic.empty(k, kind)
        assert nb == 64 and not any(buckets)
        for name, image in ic.load_cases(k, kind):      # every key canonical, in the bucket the oracle's hash gives, stored once
            nb, _, buckets = ri.parse(image, kb, kind)
            keys = [key for b in buckets for key, _ in b]
            assert len(set(keys)) == len(keys)
            assert all(ic.canon(key, k) == key and ic.bucket_of(key, nb) == b for b in range(nb) for key, _ in buckets[b]), name
            assert all(key[-1] & ~ic.last_byte_mask(k) == 0 for key in keys)
    target, groups, ones_bucket, ones_keys = ic._shared_keys(k)
    W = ic.words_of(k)
    assert groups["zero"] == [bytes(kb)] and set(groups) == {"zero", "last_byte"} | {"share%d" % j for j in range(1, W)} | ({"ones"} if ones_bucket == target else set())
    for j in range(1, W):
        g = groups["share%d" % j]
        assert len(g) >= 2 and len({key[:8 * j] for key in g}) == 1 and len({key[8 * j:8 * j + 8] for key in g}) == len(g)
    g = groups["last_byte"]
    assert len(g) >= 2 and len({key[:kb - 1] for key in g}) == 1 and len({key[kb - 1] for key in g}) == len(g)
    if k >= 64:
        ones = bytes([0xff] * 8) + bytes(kb - 8)
        nb, buckets = ic.shared_words(k, "weak")
        assert ones in [key for key, _ in buckets[ic.bucket_of(ones, 16)]] and len(buckets[ic.bucket_of(ones, 16)]) >= 2
    else:
        assert ones_bucket is None
    for kind in ("weak", "weak_ext"):
        for name, (na, nb_, shared) in {"cross_40_40_10": (40, 40, 10), "cross_200_100": (200, 100, 0), "cross_250_250_240": (250, 250, 240)}.items():
            a, b = (ri.parse(x, kb, kind)[2][5] for x in ic.merge_case(name, k, kind))
            assert (len(a), len(b), len({key for key, _ in a} & {key for key, _ in b})) == (na, nb_, shared)
        a, b = ic.merge_case("equal", k, kind)
        assert a == b and any(v[0] == 65535 and v[2] == 65535 for v in ri.table_of(a, kb, kind).values())
        a, b = (set(ic.stored_keys(x, k, kind)) for x in ic.merge_case("disjoint", k, kind))
        assert a and b and not a & b
        a, b = (set(ic.stored_keys(x, k, kind)) for x in ic.merge_case("half_shared", k, kind))
        assert a & b and a - b and b - a
        a, b, c = (set(ic.stored_keys(x, k, kind)) for x in ic.merge_case("chain3", k, kind))
        assert a & b & c and c - a - b
        assert ri.entry_count(ic.merge_case("b_empty", k, kind)[1], kb, kind) == 0 == ri.entry_count(ic.merge_case("a_empty", k, kind)[0], kb, kind)
        vals = list(ri.table_of(ic.image_of(ic.values(k, kind), k, kind), kb, kind).values())
        assert {v[0] for v in vals} == {1, 2, 255, 256, 65534, 65535} and {v[2] for v in vals} == {0, 65535} and all(any(v[4]) for v in vals)
        assert all(ri.f32_of_bits(v[1]) <= v[0] and ri.f32_of_bits(v[1]) * 128 == int(ri.f32_of_bits(v[1]) * 128) for v in vals)
        wide = {v[0] for v in ri.table_of(ic.image_of(ic.values(k, kind, True), k, kind), kb, kind).values()}
        assert len([c for c in wide if 512 <= c <= 1000]) >= 90 and 511 in wide and 1001 in wide
    for kind in ("sing", "sing_ext"):
        assert {v[0] for v in ri.table_of(ic.image_of(ic.values(k, kind), k, kind), kb, kind).values()} == {0, 1, 2, 128, 255}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", (13, 31, 33, 127))
def test_malformed_images_are_one_edit_away(k, kind):
    """every malformed image differs from a well-formed one, carries one of load's messages, and the list is whole"""
    cases = ic.malformed(k, kind)
    names = [name for name, _, _ in cases]
    assert set(names) >= {"len0", "len15", "len16", "nb0", "nb3", "nb2p62-len16", "nb2p62-len24", "nb2p63-len16", "nb2p63-len24", "mask", "one_byte_more",
                          "one_byte_less", "other_k", "other_kind", "offset_plus_4", "offsets_descending", "count_plus_1", "count_minus_1", "count_cut_4"}
    assert ("count_cut_entry" in names) == ((ic.kb_of(k) + ri.VBYTES[kind]) in (16, 20))
    good = {ic.image_of(ic.fills(k, kind, "sorted"), k, kind), ic.image_of(ic.one_bucket(k, kind), k, kind)}
    for name, image, message in cases:
        assert image not in good and message in (ic.TOO_SHORT, ic.BAD_HEADER, ic.BAD_SIZE, ic.BAD_OFFSETS, ic.PAST_END, ic.BAD_LENGTH), name
    assert len(dict((n, i) for n, i, _ in cases)["nb2p63-len16"]) == 16
