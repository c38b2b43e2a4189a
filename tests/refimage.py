"""The stored-map format and the map merge, restated plainly over bytes, lists and ints: what kmr_write_image, kmr_load_image and
kmr_merge_image are held to (tests/test_gpu_image_edges.py) and what the oracle is held to (tests/test_image_cases.py).  Nothing
here comes from kmernator_amd or from the oracle.

Written from the reference:
  KmerMapByKmerArrayPair::store      src/Kmer.h:3143-3159     {u64 numBuckets, u64 mask, u64 offset[numBuckets]}, then per bucket
                                                              {u32 size; size keys; size values} (KmerArrayPair::store :960-969)
  KmerMapByKmerArrayPair::resort     src/Kmer.h:3079-3088     every bucket sorted by key, memcmp order (Kmer::compare :311-313)
  KmerMapByKmerArrayPair::mergeAdd   src/Kmer.h:3209-3261     same bucket count or refused (:3210); per bucket the sorted union, a key
                                                              both hold keeps a's value with b's added
  TrackingData::add and kin          src/KmerTrackingData.h:489-493, 538-542, 1059-1064   += on the u16 count and directionBias (they
                                                              wrap), on the f32 weightedCount, on the twelve u32 tallies (they wrap)
  DataPointers::getCount             src/KmerSpectrum.h:642-695   weak entry first, then the singleton's, then 0
  TrackingDataSingleton              src/KmerTrackingData.h:651-659   count = _weight ? 1 : 0, weight = (_weight - 1) / 254
  Histogram::getIdx/addRecord/set    src/KmerSpectrum.h:936-938, 964-974, 1036-1056

A value kind is one of KINDS.  A weak value is (count, weighted_bits, direction_bias, tallies, padding): u16, the bits of the f32
weightedCount, u16, a tuple of twelve u32 (empty without extensions) and the four bytes of struct padding (two after count, two
after directionBias) that the reference's memcpy of the struct carries along.  A singleton value is (weight_byte, packet): the
packet is a u32, None without extensions.  A parsed image is (nb, mask, buckets): buckets[b] a list of (key_bytes, value) in
stored order.

`wrong` names a deliberately wrong variant of one rule (WRONG): tests/test_image_cases.py shows that each of them changes the
result of at least one family of tests/imagecases.py, so no family can pass without its rule."""
import math
import struct

import numpy as np

KINDS = ("weak", "weak_ext", "sing", "sing_ext")
VBYTES = {"weak": 12, "weak_ext": 60, "sing": 1, "sing_ext": 5}
WRONG = ("first_word_only", "saturating_count", "padding_kept", "bucket_search", "clamp_511")


def is_weak(kind):
    return kind.startswith("weak")


# ------------------------------------------------------------------------------------------------------------------ values
def pack_value(v, kind):
    if is_weak(kind):
        count, wbits, dirb, tallies, pad = v
        assert len(pad) == 4 and len(tallies) == (12 if kind == "weak_ext" else 0)
        return struct.pack("<H2sIH2s", count, pad[:2], wbits, dirb, pad[2:]) + struct.pack("<%dI" % len(tallies), *tallies)
    w, pkt = v
    return bytes([w]) + (struct.pack("<I", pkt) if kind == "sing_ext" else b"")


def parse_value(b, kind):
    if is_weak(kind):
        count, p0, wbits, dirb, p1 = struct.unpack_from("<H2sIH2s", b, 0)
        return (count, wbits, dirb, struct.unpack_from("<12I", b, 12) if kind == "weak_ext" else (), p0 + p1)
    return (b[0], struct.unpack_from("<I", b, 1)[0] if kind == "sing_ext" else None)


# ------------------------------------------------------------------------------------------------------------------ store / restore
def pack(nb, buckets, kb, kind, mask=None):
    """store(): the image of nb buckets, every bucket in the order given"""
    assert len(buckets) == nb
    head, body = [struct.pack("<QQ", nb, nb - 1 if mask is None else mask)], []
    off = 8 * (2 + nb)
    for b in buckets:
        head.append(struct.pack("<Q", off))
        part = struct.pack("<I", len(b)) + b"".join(k for k, _ in b) + b"".join(pack_value(v, kind) for _, v in b)
        assert all(len(k) == kb for k, _ in b)
        body.append(part)
        off += len(part)
    return b"".join(head + body)


def parse(image, kb, kind):
    """the inverse of pack: (nb, mask, buckets); follows the stored offsets as restore() does"""
    image = bytes(image)
    nb, mask = struct.unpack_from("<QQ", image, 0)
    vb = VBYTES[kind]
    buckets = []
    for b in range(nb):
        off = struct.unpack_from("<Q", image, 16 + 8 * b)[0]
        n = struct.unpack_from("<I", image, off)[0]
        ko, vo = off + 4, off + 4 + n * kb
        buckets.append([(image[ko + i * kb:ko + (i + 1) * kb], parse_value(image[vo + i * vb:vo + (i + 1) * vb], kind)) for i in range(n)])
    assert not buckets or vo + n * vb == len(image)
    return nb, mask, buckets


def entry_count(image, kb, kind):
    return sum(len(b) for b in parse(image, kb, kind)[2])


def key_order(kb, wrong=None):
    """the sort key of a stored key: its bytes (memcmp order)"""
    if wrong == "first_word_only":
        return lambda kv: kv[0][:8]
    return lambda kv: kv[0]


def zero_padding(v, kind, wrong=None):
    if is_weak(kind) and wrong != "padding_kept":
        return v[:4] + (b"\0\0\0\0",)
    return v


def canonical(image, kb, kind, wrong=None):
    """what a map that restored this image stores again: every bucket sorted by key (resort; Python's sort is stable, as the
    device's rank sort is, which only matters to the wrong variant), a weak value's struct padding zero"""
    nb, mask, buckets = parse(image, kb, kind)
    out = [[(k, zero_padding(v, kind, wrong)) for k, v in sorted(b, key=key_order(kb, wrong))] for b in buckets]
    return pack(nb, out, kb, kind, mask)


# ------------------------------------------------------------------------------------------------------------------ flat form
def bucket_of_entry(start, e, wrong=None):
    """the bucket that holds flat entry e, start[] being the exclusive scan of the bucket sizes (nb + 1 values): the last b < nb
    with start[b] <= e -- empty buckets share their start with the next bucket that is not, and must not be picked"""
    nb = len(start) - 1
    if wrong == "bucket_search":        # of the buckets that share the start, the first: right only where none of them is empty
        return start.index(max(s for s in start[:nb] if s <= e))
    return max(b for b in range(nb) if start[b] <= e)


def flatten(parsed):
    """(start, entries): the device's view of a map"""
    nb, _, buckets = parsed
    start = [0]
    for b in buckets:
        start.append(start[-1] + len(b))
    return start, [kv for b in buckets for kv in b]


def unflatten(nb, start, entries, wrong=None):
    buckets = [[] for _ in range(nb)]
    for e, kv in enumerate(entries):
        buckets[bucket_of_entry(start, e, wrong)].append(kv)
    return buckets


# ------------------------------------------------------------------------------------------------------------------ mergeAdd
def add_values(a, b, wrong=None):
    """a.add(b) of two weak values: a's padding stays"""
    count = a[0] + b[0]
    count = min(count, 65535) if wrong == "saturating_count" else count & 0xffff
    fa, fb = np.array([a[1], b[1]], dtype=np.uint32).view(np.float32)
    wbits = int(np.array([np.float32(fa) + np.float32(fb)], dtype=np.float32).view(np.uint32)[0])
    return (count, wbits, (a[2] + b[2]) & 0xffff, tuple((x + y) & 0xffffffff for x, y in zip(a[3], b[3])), a[4])


class Refused(Exception):
    """the merge the reference refuses; str() holds the word the device's message must contain"""


def merge_add(a, b, kb, kind, wrong=None):
    """mergeAdd(a, b): the image of the merged map.  Maps of differing bucket counts are refused (src/Kmer.h:3210); so are singleton
    maps that share a key (they would have to be promoted into the weak map: mergePromote, src/Kmer.h:2675-2677, refuses)"""
    na, ma, ba = parse(a, kb, kind)
    nb_, _, bb = parse(b, kb, kind)
    if na != nb_:
        raise Refused("differing")
    out = []
    for x, y in zip(ba, bb):
        d = dict(x)
        assert len(d) == len(x) and len(dict(y)) == len(y), "a key stored twice in one image is not decided here"
        for k, v in y:
            if k in d:
                if not is_weak(kind):
                    raise Refused("share")
                d[k] = add_values(d[k], v, wrong)
            else:
                d[k] = v
        out.append(sorted(d.items(), key=key_order(kb, wrong)))
    return pack(na, out, kb, kind, ma)


# ------------------------------------------------------------------------------------------------------------------ getCount
def f32_of_bits(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def sing_weight(w):
    return (w - 1) / 254.0 if w else 0.0


def table_of(image, kb, kind):
    """key -> value of a stored map (None: no map)"""
    if image is None:
        return {}
    return {k: v for b in parse(image, kb, kind)[2] for k, v in b}


def lookup(weak, sing, key):
    """getCount(key) and getCount(key, useWeights=True) against table_of() a weak and a singleton map: (count, weighted)"""
    if key in weak:
        return weak[key][0], f32_of_bits(weak[key][1])
    if key in sing:
        w = sing[key][0]
        return (1 if w else 0), sing_weight(w)
    return 0, 0.0


# ------------------------------------------------------------------------------------------------------------------ histograms
def records(weak, sing):
    """(count, weight) of every entry, the weak map's first (Histogram::set)"""
    return [(v[0], f32_of_bits(v[1])) for v in weak.values()] + [((1 if v[0] else 0), sing_weight(v[0])) for v in sing.values()]


def histogram_index(count, zoom_max, log_base, wrong=None):
    """getIdx: the count itself up to zoom_max, logarithmic steps above"""
    log_factor = math.log(log_base)
    skip = int(math.log(zoom_max + 1.0) / log_factor - 1.0)
    idx = count if count <= zoom_max else int(math.log(float(count)) / log_factor - skip + zoom_max)
    return min(idx, 511) if wrong == "clamp_511" else idx


def histogram_terms(weak, sing, zoom_max, log_base, wrong=None):
    """index -> the (count, weight) records that addRecord puts there, in set()'s order; records of count 0 are not added"""
    terms = {}
    for count, weight in records(weak, sing):
        if count:
            terms.setdefault(histogram_index(count, zoom_max, log_base, wrong), []).append((count, weight))
    return terms


def histogram(weak, sing, zoom_max, log_base, wrong=None):
    """Histogram(zoom_max, log_base).set(): (visits, visitedCount, visitedWeight), (1 << 16) + 2 + zoom_max buckets each; the
    weights added in set()'s order"""
    n = (1 << 16) + 2 + zoom_max
    visits, vcount, vweight = [0] * n, [0] * n, [0.0] * n
    for idx, recs in histogram_terms(weak, sing, zoom_max, log_base, wrong).items():
        visits[idx] = len(recs)
        vcount[idx] = sum(c for c, _ in recs)
        for _, w in recs:
            vweight[idx] += w
    return visits, vcount, vweight


def count_histogram(weak, n_bins):
    """the plain histogram of the weak map's counts, the last bin taking every larger count: (entries, weights)"""
    c, w = [0] * n_bins, [0.0] * n_bins
    for v in weak.values():
        i = min(v[0], n_bins - 1)
        c[i] += 1
        w[i] += f32_of_bits(v[1])
    return c, w
