"""Directed stored-map images for tests/test_image_cases.py (CPU: the oracle against tests/refimage.py) and
tests/test_gpu_image_edges.py (kmr_load_image, kmr_merge_image, kmr_write_image and what reads the maps they leave).  No reads and
no spectrum build: a case is a list of entries dealt into buckets by the oracle's hash (orc_hash, orc_bucket_idx -- never the
library under test), keys made canonical by orc_least_complement; quotas are filled by drawing keys and dropping those that land
in a full bucket.  Everything is drawn from seeded generators, so a case id names one image for good.

Families, each for one thing that can go wrong:
  fills         nb = 16, bucket fills FILLS: every sort path of sort_buckets_kernel (<= 64 entries: shuffle rank sort; 65..256:
                four entries per lane; > 256: heap sort) on both sides of its thresholds, empty first, middle and last buckets;
                stored sorted, reversed and shuffled
  one_bucket    nb = 1 (mask 0), 300 entries
  sparse        nb = 4096, 100 entries in 128 eligible buckets: runs of equal start[] before, between and after them
  empty         nb = 64, no entry
  shared_words  one bucket holding groups of keys that share their first 1, 2, 3 words, a group that differs in the last used byte
                only, the all-zero key A^k, and (k >= 64) T^32 A^(k-32), whose first word is all ones
  values        the ends of every value field, nonzero struct padding; values_wide adds counts over 512..1000 and beyond
  merge pairs   MERGES
  malformed     one edit of a well-formed image each, with the message it must be refused with"""
import ctypes as C
import functools
import struct

import numpy as np

import refimage as ri
from helpers import oracle_lib

KS = (13, 31, 32, 33, 64, 65, 96, 97, 127)      # kb 4 (six unused low bits), 8, 8, 9, 16, 17, 24, 25, 32: W = 1..4, last word full or partial
ORDERS = ("sorted", "reversed", "shuffled")
FILLS = (0, 1, 2, 63, 64, 65, 128, 255, 256, 257, 600, 0, 3, 66, 191, 0)      # 1951 entries, a prime: no other entry size fits by chance
MERGES = ("disjoint", "half_shared", "equal", "b_empty", "a_empty", "cross_40_40_10", "cross_200_100", "cross_250_250_240", "chain3")
SING_MERGES = ("sing_disjoint", "sing_share_one")


def kb_of(k):
    return (k + 3) // 4


def words_of(k):
    return (kb_of(k) + 7) // 8


# ------------------------------------------------------------------------------------------------------------------ keys
def canon(key, k):
    """the least complement of a packed k-mer"""
    kb = kb_of(k)
    out = (C.c_uint8 * kb)()
    oracle_lib().orc_least_complement((C.c_uint8 * kb).from_buffer_copy(key), k, out)
    return bytes(out)


def bucket_of(key, nb):
    lib = oracle_lib()
    return lib.orc_bucket_idx(lib.orc_hash(key, len(key)), nb)


def last_byte_mask(k):
    return (0xff, 0xc0, 0xf0, 0xfc)[k & 3]


def random_keys(rng, k, n):
    """n random packed k-mers (unused low bits zero), not yet canonical"""
    a = rng.integers(0, 256, size=(n, kb_of(k)), dtype=np.uint8)
    a[:, -1] &= last_byte_mask(k)
    return [r.tobytes() for r in a]


def deal(rng, k, nb, quota, seen):
    """buckets of distinct canonical keys, quota[b] of them in bucket b, none of them in `seen` (which grows)"""
    buckets = [[] for _ in range(nb)]
    need = sum(quota)
    while need:
        for key in random_keys(rng, k, 2048):
            key = canon(key, k)
            b = bucket_of(key, nb)
            if key in seen or len(buckets[b]) >= quota[b]:
                continue
            seen.add(key)
            buckets[b].append(key)
            need -= 1
            if not need:
                break
    return buckets


# ------------------------------------------------------------------------------------------------------------------ values
def dyadic_bits(x):
    """the f32 bits of a multiple of 2^-7 below 2^17: exact"""
    assert x * 128 == int(x * 128) and x < (1 << 17)
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def random_value(rng, kind, max_count=2000):
    """weightedCount a multiple of 2^-7 no greater than the count: any sum of such weights is exact in f64 in any order"""
    if ri.is_weak(kind):
        count = int(rng.integers(1, max_count + 1))
        w = int(rng.integers(0, count * 128 + 1)) / 128.0
        tallies = tuple(int(x) for x in rng.integers(0, 1 << 32, size=12, dtype=np.uint64)) if kind == "weak_ext" else ()
        return (count, dyadic_bits(w), int(rng.integers(0, 65536)), tallies, bytes(int(x) for x in rng.integers(1, 256, size=4)))
    return (int(rng.integers(0, 256)), int(rng.integers(0, 1 << 32, dtype=np.uint64)) if kind == "sing_ext" else None)


def with_values(rng, key_buckets, kind, max_count=2000):
    return [[(key, random_value(rng, kind, max_count)) for key in b] for b in key_buckets]


def ordered(rng, buckets, order):
    out = []
    for b in buckets:
        b = sorted(b, key=lambda kv: kv[0])
        if order == "reversed":
            b = b[::-1]
        elif order == "shuffled":
            b = [b[i] for i in rng.permutation(len(b))]
        out.append(b)
    return out


def _rng(*what):
    return np.random.default_rng([ord(c) for c in "/".join(str(w) for w in what)])


# ------------------------------------------------------------------------------------------------------------------ families
@functools.lru_cache(maxsize=None)
def _fills_keys(k):
    return deal(_rng("fills", k), k, 16, FILLS, set())


@functools.lru_cache(maxsize=None)
def fills(k, kind, order="shuffled"):
    """(nb, buckets): buckets[b] a list of (key, value) in stored order"""
    buckets = with_values(_rng("fills-values", k, kind), _fills_keys(k), kind)
    return 16, ordered(_rng("fills-order", k, kind), buckets, order)


@functools.lru_cache(maxsize=None)
def one_bucket(k, kind):
    rng = _rng("one_bucket", k, kind)
    return 1, ordered(rng, with_values(rng, deal(rng, k, 1, (300,), set()), kind), "shuffled")


SPARSE_ELIGIBLE = frozenset(b for b in range(1024, 3072) if b % 32 < 2)      # 128 buckets, pairs 30 apart, none in the first or last quarter


@functools.lru_cache(maxsize=None)
def sparse(k, kind):
    rng = _rng("sparse", k, kind)
    quota = [100 if b in SPARSE_ELIGIBLE else 0 for b in range(4096)]
    buckets = [[] for _ in range(4096)]
    seen = set()
    while len(seen) < 100:
        for key in random_keys(rng, k, 2048):
            key = canon(key, k)
            b = bucket_of(key, 4096)
            if quota[b] and key not in seen and len(seen) < 100:
                seen.add(key)
                buckets[b].append(key)
    return 4096, ordered(rng, with_values(rng, buckets, kind), "shuffled")


def empty(k, kind):
    return 64, [[] for _ in range(64)]


def _is_canonical(key, k):
    return canon(key, k) == key


@functools.lru_cache(maxsize=None)
def _shared_keys(k):
    """(target bucket, its keys by group name, the bucket of T^32 A^(k-32) or None, that bucket's keys)"""
    rng = _rng("shared_words", k)
    kb, W = kb_of(k), words_of(k)
    zero = bytes(kb)
    target = bucket_of(zero, 16)
    groups = {"zero": [zero]}

    def group(shared_bytes, name, want=5, tries=64):
        while True:
            head = bytes([int(rng.integers(0, 64))]) + random_keys(rng, k, 1)[0][1:shared_bytes]      # first base A: most variants are canonical
            tails = {t[shared_bytes:] for t in random_keys(rng, k, tries)}
            got = [head + t for t in sorted(tails) if bucket_of(head + t, 16) == target and _is_canonical(head + t, k)]
            if len(got) >= 2:
                groups[name] = got[:want]
                return
    for j in range(1, W):
        group(8 * j, "share%d" % j)
    group(kb - 1, "last_byte")
    ones = None
    ones_bucket, ones_keys = None, []
    if k >= 64:       # T^32 X is canonical only if X ends in A^32 (its reverse complement starts with what X ends in): no such key below k = 64
        ones = bytes([0xff] * 8) + bytes(kb - 8)
        assert _is_canonical(ones, k)
        ones_bucket = bucket_of(ones, 16)
        if ones_bucket == target:
            groups["ones"] = [ones]
        else:
            ones_keys = [ones] + deal(rng, k, 16, [5 if b == ones_bucket else 0 for b in range(16)], {ones})[ones_bucket]
    return target, groups, ones_bucket, ones_keys


@functools.lru_cache(maxsize=None)
def shared_words(k, kind):
    rng = _rng("shared_words-values", k, kind)
    target, groups, ones_bucket, ones_keys = _shared_keys(k)
    keys = [[] for _ in range(16)]
    keys[target] = sorted({key for g in groups.values() for key in g})
    if ones_bucket is not None and ones_bucket != target:
        keys[ones_bucket] = ones_keys
    # stored in descending order: a sort that looks at the first word alone and keeps ties as they stand leaves every group wrong
    return 16, ordered(rng, with_values(rng, keys, kind), "reversed")


def _edge_values(kind, wide):
    if not ri.is_weak(kind):
        return [(w, p if kind == "sing_ext" else None) for w in (0, 1, 2, 128, 255) for p in (0, 0xffffffff)]
    out = []
    counts = [1, 2, 255, 256, 65534, 65535]
    if wide:      # Histogram indices 512..1000 at zoom 1000, counts past the zoom, and both sides of HIST_LDS = 512
        counts += list(range(505, 1001, 5)) + [511, 512, 513, 999, 1000, 1001, 1024, 2047, 2048, 40000]
    for i, count in enumerate(counts):
        for dirb in (0, 65535):
            for t in (0, 0xffffffff):
                w = (count, count / 2.0, 0.0, 1 / 128.0)[(i + (dirb & 1) + (t & 1)) % 4]
                out.append((count, dyadic_bits(w), dirb, (t,) * 12 if kind == "weak_ext" else (), b"\xa5\x5a\xff\x01"))
    return out


@functools.lru_cache(maxsize=None)
def values(k, kind, wide=False):
    rng = _rng("values", k, kind, wide)
    vals = _edge_values(kind, wide)
    keys = []
    seen = set()
    while len(keys) < len(vals):
        for key in random_keys(rng, k, 256):
            key = canon(key, k)
            if key not in seen and len(keys) < len(vals):
                seen.add(key)
                keys.append(key)
    buckets = [[] for _ in range(16)]
    for key, v in zip(keys, vals):
        buckets[bucket_of(key, 16)].append((key, v))
    return 16, ordered(rng, buckets, "shuffled")


FAMILIES = {"fills": fills, "one_bucket": one_bucket, "sparse": sparse, "empty": empty, "shared_words": shared_words, "values": values}


def image_of(case, k, kind):
    nb, buckets = case
    return ri.pack(nb, buckets, kb_of(k), kind)


def load_cases(k, kind):
    """(id, image) of every well-formed image of this k and value kind"""
    out = [("fills-" + order, image_of(fills(k, kind, order), k, kind)) for order in ORDERS]
    out += [(name, image_of(FAMILIES[name](k, kind), k, kind)) for name in ("one_bucket", "sparse", "empty", "shared_words", "values")]
    return out


# ------------------------------------------------------------------------------------------------------------------ merge pairs
def _revalued(rng, entries, kind):
    return [(key, random_value(rng, kind)) for key, _ in entries]


@functools.lru_cache(maxsize=None)
def merge_case(name, k, kind):
    """the images to merge, in order (two, or three for the chain), all of nb = 16 but for "nb16_vs_32" """
    rng = _rng("merge", name, k, kind)
    kb = kb_of(k)
    seen = set()

    def draw(quota, nb=16):
        return ordered(rng, with_values(rng, deal(rng, k, nb, quota, seen), kind), "shuffled")

    def img(buckets, nb=16):
        return ri.pack(nb, buckets, kb, kind)

    small = [int(x) for x in rng.integers(0, 12, size=16)]
    small[0] = small[15] = 0
    if name in ("disjoint", "sing_disjoint"):
        return img(draw(small)), img(draw(small[::-1]))
    if name == "half_shared":
        a, extra = draw(small), draw(small)
        b = [ordered(rng, [_revalued(rng, x[:len(x) // 2], kind) + y], "shuffled")[0] for x, y in zip(a, extra)]
        return img(a), img(b)
    if name == "equal":      # B is A: every count doubles, 65535 + 65535 wraps to 65534
        a = draw(small)
        full = (65535, dyadic_bits(65535.0), 65535, (0xffffffff,) * 12 if kind == "weak_ext" else (), b"\1\2\3\4")
        b0 = next(b for b in a if b)
        b0[0] = (b0[0][0], full)
        return img(a), img(a)
    if name == "b_empty":
        return img(draw(small)), img([[] for _ in range(16)])
    if name == "a_empty":
        return img([[] for _ in range(16)]), img(draw(small))
    if name.startswith("cross_"):      # bucket 5 crosses a sort path only once the two maps stand together
        na, nb_, shared = {"cross_40_40_10": (40, 40, 10), "cross_200_100": (200, 100, 0), "cross_250_250_240": (250, 250, 240)}[name]
        qa, qb = list(small), list(small)
        qa[5], qb[5] = na, nb_ - shared
        a, b = draw(qa), draw(qb)
        b[5] = ordered(rng, [b[5] + _revalued(rng, a[5][:shared], kind)], "shuffled")[0]
        return img(a), img(b)
    if name == "chain3":
        a, extra, more = draw(small), draw(small), draw(small)
        b = [_revalued(rng, x[:len(x) // 2], kind) + y for x, y in zip(a, extra)]
        c = [_revalued(rng, x[len(x) // 3:], kind) + y[:1] + z for x, y, z in zip(a, extra, more)]
        return img(a), img(b), img(ordered(rng, c, "reversed"))
    if name == "sing_share_one":
        a, b = draw(small), draw(small)
        src = next(x for x in a if x)
        b[a.index(src)].append((src[0][0], random_value(rng, kind)))
        return img(a), img(b)
    if name == "nb16_vs_32":
        return img(draw(small)), img(draw(small + small, 32), 32)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------ malformed
TOO_SHORT = "image too short"
BAD_HEADER = "bad image header"
BAD_SIZE = "image size does not match"
BAD_OFFSETS = "not the packed store() layout"
PAST_END = "runs past the end"
BAD_LENGTH = "length mismatch"


def _put(image, at, fmt, v):
    return image[:at] + struct.pack(fmt, v) + image[at + struct.calcsize(fmt):]


def other_k(k, kind):
    """the nearest k whose `fills` image is not by chance a whole number of this k's entries long"""
    n, esz, vb = sum(FILLS), kb_of(k) + ri.VBYTES[kind], ri.VBYTES[kind]
    return next(o for o in sorted(KS, key=lambda o: abs(o - k)) if kb_of(o) != kb_of(k) and n * (kb_of(o) + vb) % esz)


def other_kind(k, kind):
    """the other value kind of the same map (else of the other map) whose `fills` image does not fit by chance either"""
    n, kb = sum(FILLS), kb_of(k)
    return next(o for o in sorted(ri.KINDS, key=lambda o: ri.is_weak(o) != ri.is_weak(kind)) if o != kind and n * (kb + ri.VBYTES[o]) % (kb + ri.VBYTES[kind]))


@functools.lru_cache(maxsize=None)
def malformed(k, kind):
    """(id, bytes, the message it must be refused with): one edit each of the sorted `fills` image of this k and kind (of the
    one_bucket image where the edit needs a last bucket that is not empty).  The fills image has nb = 16, buckets 11 and 15 empty
    and bucket 10 the fullest, so every message below follows from the order of load's checks: length >= 16; header (nb a power
    of two, mask = nb - 1, 12 nb <= len - 16); (len - 16 - 12 nb) a multiple of the entry size; then bucket by bucket the offset
    and the room for the count ("not the packed store() layout"), the room for the entries ("runs past the end"); at last the
    end ("length mismatch")"""
    kb, vb = kb_of(k), ri.VBYTES[kind]
    esz = kb + vb
    good = image_of(fills(k, kind, "sorted"), k, kind)
    one = image_of(one_bucket(k, kind), k, kind)
    offs = list(struct.unpack_from("<16Q", good, 16))
    out = [("len0", b"", TOO_SHORT), ("len15", good[:15], TOO_SHORT), ("len16", good[:16], BAD_HEADER),
           ("nb0", _put(_put(good, 0, "<Q", 0), 8, "<Q", 0xffffffffffffffff), BAD_HEADER),
           ("nb3", _put(_put(good, 0, "<Q", 3), 8, "<Q", 2), BAD_HEADER),
           # 8 (2 + nb) + 4 nb wraps to 16 for these two: the buffers end where a wrapped sum says the offsets do
           ("nb2p62-len16", struct.pack("<QQ", 1 << 62, (1 << 62) - 1), BAD_HEADER),
           ("nb2p62-len24", struct.pack("<QQQ", 1 << 62, (1 << 62) - 1, 16), BAD_HEADER),
           ("nb2p63-len16", struct.pack("<QQ", 1 << 63, (1 << 63) - 1), BAD_HEADER),
           ("nb2p63-len24", struct.pack("<QQQ", 1 << 63, (1 << 63) - 1, 16), BAD_HEADER),
           ("mask", _put(good, 8, "<Q", 16), BAD_HEADER),
           ("one_byte_more", good + b"\0", BAD_SIZE), ("one_byte_less", good[:-1], BAD_SIZE)]
    ok, okind = other_k(k, kind), other_kind(k, kind)
    out.append(("other_k", image_of(fills(ok, kind, "sorted"), ok, kind), BAD_SIZE))
    out.append(("other_kind", image_of(fills(k, okind, "sorted"), k, okind), BAD_SIZE))
    out.append(("offset_plus_4", _put(good, 16 + 8 * 7, "<Q", offs[7] + 4), BAD_OFFSETS))
    out.append(("offsets_descending", good[:16] + struct.pack("<16Q", *offs[::-1]) + good[144:], BAD_OFFSETS))
    out.append(("count_plus_1", _put(good, offs[15], "<I", 1), PAST_END))                    # the last bucket: nothing follows its count
    out.append(("count_minus_1", _put(one, 24, "<I", 299), BAD_LENGTH))                      # nb = 1: the walk ends one entry early
    assert esz != 4
    out.append(("count_cut_4", good[:-4], BAD_SIZE))                                         # the last count is gone, and the size no longer fits
    cut = cut_count_case(k, kind)
    if cut:
        out.append(cut)
    return out


def cut_count_case(k, kind):
    """the last bucket's count field cut off by the end of the buffer while the size still fits the entry size: an image whose
    last five buckets are empty, cut by esz bytes (possible where esz is a multiple of 4 no greater than 20: k = 13, 31, 32 with
    plain weak values), or None.  The walk then finds no room for a count at a bucket whose offset is still right"""
    kb, vb = kb_of(k), ri.VBYTES[kind]
    esz = kb + vb
    if esz % 4 or esz > 20:
        return None
    nb, buckets = fills(k, kind, "sorted")
    buckets = list(buckets[:11]) + [[] for _ in range(5)]
    return ("count_cut_entry", ri.pack(16, buckets, kb, kind)[:-esz], BAD_OFFSETS)


# ------------------------------------------------------------------------------------------------------------------ lookups
def stored_keys(image, k, kind):
    return [key for b in ri.parse(image, kb_of(k), kind)[2] for key, _ in b]


def absent_keys(image, k, kind, n=64):
    """n canonical keys the image does not hold: half of them land in buckets that hold entries, half in empty ones (all of them in
    the one sort there is where the image has no bucket of the other)"""
    nb, _, buckets = ri.parse(image, kb_of(k), kind)
    held = {key for b in buckets for key, _ in b}
    full = any(buckets) and not all(buckets)
    want = {True: n // 2 if full else (n if any(buckets) else 0), False: n // 2 if full else (0 if any(buckets) else n)}
    out = {True: [], False: []}
    rng = _rng("absent", k, kind, len(image))
    while len(out[True]) < want[True] or len(out[False]) < want[False]:
        for key in random_keys(rng, k, 512):
            key = canon(key, k)
            occupied = bool(buckets[bucket_of(key, nb)])
            if key not in held and len(out[occupied]) < want[occupied]:
                held.add(key)
                out[occupied].append(key)
    return out[True] + out[False]


def both_maps_singleton(k, kind):
    """a singleton image that holds the keys of the `values` weak image of this k (weight bytes 0, 1, 2, ... in turn) next to the
    `values` singleton image's own"""
    nb, buckets = values(k, kind)
    buckets = [list(b) for b in buckets]
    for i, key in enumerate(stored_keys(image_of(values(k, "weak"), k, "weak"), k, "weak")):
        buckets[bucket_of(key, nb)].append((key, (i % 256, 7 * i if kind == "sing_ext" else None)))
    return ri.pack(nb, buckets, kb_of(k), kind)
