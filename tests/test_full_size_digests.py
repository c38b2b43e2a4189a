"""The plumbing the full-size parity tests stand on, checked on the CPU: SURVEY.md 8(d)'s generator is pinned to committed
values, the map digest of include/kmernator_amd.h (kmr_map_digest / orc_map_digest) is held to a numpy restatement over the
bytes of the stored map, and the oracle digests under tests/golden/full_size_digests.json (built part by part by
tests/golden/make_full_size_digests.py) are reproduced by ONE serial oracle build of the whole input at the sizes that takes
seconds -- which is what lets part digests stand for a whole spectrum at C2 / C4 size.

The same holds for the weight profiles under tests/golden/full_size_weights.npz (tests/golden/make_full_size_weights.py): weightedCount
per key-hash bin and per sampled entry, which the digest only sums over the whole map.  They are reproduced by one whole build, the
producer over image bytes the GPU tests use equals the one over the oracle's entries, and perturbed weights that the digest lets
through are caught."""
import functools
import hashlib

import numpy as np
import pytest

from helpers import (KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_EXT, PROFILE_SAMPLE, RC_ABSENT, OracleSpectrum, default_config,
                     digest_of_image, digests_agree, full_size_golden, full_size_weights, key_mix, parse_image, profile_bin,
                     singleton_entries, synth_reads_8d, weight_bin_bound, weight_bin_ratio, weight_entry_bound, weight_profile,
                     weight_profile_agrees, weight_profile_of_image, weighted_answers)

WEIGHT_REL = 1e-6          # what tests/test_zz_gpu_at_scale.py allows the sum of weightedCount over a map


def _h(a):
    return hashlib.blake2b(a.tobytes(), digest_size=8).hexdigest()


def test_generator_known_answers():
    """the first reads of job seed 1 (C2's), flat and noisy, and a slice far into a job (global read indices, not positions in the
    call): committed digests, so that neither statement of the generator can drift unnoticed"""
    rb = synth_reads_8d(1, 0, 1_000_000, 150, 5_000_000, True)
    assert rb.seq(0) == b"CGACCCGTTTTCAGTAGGTGCGAAACAAATATTACCGTCCCCGGAGGGGACTTGCGAATGGGTAGACTTGGGCGCGGTCGGCTATGGGATCCATTGTGATACGTACCTACGCTGACAGGCGCCCTCTAAGGGAAGGCGGGGTCGGTTTTG"
    assert (_h(rb.bases), _h(rb.quals)) == ("9f4046b99b531874", "bb8f8202ba5937d0")
    flat = synth_reads_8d(1, 0, 1000, 150, 5_000_000, False)
    assert np.array_equal(flat.bases, rb.bases[:150_000]) and np.all(flat.quals == ord("I"))
    # a slice is a slice of the job: reads 700..900 generated alone equal reads 700..900 of the first thousand
    part = synth_reads_8d(1, 700, 200, 150, 5_000_000, True, threads=3)
    assert np.array_equal(part.bases, rb.bases[700 * 150:900 * 150]) and np.array_equal(part.quals, rb.quals[700 * 150:900 * 150])
    # error rate 1 %, quality mix .80/.10/.05/.04/.01 with errors at Q10
    q = np.bincount(rb.quals[:3_000_000], minlength=128) / 3e6
    assert abs(q[73] - 0.80 * 0.99) < 2e-3 and abs(q[63] - 0.10 * 0.99) < 1e-3 and abs(q[53] - 0.05 * 0.99) < 1e-3
    assert abs(q[43] - (0.04 * 0.99 + 0.01)) < 1e-3 and abs(q[35] - 0.01 * 0.99) < 5e-4


@pytest.mark.parametrize("k,ext,min_depth", [(31, False, 2), (51, False, 1), (21, True, 1), (21, True, 2)])
def test_map_digest_is_what_the_header_says(k, ext, min_depth):
    """orc_map_digest against the numpy restatement over the stored map's bytes (weak and singleton maps, 12 / 60 / 1 / 5-byte values)"""
    rb = synth_reads_8d(21, 0, 3000, 150, 20_000, True)
    kw = dict(value_kind=KMR_VALUE_EXT, min_weight=0.0, min_quality_score=2) if ext else {}
    o = OracleSpectrum(default_config(k, estimated_raw_kmers=3000 * (150 - k + 1), **kw))
    o.add_reads(rb)
    o.finalize(min_depth)
    kb = (k + 3) // 4
    d = o.digest(KMR_MAP_WEAK)
    assert d["entries"] == o.stats()["weak_entries"] > 1000
    assert digests_agree(d, digest_of_image(o.image(KMR_MAP_WEAK), kb, ext=ext), rel=1e-12)
    ds = o.digest(KMR_MAP_SINGLETON)
    if min_depth == 1:
        assert ds["entries"] == o.stats()["singleton_kmers"] > 100
        assert digests_agree(ds, digest_of_image(o.image(KMR_MAP_SINGLETON), kb, ext=ext, singleton=True), rel=1e-12)
    else:
        assert ds["entries"] == 0


@functools.lru_cache(maxsize=None)
def _whole_build(name):
    """one serial oracle build of the whole input of full_size_digests.json[name] (no parts)"""
    c = full_size_golden(name)["config"]
    rb = synth_reads_8d(c["seed"], 0, c["reads"], c["read_len"], c["genome"], c["noisy"])
    o = OracleSpectrum(default_config(c["k"], estimated_raw_kmers=c["reads"] * (c["read_len"] - c["k"] + 1), **c.get("cfg", {})))
    o.add_reads(rb)
    o.finalize(c["min_depth"])
    return o


@pytest.mark.parametrize("name", ["small_k31_noisy", "small_k51_flat"])
def test_part_digests_add_up_to_the_whole_build(name):
    """the committed digest (sum of the parts' digests) == the digest of one serial oracle build of the whole input, statistics
    included: exact, weightedCount too (each k-mer meets the same weights in the same order in its part as in the whole)"""
    g = full_size_golden(name)
    o = _whole_build(name)
    assert o.stats() == g["stats"]
    assert digests_agree(o.digest(KMR_MAP_WEAK), g["weak_digest"], rel=1e-12)


def test_oracle_merge_add_against_a_joint_build():
    """orc_merge_add (KmerMapByKmerArrayPair::mergeAdd, src/Kmer.h:3209-3261) of the weak maps of two spectra built WITHOUT a singleton
    map (so that no first sighting is set aside) == the weak map of one build over both read sets: keys, counts and direction
    biases exactly, weightedCount up to the float additions' order -- the self-consistency the GPU test of kmr_merge_image leans on"""
    from helpers import synth_reads
    a = synth_reads(1500, read_len=120, genome_len=12000, seed=5, quality="noisy", n_rate=0.002)
    b = synth_reads(1500, read_len=120, genome_len=12000, seed=5, quality="noisy", n_rate=0.002)
    b.bases[:] = np.roll(b.bases.reshape(1500, 120), 7, axis=0).reshape(-1)          # the same genome, the reads in another order ...
    b.quals[:] = np.roll(b.quals.reshape(1500, 120), 311, axis=0).reshape(-1)        # ... under other qualities
    cfg = default_config(27, num_buckets_weak=256, num_buckets_singleton=256, separate_singletons=0)
    oa, ob, oj = OracleSpectrum(cfg), OracleSpectrum(cfg), OracleSpectrum(cfg)
    oa.add_reads(a); ob.add_reads(b)
    oj.add_reads(a); oj.add_reads(b, first_idx=1500)
    for o in (oa, ob, oj):
        o.finalize(1)
    oa.merge_add(ob)
    ka_, ca, da, wa, _ = oa.entries()
    kj, cj, dj, wj, _ = oj.entries()
    assert np.array_equal(ka_, kj) and np.array_equal(ca, cj) and np.array_equal(da, dj)
    assert np.all(np.abs(wa.astype(np.float64) - wj) <= 1e-5 * cj)
    assert ob.stats()["weak_entries"] == 0 or ob.entries()[0].shape[0] == 0          # the source map is emptied (src.clear(), :3259)


@pytest.mark.parametrize("name", ["small_k31_noisy", "small_k51_flat"])
def test_part_weight_profiles_add_up_to_the_whole_build(name):
    """the committed weight profile (bins added over the parts, samples merged, read-cut keys answered by the part holding them) ==
    the profile of one serial build of the whole input: integers, sample keys and sample weights exactly (a part adds the same
    weights in the same order), the bins' weight sums within 1e-12 (the parts' partial sums are added in another order)"""
    want = full_size_weights(name)
    assert want is not None
    o = _whole_build(name)
    keys, count, _, w, _ = o.entries()
    got = weight_profile(keys, count, w)
    for field in ("entries", "count_sum"):
        assert np.array_equal(got[field], want[field].astype(np.int64)), field
    assert int(want["entries"].sum()) == o.stats()["weak_entries"]
    for field in ("wsum", "nwsum"):
        assert np.all(np.abs(got[field] - want[field]) <= 1e-12 * np.abs(want[field])), field
    assert want["sample_keys"].shape == (PROFILE_SAMPLE, o.kb)
    assert np.all(np.diff(key_mix(want["sample_keys"]).astype(np.float64)) > 0)          # in key_mix order, no repeats
    assert np.array_equal(got["sample_keys"], want["sample_keys"])
    assert np.array_equal(got["sample_count"], want["sample_count"])
    assert np.array_equal(got["sample_w"].view(np.uint32), want["sample_w"].view(np.uint32))
    # the read-cut keys: the whole build's maps give the committed answers, bit for bit
    sk, s8 = singleton_entries(o.image(KMR_MAP_SINGLETON), o.kb)
    kind, cnt, ans = weighted_answers(want["rc_keys"], keys, count, w, sk, s8)
    assert np.array_equal(kind, want["rc_kind"]) and np.array_equal(cnt, want["rc_count"])
    assert np.array_equal(ans.view(np.uint64), want["rc_w"].view(np.uint64))
    assert np.array_equal(cnt, o.lookup(want["rc_keys"]))
    assert (want["rc_kind"] == RC_ABSENT).any() and (want["rc_kind"] != RC_ABSENT).any()


@pytest.mark.parametrize("k,ext", [(31, False), (21, True)])
def test_weight_profile_of_image_bytes_equals_the_entries(k, ext):
    """weight_profile_of_image (what the GPU tests run over a product image, a run of buckets at a time) == weight_profile over
    OracleSpectrum.entries() of the same map, with 12- and 60-byte values and pieces of 7 buckets or all of them"""
    rb = synth_reads_8d(21, 0, 6000, 150, 40_000, True)
    kw = dict(value_kind=KMR_VALUE_EXT, min_weight=0.0, min_quality_score=2) if ext else {}
    o = OracleSpectrum(default_config(k, estimated_raw_kmers=6000 * (150 - k + 1), **kw))
    o.add_reads(rb)
    o.finalize(2)
    keys, count, _, w, _ = o.entries()
    assert keys.shape[0] > PROFILE_SAMPLE
    want = weight_profile(keys, count, w)
    img = o.image(KMR_MAP_WEAK)
    for piece in (7, 1 << 16):
        got = weight_profile_of_image(img, o.kb, ext=ext, buckets_per_piece=piece)
        for field in ("entries", "count_sum"):
            assert np.array_equal(got[field], want[field]), field
        for field in ("wsum", "nwsum"):
            assert np.all(np.abs(got[field] - want[field]) <= 1e-12 * np.abs(want[field])), field
        assert np.array_equal(got["sample_keys"], want["sample_keys"]) and np.array_equal(got["sample_count"], want["sample_count"])
        assert np.array_equal(got["sample_w"].view(np.uint32), want["sample_w"].view(np.uint32))
        assert weight_profile_agrees(got, want, build_mode=0)


def _image_entries(img, kb):
    """(keys [n, kb], counts, f32 weight views INTO img) of a stored weak map: writing a weight writes the image"""
    _, _, buckets = parse_image(img, kb, 12)
    keys = np.concatenate([b[0] for b in buckets])
    counts = np.concatenate([np.ascontiguousarray(b[1][:, 0:2]).view(np.uint16).reshape(-1) for b in buckets])
    wviews = [b[1][:, 4:8] for b in buckets]
    return keys, counts, wviews


def _set_weight(wviews, i, value):
    for v in wviews:
        if i < v.shape[0]:
            v[i] = np.frombuffer(np.float32(value).tobytes(), np.uint8)
            return
        i -= v.shape[0]


def test_weight_profile_catches_what_the_digest_lets_through():
    """the gap and its closure on the CPU: the oracle's own image of small_k31_noisy, perturbed in two ways the reference would call
    wrong -- two entries' weights swapped (each credited to the other key, counts untouched), one sampled entry's weight off by one
    first-sighting step (1/254) -- still passes the whole-map digest check at the GPU tests' WEIGHT_REL, and fails the profile
    check even at its loosest bound (build modes 1 and 2)"""
    name = "small_k31_noisy"
    g, want = full_size_golden(name), full_size_weights(name)
    o = _whole_build(name)
    kb = o.kb
    clean = o.image(KMR_MAP_WEAK)
    assert digests_agree(digest_of_image(clean, kb), g["weak_digest"], WEIGHT_REL)
    assert weight_profile_agrees(weight_profile_of_image(clean, kb), want)

    keys, counts, _ = _image_entries(clean, kb)
    w = np.concatenate([np.ascontiguousarray(v).view(np.float32).reshape(-1) for v in _image_entries(clean, kb)[2]])
    x = key_mix(keys)
    b = profile_bin(x)
    bound = weight_bin_bound(want)
    sampled = np.isin(x, key_mix(want["sample_keys"]))

    # 1. swap: two entries outside the sample, the same count, other bins, weights further apart than either bin's bound
    cand = np.flatnonzero(~sampled & (counts == 12))
    i = int(cand[0])
    far = cand[(b[cand] != b[i]) & (np.abs(w[cand] - w[i]) > 2 * max(bound[b[i]], bound[b[cand]].max()))]
    assert far.size
    j = int(far[0])
    img = clean.copy()
    views = _image_entries(img, kb)[2]
    _set_weight(views, i, w[j])
    _set_weight(views, j, w[i])
    assert digests_agree(digest_of_image(img, kb), g["weak_digest"], WEIGHT_REL)
    got = weight_profile_of_image(img, kb)
    assert np.array_equal(got["sample_w"], want["sample_w"])          # the sample does not see it ...
    assert weight_bin_ratio(got, want) > 1.0                           # ... the bins do
    assert not weight_profile_agrees(got, want)

    # 2. one sampled entry's weight shifted by 1/254 (a first sighting quantised from the wrong sighting)
    s = int(np.flatnonzero(sampled)[0])
    assert weight_entry_bound(counts[s], w[s], 1) < 1.0 / 254
    img = clean.copy()
    _set_weight(_image_entries(img, kb)[2], s, w[s] + np.float32(1.0 / 254))
    assert digests_agree(digest_of_image(img, kb), g["weak_digest"], WEIGHT_REL)
    assert not weight_profile_agrees(weight_profile_of_image(img, kb), want)
