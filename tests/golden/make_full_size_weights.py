#!/usr/bin/env python3
"""Writes tests/golden/full_size_weights.npz: the weight profile (tests/helpers.py, weight_profile) of what the serial ORACLE makes
of the full-size configurations of full_size_digests.json, so that the GPU tests can hold weightedCount per key-hash bin and per
entry, where the digest only holds its sum over the whole map.

The oracle runs exactly as in make_full_size_digests.py (its CONFIGS and its part-by-part serial builds).  For every part the
script keeps the weak map's profile, the answers of the part's maps to the read-cut keys, and the part's statistics and digests;
bins add over the parts, samples merge by the smallest key mix, and each read-cut key is answered by the one part that holds it.
The statistics and weak digest summed over the parts must equal the committed full_size_digests.json, which shows the profile
came from the same maps (that file is only read).

Per configuration <name>, the arrays <name>/<field>:
  entries, count_sum (uint32), wsum, nwsum (float64)    per bin (PROFILE_BINS, by the top 11 bits of key_mix)
  sample_keys, sample_count, sample_w (float32)          the PROFILE_SAMPLE entries of smallest key_mix, in that order
  rc_keys, rc_kind, rc_count, rc_w (float64)             the read-cut keys (helpers.read_cut_keys) and what getCount answers
c4_flat is not in the default list.  Asked for by name it is kept to the sample and the read-cut keys (its GPU test reads them through
getCount only; an 8 GB image is not read back), and each of its 16 parts takes about 9 GB of host memory, so a 64 GB machine runs
it with DIGEST_PROCS=5 or fewer.

Run time (8 cores, 8 processes): 4 minutes per C2 configuration, up to 2 per 3 M configuration, about 15 minutes for the default list.

    python tests/golden/make_full_size_weights.py [name ...]
"""
import ctypes as C
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_full_size_digests import CHUNK, CONFIGS, MIN_DEPTH, READ_LEN      # noqa: E402

WEIGHT_CONFIGS = ["small_k31_noisy", "small_k51_flat", "k51_noisy_3m", "k96_noisy_3m", "k127_noisy_3m", "sing_k51_d1_noisy",
                  "ext_k21_noisy_2m", "c2_flat", "c2_noisy"]
NO_BINS = {"c4_flat"}
BIN_FIELDS = ("entries", "count_sum", "wsum", "nwsum")
CACHE = os.environ.get("WEIGHTS_CACHE", "/tmp/kmr_weight_parts")      # not the digest script's cache: those parts hold no profile


def job_config(name, part=0):
    from helpers import default_config
    c = CONFIGS[name]
    per = READ_LEN - c["k"] + 1
    return default_config(c["k"], estimated_raw_kmers=c["reads"] * per, num_parts=c["parts"], part_idx=part, **c.get("cfg", {}))


def job_read_cut_keys(name):
    from helpers import read_cut_keys
    c = CONFIGS[name]
    return read_cut_keys(job_config(name), c["seed"], c["reads"], READ_LEN, c["genome"], c["noisy"])


def weak_entries(o):
    """keys, counts, f32 weightedCount of the oracle's weak map (OracleSpectrum.entries() without the extension tallies)"""
    n = o.stats()["weak_entries"]
    keys = np.zeros((n, o.kb), dtype=np.uint8)
    count = np.zeros(n, dtype=np.uint32)
    dirb = np.zeros(n, dtype=np.uint32)
    w = np.zeros(n, dtype=np.float32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))          # noqa: E731
    assert o.lib.orc_export_entries(o.h, p(keys, C.c_uint8), p(count, C.c_uint32), p(dirb, C.c_uint32), p(w, C.c_float), None, n) == n
    return keys, count, w


def one_part(args):
    name, part = args
    from helpers import (KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_EXT, OracleSpectrum, singleton_entries, synth_reads_8d,
                         weight_profile, weighted_answers)
    c = CONFIGS[name]
    cached = os.path.join(CACHE, "%s_%dof%d" % (name, part, c["parts"]))
    if os.path.exists(cached + ".npz"):
        with np.load(cached + ".npz") as z:
            return json.load(open(cached + ".json")), {key: z[key] for key in z.files}
    cfg = job_config(name, part)
    o = OracleSpectrum(cfg)
    t0 = time.time()
    for lo in range(0, c["reads"], CHUNK):
        m = min(CHUNK, c["reads"] - lo)
        rb = synth_reads_8d(c["seed"], lo, m, READ_LEN, c["genome"], c["noisy"], threads=1)
        o.add_reads(rb, lo, 1)
    o.finalize(c.get("min_depth", MIN_DEPTH))
    meta = [o.stats(), o.digest(KMR_MAP_WEAK), o.digest(KMR_MAP_SINGLETON)]
    keys, count, w = weak_entries(o)
    prof = weight_profile(keys, count, w)
    sk, s8 = singleton_entries(o.image(KMR_MAP_SINGLETON), o.kb, ext=cfg.value_kind == KMR_VALUE_EXT)
    o.close()
    rc = job_read_cut_keys(name)
    kind, cnt, ans = weighted_answers(rc, keys, count, w, sk, s8)
    prof.update(rc_keys=rc, rc_kind=kind, rc_count=cnt, rc_w=ans)
    sys.stderr.write("%s part %d/%d: %.0f s, %d weak entries\n" % (name, part, c["parts"], time.time() - t0, meta[1]["entries"]))
    os.makedirs(CACHE, exist_ok=True)
    np.savez(cached + ".tmp.npz", **prof)
    json.dump(meta, open(cached + ".json", "w"))
    os.replace(cached + ".tmp.npz", cached + ".npz")
    return meta, prof


def combine(name, results):
    from helpers import add_digests, add_profiles, empty_profile
    stats, weak = {}, None
    prof = None
    kind = cnt = ans = None
    for (st, dg, _), p in results:
        for key, v in st.items():
            stats[key] = stats.get(key, 0) + v
        weak = add_digests(weak, dg)
        prof = add_profiles(prof if prof is not None else empty_profile(p["sample_keys"].shape[1]), p)
        held = p["rc_kind"] != 0
        if kind is None:
            kind, cnt, ans = p["rc_kind"].copy(), p["rc_count"].copy(), p["rc_w"].copy()
        else:
            assert not np.any(held & (kind != 0)), "a read-cut key in two parts"
            kind[held], cnt[held], ans[held] = p["rc_kind"][held], p["rc_count"][held], p["rc_w"][held]
    stats["reads"] //= CONFIGS[name]["parts"]          # every pass saw every read
    prof.update(rc_keys=results[0][1]["rc_keys"], rc_kind=kind, rc_count=cnt, rc_w=ans)
    return stats, weak, prof


def main():
    from helpers import build_oracle, full_size_golden
    build_oracle()          # once, before the workers load it
    names = sys.argv[1:] or WEIGHT_CONFIGS
    path = os.path.join(HERE, "full_size_weights.npz")
    out = {}
    if os.path.exists(path):
        with np.load(path) as z:
            out = {key: z[key] for key in z.files}
    procs = int(os.environ.get("DIGEST_PROCS", "8"))
    with mp.get_context("spawn").Pool(procs) as pool:
        for name in names:
            c = CONFIGS[name]
            t0 = time.time()
            stats, weak, prof = combine(name, pool.map(one_part, [(name, p) for p in range(c["parts"])], chunksize=1))
            g = full_size_golden(name)
            assert stats == g["stats"], (name, stats, g["stats"])
            assert weak == g["weak_digest"], (name, weak, g["weak_digest"])
            assert int(prof["entries"].sum()) == stats["weak_entries"] and int(prof["count_sum"].sum()) == weak["count_sum"]
            for key in [key for key in out if key.startswith(name + "/")]:
                del out[key]
            for field, v in prof.items():
                if name in NO_BINS and field in BIN_FIELDS:
                    continue
                out[name + "/" + field] = v.astype(np.uint32) if field in ("entries", "count_sum") else v
            np.savez_compressed(path, **dict(sorted(out.items())))
            print("%s: %.0f s, %d read-cut keys (%d weak, %d singleton), npz %d bytes" % (
                name, time.time() - t0, prof["rc_kind"].size, (prof["rc_kind"] == 2).sum(), (prof["rc_kind"] == 1).sum(),
                os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    main()
