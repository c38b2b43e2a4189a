"""development tool: coverage normalization (kmr_normalize_reads_dev) against one round of kmr_partition_reads_dev on the same
batch: 1 M interleaved pairs x 150 bp (the bench's generator), scores and trims handed in (array form, no spectrum is built), the
FASTQ text in device memory.  Scores are whole numbers spread evenly over 1 .. 120; the target depth T is chosen so that about a
third of the pairs survive (mean of min(1, (T + 1) / max(s1, s2))), and the partition's threshold so that its one round picks
about as many reads (the matching quantile of max(s1, s2)).  The added work of the normalization is one Philox per pair and a
scan over 2 n slots instead of n reads.
The two calls alternate inside every repetition after a warm-up of each; a call's time is the host clock around it (a call ends in
a device synchronise and includes the copy of its per-read arrays to the device) and the library's HIP-event time of selection +
writer and of the writer alone (kmr_tune select_timing).  Reported per call: median, minimum, 10th - 90th percentile.
--partition-only measures the partition alone and needs nothing of the normalization, so that the same file runs in a checkout of
the commit before it; --parent-json takes what such a run printed and adds it, and the ratios against it, to the result.
Writes profiles/normalize.json (or --out) and prints it as one JSON line.
usage: tools/normalize_bench.py [pairs] [repetitions] [--partition-only] [--parent-json FILE ...] [--out FILE]"""
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmernator_amd as ka
import bench

args = sys.argv[1:]
partition_only = "--partition-only" in args
parent_json, out_path = [], os.path.join(ROOT, "profiles", "normalize.json")
pos = []
i = 0
while i < len(args):
    if args[i] == "--partition-only":
        pass
    elif args[i] == "--parent-json":
        i += 1
        parent_json.append(args[i])
    elif args[i] == "--out":
        i += 1
        out_path = args[i]
    else:
        pos.append(args[i])
    i += 1
n_pairs = int(pos[0]) if len(pos) > 0 else 1_000_000
reps = int(pos[1]) if len(pos) > 1 else 30
n = 2 * n_pairs
L, NAME = bench.READ_LEN, 11
dev = torch.device("cuda", 0)
bases, quals, offsets = bench.gen_reads(torch, n, 5 * n, 1234, 0, dev, "noisy")
# FASTQ text of the batch, made on the device: "@r%010d\n" bases "\n+\n" quals "\n"
rec = 1 + NAME + 1 + L + 3 + L + 1
text = torch.empty((n, rec), dtype=torch.uint8, device=dev)
text[:, 0] = ord("@"); text[:, 1] = ord("r")
idx = torch.arange(n, device=dev, dtype=torch.int64)
for d in range(NAME - 1):
    text[:, 2 + d] = ((idx // 10 ** (NAME - 2 - d)) % 10 + 48).to(torch.uint8)
c = 1 + NAME
text[:, c] = 10; text[:, c + 1:c + 1 + L] = bases[:n * L].view(n, L); c += 1 + L
text[:, c] = 10; text[:, c + 1] = ord("+"); text[:, c + 2] = 10; text[:, c + 3:c + 3 + L] = quals[:n * L].view(n, L); text[:, c + 3 + L] = 10
text = text.view(-1)
torch.cuda.synchronize()
del bases, quals, offsets, idx

sp = ka.KmerSpectrum(ka.default_config(bench.K, estimated_raw_kmers=1 << 20, device=0))
lib = sp.lib
r = C.c_void_p()
rc = lib.kmr_ingest_fastq_dev(sp.h, text.data_ptr(), text.numel(), 33, 1, C.byref(r))
assert rc == 0, lib.kmr_last_error(sp.h)
rng = np.random.default_rng(5)
mate = np.arange(n, dtype=np.int64) ^ 1
read1, read2 = np.arange(0, n, 2, dtype=np.int64), np.arange(1, n, 2, dtype=np.int64)
score = rng.integers(1, 121, n).astype(np.float32)
tl = rng.integers(60, L + 1, n).astype(np.uint32)          # every read passes the length
to = ((L - tl) // 2).astype(np.uint32)
wt = (tl < L).astype(np.uint8)
smax = np.maximum(score[0::2], score[1::2]).astype(np.float64)
T = min(range(1, 120), key=lambda t: abs(float(np.minimum(1.0, (t + 1) / smax).mean()) - 1.0 / 3.0))
expected_share = float(np.minimum(1.0, (T + 1) / smax).mean())
threshold = float(np.quantile(smax, 1.0 - expected_share, method="higher"))
u8, u32, i64p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
trims = [to.ctypes.data_as(u32), tl.ctypes.data_as(u32), score.ctypes.data_as(f32p), wt.ctypes.data_as(u8)]
pcfg = ka.KmrPartitionConfig()
lib.kmr_partition_config_init(C.byref(pcfg))
pcfg.select.minimum_score = threshold
KINDS = ("partition",) if partition_only else ("normalize", "partition")
if not partition_only:
    ncfg = ka.KmrNormalizeConfig()
    lib.kmr_normalize_config_init(C.byref(ncfg))
    ncfg.select.minimum_score, ncfg.target_depth, ncfg.seed, ncfg.by_pair = 1.0, T, 1, 1
sp.tune(select_timing=1)


def call(which):
    out = C.c_void_p()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if which == "normalize":
        rc = lib.kmr_normalize_reads_dev(sp.h, r, text.data_ptr(), text.numel(), read1.ctypes.data_as(i64p), read2.ctypes.data_as(i64p), n_pairs, None, None, None, *trims, None, 0, C.byref(ncfg), C.byref(out))
    else:
        rc = lib.kmr_partition_reads_dev(sp.h, r, text.data_ptr(), text.numel(), mate.ctypes.data_as(i64p), None, None, None, *trims, None, 0, C.byref(pcfg), C.byref(out))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kmr_last_error(sp.h)
    npk, nb = C.c_uint64(), C.c_uint64()
    lib.kmr_picks_info(out, C.byref(npk), C.byref(nb))
    lib.kmr_picks_free(out)
    return {"call_ms": ms, "select_ms": sp.build_info("select_ms"), "write_ms": sp.build_info("select_write_ms"), "picked": npk.value, "bytes": nb.value}


for k in KINDS:          # warm-up of every shape
    for _ in range(3):
        call(k)
runs = {k: [] for k in KINDS}
for rep in range(reps):
    for k in KINDS:
        runs[k].append(call(k))


def summary(xs):
    xs = np.array(xs)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90))}


res = {"tool": "normalize_bench", "pairs": n_pairs, "reads": n, "read_len": L, "repetitions": reps, "target_depth": T, "expected_share_of_pairs": expected_share,
       "partition_threshold": threshold}
for k in KINDS:
    assert len(set((t["picked"], t["bytes"]) for t in runs[k])) == 1, "the picks of %s changed between repetitions" % k
    res[k] = {m: summary([t[m] for t in runs[k]]) for m in ("call_ms", "select_ms", "write_ms")}
    res[k]["select_without_writer_ms"] = summary([t["select_ms"] - t["write_ms"] for t in runs[k]])
    res[k]["picked_reads"], res[k]["output_bytes"] = runs[k][0]["picked"], runs[k][0]["bytes"]
    res[k]["output_GBps_of_call"] = res[k]["output_bytes"] / res[k]["call_ms"]["median"] / 1e6
    res[k]["output_GBps_of_select"] = res[k]["output_bytes"] / res[k]["select_ms"]["median"] / 1e6
if not partition_only:
    res["ratio_same_tree"] = {m: res["normalize"][m]["median"] / res["partition"][m]["median"] for m in ("call_ms", "select_ms")}
    parents = [json.load(open(p)) for p in parent_json]
    if parents:
        res["partition_parent_commit"] = [p["partition"] for p in parents]
        for m in ("call_ms", "select_ms"):
            med = float(np.median([p["partition"][m]["median"] for p in parents]))
            res.setdefault("ratio_to_parent_commit", {})[m] = res["normalize"][m]["median"] / med
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print(json.dumps(res))
