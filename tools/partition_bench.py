"""development tool: selectReads' last stage on the C2-shaped synthetic batch (1 M reads x 150 bp, the bench's generator), the scores and
trims handed in (array form, so no spectrum is built), scores spread evenly over 0 .. 40 so that every round of 16 / 8 / 4 / 2 takes
reads.  Three calls on the same arrays, the FASTQ text in device memory:
 (a) kmr_select_reads_dev at min depth 2: the plain entry point's timing.  It runs the kernels of (b) since the plain branch (per-read
     count, two scans over the reads, compaction) was retired, and keeps no per-read segments;
 (b) kmr_partition_reads_dev with partition_by_depth 0: one round, the same bytes (checked);
 (c) kmr_partition_reads_dev with partition_by_depth 16 and remainder_trim 25: five rounds.
The three alternate inside every repetition after a warm-up of each; a call's time is the host clock around it (a call ends in a
device synchronise and includes the copy of its per-read arrays to the device, the same arrays for all three), and the library's
HIP-event time of selection + writer and of the writer alone (kmr_tune select_timing).  Reported per call: median, minimum and the
10th - 90th percentile spread.  Writes profiles/partition_bench.json and prints it as one JSON line.
usage: tools/partition_bench.py [reads] [repetitions]"""
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
n -= n & 1
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
score = rng.integers(0, 41, n).astype(np.float32)
tl = rng.integers(20, L + 1, n).astype(np.uint32)
to = ((L - tl) // 2).astype(np.uint32)
wt = (tl < L).astype(np.uint8)
u8, u32, i64p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
head = [sp.h, r, text.data_ptr(), text.numel(), mate.ctypes.data_as(i64p), None, None, None, to.ctypes.data_as(u32), tl.ctypes.data_as(u32), score.ctypes.data_as(f32p), wt.ctypes.data_as(u8)]
scfg = ka.KmrSelectConfig()
lib.kmr_select_config_init(C.byref(scfg))


def partition_config(pbd, rem):
    p = ka.KmrPartitionConfig()
    lib.kmr_partition_config_init(C.byref(p))
    p.partition_by_depth, p.remainder_trim = pbd, rem
    return p


one, five = partition_config(0, -1.0), partition_config(16, 25.0)
sp.tune(select_timing=1)


def call(which):
    out = C.c_void_p()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if which == "select":
        rc = lib.kmr_select_reads_dev(*head, C.byref(scfg), C.byref(out))
    else:
        rc = lib.kmr_partition_reads_dev(*head, None, 0, C.byref(one if which == "one_round" else five), C.byref(out))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kmr_last_error(sp.h)
    return out, {"call_ms": ms, "select_ms": sp.build_info("select_ms"), "write_ms": sp.build_info("select_write_ms")}


def text_of(out):
    npk, nb = C.c_uint64(), C.c_uint64()
    lib.kmr_picks_info(out, C.byref(npk), C.byref(nb))
    buf = np.zeros(max(1, nb.value), dtype=np.uint8)
    assert lib.kmr_picks_copy(out, buf.ctypes.data_as(C.c_void_p), nb.value, None) == 0
    return npk.value, buf[:nb.value]


KINDS = ("select", "one_round", "five_rounds")
sizes, texts = {}, {}
for k in KINDS:          # warm-up of every shape, and the outputs
    for _ in range(3):
        out, _t = call(k)
        sizes[k], texts[k] = text_of(out)
        lib.kmr_picks_free(out)
same = bool(sizes["select"] == sizes["one_round"] and np.array_equal(texts["select"], texts["one_round"]))
bytes_out = {k: int(texts[k].size) for k in KINDS}
del texts
runs = {k: [] for k in KINDS}
for rep in range(reps):
    for k in KINDS:
        out, t = call(k)
        lib.kmr_picks_free(out)
        runs[k].append(t)


def summary(xs):
    xs = np.array(xs)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90))}


res = {"tool": "partition_bench", "reads": n, "read_len": L, "repetitions": reps, "one_round_same_bytes_as_select": same,
       "picked": sizes, "output_bytes": bytes_out}
for k in KINDS:
    res[k] = {m: summary([t[m] for t in runs[k]]) for m in ("call_ms", "select_ms", "write_ms")}
    res[k]["select_without_writer_ms"] = summary([t["select_ms"] - t["write_ms"] for t in runs[k]])
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "partition_bench.json"), "w"), indent=1)
print(json.dumps(res))
assert same, "one round of the partition and kmr_select_reads disagree"
