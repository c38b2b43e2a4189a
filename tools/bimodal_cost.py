"""development tool: what the bimodal pass (ReadSelector --bimodal-sigmas, bimodal_trim_kernel) adds to scoreAndTrimReads of a
C2-size batch (10 M x 150 bp, k = 31, the bench's generator) on a device-resident read batch.  One handle, one process: after a
warm-up of every setting, `rounds` rounds that score the batch once under each of the settings off (-1), 2.5 and 0, so that drift
of the machine falls on all three alike.  A call is timed by the host clock around kmr_score_read_batch, which ends in a wait for
the stream.  Per setting: every round's time, the median, the spread (max - min), the share of reads cut and a checksum of the
results; one JSON document (profiles/bimodal.json).
A library without kmr_set_bimodal_sigmas (the commit before the pass) is timed with the off setting alone: --tree names the
checkout (built) whose kmernator_amd package is loaded in place of this one's.
usage: tools/bimodal_cost.py [--reads N] [--rounds R] [--tree DIR] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bimodal.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np
import torch
import kmernator_amd as ka
import bench

n = args.reads
dev = torch.device("cuda", 0)
bases, quals, offsets = bench.gen_reads(torch, n, 5 * n, 1234, 0, dev, "flat")
total = n * bench.READ_LEN
kmers = n * (bench.READ_LEN - bench.K + 1)
sp = ka.KmerSpectrum(ka.default_config(bench.K, estimated_raw_kmers=kmers, device=0))
sp.buildKmerSpectrumDevice(bases.data_ptr(), quals.data_ptr(), offsets.data_ptr(), n, total)
sp.finalize(2)
lib = sp.lib
has_pass = hasattr(lib, "kmr_set_bimodal_sigmas")
hb, hq, ho = bases[:total].cpu().numpy(), quals[:total].cpu().numpy(), offsets.cpu().numpy().astype(np.uint64)
r = C.c_void_p()
lib.kmr_reads_from_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_void_p)]
rc = lib.kmr_reads_from_host(sp.h, hb.ctypes.data_as(C.c_void_p), hq.ctypes.data_as(C.c_void_p), ho.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(r))
assert rc == 0, lib.kmr_last_error(sp.h)
to = np.zeros(n, np.uint32); tl = np.zeros(n, np.uint32); sc = np.zeros(n, np.float32); wt = np.zeros(n, np.uint8); words = np.zeros(n, np.uint64)
settings = [-1.0, 2.5, 0.0] if has_pass else [-1.0]
res = {s: dict(ms=[]) for s in settings}


def score(sigmas):
    if has_pass:
        rc = lib.kmr_set_bimodal_sigmas(sp.h, C.c_double(sigmas))
        assert rc == 0, lib.kmr_last_error(sp.h)
    torch.cuda.synchronize(); t0 = time.time()
    rc = lib.kmr_score_read_batch(sp.h, r, 2.0, 1, to.ctypes.data_as(C.POINTER(C.c_uint32)), tl.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_uint8)))
    dt = time.time() - t0
    assert rc == 0, lib.kmr_last_error(sp.h)
    return dt * 1e3


for rnd in range(-1, args.rounds):          # round -1 is the warm-up
    for s in settings:
        ms = score(s)
        if rnd < 0:
            cut = 0
            if has_pass:
                rc = lib.kmr_bimodal_copy(sp.h, words.ctypes.data_as(C.POINTER(C.c_uint64)), n)
                assert rc == 0, lib.kmr_last_error(sp.h)
                cut = int((words != 0).sum())
            res[s].update(reads_cut=cut, share_cut=cut / n, trimmed=int(wt.sum()), checksum=int(sc.astype(np.float64).sum()) + int(tl.astype(np.uint64).sum()))
        else:
            res[s]["ms"].append(round(ms, 3))
        print("round %d sigmas %s: %.1f ms" % (rnd, s, ms), flush=True)
doc = dict(tool="tools/bimodal_cost.py", library="this tree's" if os.path.abspath(args.tree) == ROOT else "another tree's", has_bimodal_pass=has_pass, reads=n, read_len=bench.READ_LEN, k=bench.K,
           kmers=kmers, rounds=args.rounds, score_path=sp.build_info("score_path"), settings={})
for s in settings:
    ms = res[s]["ms"]
    doc["settings"]["off" if s < 0 else str(s)] = dict(res[s], median_ms=round(float(np.median(ms)), 3), min_ms=min(ms), max_ms=max(ms), spread_ms=round(max(ms) - min(ms), 3))
print(json.dumps(doc), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
