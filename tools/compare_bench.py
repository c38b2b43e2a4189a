"""development tool: CompareSpectrums on C2's shape (10 M x 150 bp made on the device, k = 31, set 2 the spectrum of the same reads,
min-depth 1 so that it is the reference's solid map).  HIP events on the handle's stream, one warm-up, then the median of the
repetitions with every value shown:
  compare_reads        kmr_compare_reads_dev of the whole batch with the default LDS bound (one wavefront per read)
  compare_reads_sorted the same over the first 1 M reads with kmr_tune compare_lds_kmers 0 (every read through the sorted path)
  compare_reads_lds_1m the first 1 M reads with the default bound, for the per-read comparison of the two paths
  score_read_batch     kmr_score_read_batch of the whole batch: existing code, one extraction plus one lookup per k-mer
  compare_spectrums    kmr_compare_spectrums of two C2 spectra (the second from the next 10 M reads of the same genome)
The records of the 1 M slice must be the same by both paths.  Prints one JSON line and writes it to out.json (default
profiles/compare_bench.json).
usage: tools/compare_bench.py [reads] [repetitions] [out.json]"""
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmernator_amd as ka

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10_000_000
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "compare_bench.json")
L, K = 150, 31
n_slice = min(n, 1_000_000)
dev = torch.device("cuda", 0)
genome = 5 * n


def spectrum_of(first_read):
    b, q, o = ka.synth_reads_device(torch, 1, first_read, n, L, genome, False, dev)
    sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=n * (L - K + 1), device=0))
    sp.buildKmerSpectrumDevice(b.data_ptr(), q.data_ptr(), o.data_ptr(), n, n * L)
    sp.finalize(1)
    return sp, (b, q, o)


def batch(sp, arrays, m):
    b, q, o = arrays
    return ka.ReadSet.from_arrays(sp, b[:m * L].cpu().numpy(), q[:m * L].cpu().numpy(), o[:m + 1].cpu().numpy().astype(np.uint64))


sp, arrays = spectrum_of(0)
stream = torch.cuda.ExternalStream(sp.stream(), device=dev)
rs, rs1 = batch(sp, arrays, n), batch(sp, arrays, n_slice)
out = torch.zeros(n * 8, dtype=torch.int64, device=dev)
torch.cuda.synchronize()


def timed(fn):
    ms = []
    for rep in range(reps + 1):          # the first run warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return ms


def compare_dev(reads):
    sp._call("compare_reads_dev", sp.h, reads.r, C.c_void_p(out.data_ptr()))


def records(m):
    return out[:m * 8].cpu().numpy().view(np.uint64).reshape(m, 8)


res = {"tool": "compare_bench", "reads": n, "read_len": L, "k": K, "repetitions": reps, "slice_reads": n_slice, "all": {}}
res["all"]["compare_reads"] = timed(lambda: compare_dev(rs))
whole = records(n_slice).copy()
res["all"]["compare_reads_lds_1m"] = timed(lambda: compare_dev(rs1))
lds = records(n_slice).copy()
sp.tune(compare_lds_kmers=0)
res["all"]["compare_reads_sorted"] = timed(lambda: compare_dev(rs1))
srt = records(n_slice).copy()
sp.tune(compare_lds_kmers=-1)
res["all"]["score_read_batch"] = timed(lambda: sp.scoreAndTrimReadSet(rs, 2.0))
res["score_path"] = sp.build_info("score_path")
sp2, _ = spectrum_of(n)
counts = {}
res["all"]["compare_spectrums"] = timed(lambda: counts.update(sp2.countCommonKmers(sp)))
for name, ms in res["all"].items():
    res[name + "_ms"] = float(np.median(ms))
res["lds_ns_per_read"] = res["compare_reads_lds_1m_ms"] * 1e6 / n_slice
res["sorted_ns_per_read"] = res["compare_reads_sorted_ms"] * 1e6 / n_slice
res["whole_batch_ns_per_read"] = res["compare_reads_ms"] * 1e6 / n
res["paths_agree"] = bool(np.array_equal(lds, srt) and np.array_equal(whole, lds))
res["first_record"] = [int(v) for v in lds[0]]
res["spectrums"] = counts
print(json.dumps(res))
with open(out_path, "w") as f:
    f.write(json.dumps(res) + "\n")
assert res["paths_agree"], "the LDS path and the sorted path disagree"
