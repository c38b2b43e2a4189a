"""development tool: TnfDistance at the shape of a few shredded genomes -- 8 inputs of one 5 Mb contig each (made on the host from a
seed, every input with a GC content of its own), window 10000, step 1000, so 5000 windows an input.  HIP events on the handle's
stream, one warm-up, then the median of the repetitions with every value shown:
  (a) tnf_reads, tnf_windows       kmr_tnf_reads / kmr_tnf_windows at k = 4 over the 8 inputs: bases/s, and window-bases/s for the windows
  (b) likelihoods_<formula>        kmr_tnf_likelihoods on the same: pairs/s and pair-columns/s (a pair-column: one column of one pair)
  (c) triangle_k<k>_<formula>      kmr_tnf_distances_dev of the strict lower triangle of 20 000 vectors (the windows of the first four
                                   inputs) at k = 4 and at k = 6, the per-vector part made by the warm-up
Prints one JSON line and writes it to out.json (default profiles/tnf_bench.json).
usage: tools/tnf_bench.py [inputs] [repetitions] [out.json] [--only-triangle]"""
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
n_inputs = int(args[0]) if len(args) > 0 else 8
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "tnf_bench.json")
only_triangle = "--only-triangle" in sys.argv
WINDOW, STEP, PER_INPUT = 10000, 1000, 5000
L = WINDOW + STEP * PER_INPUT                    # i < L - window: exactly PER_INPUT windows
dev = torch.device("cuda", 0)


def contigs(m):
    rng = np.random.default_rng(7)
    out = []
    for i in range(m):
        gc = 0.30 + 0.05 * i
        out.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=L, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])])
    return np.concatenate(out)


def read_set(sp, m, bases):
    b = bases[:m * L]
    return ka.ReadSet.from_arrays(sp, b, np.full(b.size, 127, dtype=np.uint8), np.arange(m + 1, dtype=np.uint64) * L)


def timed(sp, fn):
    stream = torch.cuda.ExternalStream(sp.stream(), device=dev)
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


bases = contigs(n_inputs)
starts = np.arange(n_inputs + 1, dtype=np.uint64)
res = {"tool": "tnf_bench", "inputs": n_inputs, "contig_bases": L, "window": WINDOW, "step": STEP, "repetitions": reps, "all": {}, "rates": {}}
med = lambda name: float(np.median(res["all"][name]))

sp4 = ka.KmerSpectrum(ka.default_config(4, device=0, estimated_raw_kmers=4096))
D4 = ka.tnf_dims(4)
if not only_triangle:
    rs = read_set(sp4, n_inputs, bases)
    keep = {}

    def vectors(name, make):
        def fn():
            with make() as t:
                keep[name] = t.n
        res["all"][name] = timed(sp4, fn)

    vectors("tnf_reads", lambda: rs.tnf(starts))
    vectors("tnf_windows", lambda: rs.tnfWindows(WINDOW, STEP, input_starts=starts))
    res["windows"] = keep["tnf_windows"]
    res["rates"]["tnf_reads_bases_per_s"] = n_inputs * L / (med("tnf_reads") * 1e-3)
    res["rates"]["tnf_windows_bases_per_s"] = n_inputs * L / (med("tnf_windows") * 1e-3)
    res["rates"]["tnf_windows_window_bases_per_s"] = keep["tnf_windows"] * WINDOW / (med("tnf_windows") * 1e-3)
    for formula, fname in ((0, "euclidean"), (1, "spearman")):
        hist = {}
        name = "likelihoods_" + fname
        res["all"][name] = timed(sp4, lambda: hist.update(h=rs.tnfLikelihoods(starts, window=WINDOW, step=STEP, bins=100, formula=formula)))
        pairs = int(hist["h"].sum())
        res[name + "_pairs"] = pairs
        res[name + "_totals"] = [int(x) for x in hist["h"].sum(axis=1)]
        res["rates"][name + "_pairs_per_s"] = pairs / (med(name) * 1e-3)
        res["rates"][name + "_pair_columns_per_s"] = pairs * D4 / (med(name) * 1e-3)
    rs.close()

for k in (4, 6):
    sp = sp4 if k == 4 else ka.KmerSpectrum(ka.default_config(6, device=0, estimated_raw_kmers=4096))
    m = min(4, n_inputs)
    with read_set(sp, m, bases) as rs, rs.tnfWindows(WINDOW, STEP) as t:
        n, D = t.n, t.dims
        pairs = n * (n - 1) // 2
        out = torch.zeros(max(pairs, 1), dtype=torch.float32, device=dev)
        for formula, fname in ((0, "euclidean"), (1, "spearman")):
            name = "triangle_k%d_%s" % (k, fname)
            res["all"][name] = timed(sp, lambda: sp._call("tnf_distances_dev", sp.h, t._t, None, formula, 0, n, C.c_void_p(out.data_ptr())))
            res[name + "_vectors"], res[name + "_pairs"] = n, pairs
            res["rates"][name + "_pairs_per_s"] = pairs / (med(name) * 1e-3)
            res["rates"][name + "_pair_columns_per_s"] = pairs * D / (med(name) * 1e-3)
            res[name + "_checksum"] = float(out[:pairs].double().sum().item())
        del out
    if k != 4:
        sp.close()
sp4.close()
for name, ms in res["all"].items():
    res[name + "_ms"] = float(np.median(ms))
print(json.dumps(res))
with open(out_path, "w") as f:
    f.write(json.dumps(res) + "\n")
