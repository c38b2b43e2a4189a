"""development tool: ReadSet::identifyPairs on a C2-size batch (10 M reads as FASTQ text made on the device, the names of
tools/select_bench.py -- "r%010d", here the fragment's number -- with /1 or /2 behind them), once interleaved and once as an R1 block
followed by an R2 block: kmr_identify_pairs_dev, HIP-event times of kmr_build_info (kmr_tune pairs_timing): the whole call, its name
parse and its radix sort; one warm-up run, then the median of the repetitions.  With --baseline also the wall time of the sequential
Python restatement of tests/refpairs.py on the same names (an interpreted baseline, for scale only), whose result the device's must equal.
Prints one JSON line.  usage: tools/pairs_bench.py [reads] [repetitions] [--baseline]"""
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import kmernator_amd as ka

args = [a for a in sys.argv[1:] if not a.startswith("--")]
baseline = "--baseline" in sys.argv
n = int(args[0]) if len(args) > 0 else 10_000_000
reps = int(args[1]) if len(args) > 1 else 5
n -= n & 1
L, DIGITS = 150, 10
dev = torch.device("cuda", 0)


def fastq_text(fragment, end):
    """"@r%010d/%d\\n" bases "\\n+\\n" quals "\\n" per read, on the device (bases and qualities are one character each: the names are what matters)"""
    name = 1 + DIGITS + 2
    rec = 1 + name + 1 + L + 3 + L + 1
    text = torch.empty((n, rec), dtype=torch.uint8, device=dev)
    text[:, 0] = ord("@"); text[:, 1] = ord("r")
    for d in range(DIGITS):
        text[:, 2 + d] = ((fragment // 10 ** (DIGITS - 1 - d)) % 10 + 48).to(torch.uint8)
    text[:, 2 + DIGITS] = ord("/"); text[:, 3 + DIGITS] = (end + 49).to(torch.uint8)
    c = 1 + name
    text[:, c] = 10; text[:, c + 1:c + 1 + L] = ord("A"); c += 1 + L
    text[:, c] = 10; text[:, c + 1] = ord("+"); text[:, c + 2] = 10; text[:, c + 3:c + 3 + L] = ord("I"); text[:, c + 3 + L] = 10
    return text.view(-1)


idx = torch.arange(n, device=dev, dtype=torch.int64)
layouts = {"interleaved": (idx >> 1, idx & 1), "r1_then_r2": (idx % (n // 2), idx // (n // 2))}
sp = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1 << 20, device=0))
lib = sp.lib
sp.tune(pairs_timing=1)
med = lambda xs: float(np.median(xs))
res = {"tool": "pairs_bench", "reads": n, "read_len": L, "repetitions": reps, "layouts": {}}
for layout, (fragment, end) in layouts.items():
    text = fastq_text(fragment, end)
    torch.cuda.synchronize()
    r = C.c_void_p()
    rc = lib.kmr_ingest_fastq_dev(sp.h, text.data_ptr(), text.numel(), 33, 1, C.byref(r))
    assert rc == 0, lib.kmr_last_error(sp.h)
    runs = []
    for rep in range(reps + 1):          # the first run warms up
        out = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.kmr_identify_pairs_dev(sp.h, r, text.data_ptr(), text.numel(), 1, C.byref(out))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, lib.kmr_last_error(sp.h)
        t = {k: sp.build_info(k) for k in ("pairs_ms", "pairs_parse_ms", "pairs_sort_ms")}
        t["wall_ms"] = wall
        if rep:
            runs.append(t)
        if rep < reps:
            lib.kmr_pairs_free(out)
    v = [C.c_uint64() for _ in range(5)]
    hp = C.c_int()
    lib.kmr_pairs_info(out, *[C.byref(x) for x in v], C.byref(hp))
    mate = np.zeros(n, dtype=np.int64)
    assert lib.kmr_pairs_copy(out, mate.ctypes.data_as(C.POINTER(C.c_int64)), None, None) == 0
    lib.kmr_pairs_free(out)
    expect = np.arange(n, dtype=np.int64) ^ 1 if layout == "interleaved" else (np.arange(n, dtype=np.int64) + n // 2) % n
    ok = bool(np.array_equal(mate, expect))
    total = med([t["pairs_ms"] for t in runs])
    entry = {"total_ms": total, "parse_ms": med([t["pairs_parse_ms"] for t in runs]), "sort_ms": med([t["pairs_sort_ms"] for t in runs]),
             "wall_ms": med([t["wall_ms"] for t in runs]), "total_all_ms": [t["pairs_ms"] for t in runs],
             "pairs": v[1].value, "full": v[2].value, "sequential": v[3].value, "conflicts": v[4].value, "has_pairs": bool(hp.value), "mate_as_expected": ok}
    entry["parse_share"] = entry["parse_ms"] / total if total else 0.0
    entry["sort_share"] = entry["sort_ms"] / total if total else 0.0
    if baseline:
        import refpairs
        frag, e = fragment.cpu().numpy(), end.cpu().numpy()
        lines = ["r%010d/%d" % (f, x + 1) for f, x in zip(frag.tolist(), e.tolist())]
        t0 = time.perf_counter()
        want = refpairs.identify_pairs(lines, 1)
        entry["python_restatement_s"] = time.perf_counter() - t0
        entry["same_as_restatement"] = bool(np.array_equal(mate, want.mate_array()) and want.n_pairs == v[1].value and want.n_sequential == v[3].value)
        del lines, want
    res["layouts"][layout] = entry
    lib.kmr_reads_free(r)
    del text
    assert ok, "mate is not what the layout implies"
print(json.dumps(res))
