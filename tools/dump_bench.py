"""development tool: MeraculousCounter's two text products on a C2-size spectrum (10 M x 150 bp, the bench's generator, noisy
qualities, k = 31, extension values, MeraculousCounter's settings: min_weight 0, min_quality_score 2; min depth 2).  For mercount
and mergraph: HIP-event times of the size pass (with its scan) and of the writer (kmr_build_info, kmr_tune dump_timing), medians of
the repetitions after a warm-up, the kept entries and the bytes of the text, the writer's bytes per second (map bytes read plus
text written over the writer's time) and the time of kmr_text_copy.  With a path as third argument, also the wall time of the
file forms (kmr_dump_mercount / kmr_dump_mergraph) appending to files in that directory.
Runs the project's own library only.  Prints one JSON line.  usage: tools/dump_bench.py [reads] [repetitions] [directory]"""
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_dir = sys.argv[3] if len(sys.argv) > 3 else None
L, K, MIN_DEPTH = bench.READ_LEN, bench.K, 2
dev = torch.device("cuda", 0)
bases, quals, offsets = bench.gen_reads(torch, n, 5 * n, 1234, 0, dev, "noisy")
sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=n * (L - K + 1), device=0, value_kind=ka.KMR_VALUE_EXT, min_weight=0.0, min_quality_score=2))
torch.cuda.synchronize(); t0 = time.perf_counter()
sp.buildKmerSpectrumDevice(bases.data_ptr(), quals.data_ptr(), offsets.data_ptr(), n, n * L, 0)
sp.finalize(MIN_DEPTH)
build_ms = (time.perf_counter() - t0) * 1e3
del bases, quals, offsets
entries = sp.stats()["weak_entries"]
sp.tune(dump_timing=1)
med = lambda xs: float(np.median(xs))
HBM_PEAK, SELECT_WRITER = 8.0e12, 222e9
res = {"tool": "dump_bench", "reads": n, "read_len": L, "k": K, "min_depth": MIN_DEPTH, "repetitions": reps, "weak_entries": entries, "build_wall_ms": build_ms}
for kind, make in (("mercount", sp.dumpCountsText), ("mergraph", sp.dumpGraphsText)):
    make(MIN_DEPTH).close()          # warm-up
    size_ms, write_ms, copy_ms, size_only_ms = [], [], [], []
    for rep in range(reps):
        kept, nbytes = sp.dumpTextSize(kind, MIN_DEPTH)
        size_only_ms.append(sp.build_info("dump_size_ms"))
        t = make(MIN_DEPTH)
        size_ms.append(sp.build_info("dump_size_ms")); write_ms.append(sp.build_info("dump_write_ms"))
        assert (t.kept, t.bytes) == (kept, nbytes)
        if rep == 0:
            host = np.zeros(nbytes, dtype=np.uint8)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        assert sp.lib.kmr_text_copy(t._t, host.ctypes.data_as(C.c_void_p), nbytes) == 0
        copy_ms.append((time.perf_counter() - t0) * 1e3)
        t.close()
    # what the writer moves: every entry's offset pair, a kept entry's key and value words in, the text out
    map_in = 8 * entries + kept * (8 * ((K + 31) // 32) + 4 * 15)
    w = med(write_ms)
    res[kind] = {"kept": kept, "text_bytes": nbytes, "size_pass_ms": med(size_ms), "size_pass_all_ms": size_ms, "size_only_call_ms": med(size_only_ms),
                 "writer_ms": w, "writer_all_ms": write_ms, "text_to_host_ms": med(copy_ms), "text_to_host_all_ms": copy_ms,
                 "writer_bytes_per_s": (map_in + nbytes) / (w * 1e-3), "writer_share_of_hbm_peak": (map_in + nbytes) / (w * 1e-3) / HBM_PEAK,
                 "writer_over_select_writer": (map_in + nbytes) / (w * 1e-3) / SELECT_WRITER}
    del host
    if out_dir:
        path = os.path.join(out_dir, "dump_bench." + kind)
        file_ms = []
        for rep in range(reps):
            if os.path.exists(path):
                os.remove(path)
            t0 = time.perf_counter()
            (sp.dumpCounts if kind == "mercount" else sp.dumpGraphs)(path, MIN_DEPTH)
            file_ms.append((time.perf_counter() - t0) * 1e3)
        assert os.path.getsize(path) == nbytes
        os.remove(path)
        res[kind]["file_form_ms"] = med(file_ms); res[kind]["file_form_all_ms"] = file_ms
print(json.dumps(res))
