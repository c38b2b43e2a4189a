"""development tool: ContigExtender on C2's shape (10 M x 150 bp made on the device, the spectrum of the same reads at k = 31, min-depth 2)
with the pools KmerMatch gives (edge setting 500, no sampling cut beyond the default):
  narrow  the match benchmark's 25 contigs of 3000 bp cut from the generator's genome
  wide    a few thousand contigs of 500 bp cut from the same genome
each at k = 31 (one key word) and k = 101 (four key words; the pools are the same reads).  HIP events inside the library (kmr_tune
"extend_timing": gather, extract, sort, reduce, walk) and around the whole call, one warm-up, then the median of the repetitions with
every value shown.  For context the wall time of the serial restatement of tests/refextend.py on the narrow input at k = 31: that is
Python over the C++ oracle, not the reference.  Prints one JSON line and writes it to out.json (default profiles/extend_bench.json).
usage: tools/extend_bench.py [reads] [repetitions] [wide contigs] [out.json]"""
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
n = int(args[0]) if len(args) > 0 else 10_000_000
reps = int(args[1]) if len(args) > 1 else 5
n_wide = int(args[2]) if len(args) > 2 else 3000
out_path = args[3] if len(args) > 3 else os.path.join(ROOT, "profiles", "extend_bench.json")
L, K, K4, SEED, EDGE = 150, 31, 101, 1, 500
dev = torch.device("cuda", 0)
genome = 5 * n
M64 = (1 << 64) - 1
PHASES = ("gather", "extract", "sort", "reduce", "walk")


def genome_bases(start, length):
    """the generator's genome (kmr_synth.hpp): base j = (next(state(seed, 1, j >> 5)) >> 2 (j & 31)) & 3"""
    def word(block):
        z = ((SEED ^ (1 * 0xD1B54A32D192ED03)) + block * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        s = z if z else 0x9E3779B97F4A7C15
        s ^= s >> 12; s = (s ^ (s << 25)) & M64; s ^= s >> 27
        return (s * 0x2545F4914F6CDD1D) & M64
    words = {}
    out = bytearray()
    for j in range(start, start + length):
        w = words.setdefault(j >> 5, word(j >> 5))
        out.append(b"ACGT"[(w >> (2 * (j & 31))) & 3])
    return bytes(out)


def contig_set(sp, contigs):
    return ka.ReadSet.from_fasta(sp, b"".join(b">c%d\n%s\n" % (i, s) for i, s in enumerate(contigs)))


b, q, o = ka.synth_reads_device(torch, SEED, 0, n, L, genome, False, dev)
sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=n * (L - K + 1), device=0))
sp.buildKmerSpectrumDevice(b.data_ptr(), q.data_ptr(), o.data_ptr(), n, n * L)
sp.finalize(2)
hb, hq, ho = b[:n * L].cpu().numpy(), q[:n * L].cpu().numpy(), o[:n + 1].cpu().numpy().astype(np.uint64)
rs = ka.ReadSet.from_arrays(sp, hb, hq, ho)
sp4 = ka.KmerSpectrum(ka.default_config(K4, estimated_raw_kmers=4096, device=0))      # never fed: k and the config
sp.tune(extend_timing=1)
sp4.tune(extend_timing=1)
torch.cuda.synchronize()

res = {"tool": "extend_bench", "reads": n, "read_len": L, "edge": EDGE, "repetitions": reps, "max_extend": 50, "cases": {}}
for shape, count, length in (("narrow", 25, 3000), ("wide", n_wide, 500)):
    stride = (genome - length) // count
    contigs = [genome_bases(i * stride, length) for i in range(count)]
    cs = contig_set(sp, contigs)
    with ka.KmerMatch(sp, cs, EDGE) as km:
        km.addReads(rs, 0)
        pools = km.finish()
    for k, handle in ((K, sp), (K4, sp4)):
        case = {"contigs": count, "contig_len": length, "k": k, "pooled_reads": int(pools.reads.size), "largest_pool": int(np.diff(pools.offsets.astype(np.int64)).max()),
                "all": {p: [] for p in PHASES + ("call_wall",)}}
        ex = ka.ContigExtender(handle)
        for rep in range(reps + 1):          # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ex.extendContigs(cs, rs, pools) as r:
                wall = (time.perf_counter() - t0) * 1e3
                case.update(extended=r.n_extended, bases_added=r.bases_added, runs=handle.build_info("extend_runs"))
            if rep:
                for p in PHASES:
                    case["all"][p].append(handle.build_info("extend_%s_ms" % p))
                case["all"]["call_wall"].append(wall)
        for p, ms in case["all"].items():
            case[p + "_ms"] = float(np.median(ms))
        res["cases"]["%s_k%d" % (shape, k)] = case
    if shape == "narrow":                    # the serial restatement on the same input, for context: Python over the C++ oracle
        import refextend as rx
        from helpers import default_config
        reads_of = lambda ids: [(hb[int(ho[j]):int(ho[j + 1])].tobytes(), hq[int(ho[j]):int(ho[j + 1])].tobytes()) for j in ids]
        t0 = time.perf_counter()
        w = rx.Extender(default_config(K)).extend(contigs, [reads_of(pools[i]) for i in range(count)])
        res["restatement_python_narrow_k31_s"] = time.perf_counter() - t0
        with ka.ContigExtender(sp).extendContigs(cs, rs, pools) as r:
            res["narrow_k31_equals_restatement"] = bool(r.sequences() == [x[0] for x in w])
    cs.close()
print(json.dumps(res))
with open(out_path, "w") as f:
    f.write(json.dumps(res) + "\n")
