"""development tool: KmerMatch on C2's shape (10 M x 150 bp made on the device, k = 31, the spectrum of the same reads at min-depth 2)
against 25 contigs of 3000 bp cut from the generator's genome, edge setting 500.  HIP events on the handle's stream, one warm-up, then
the median of the repetitions with every value shown:
  create          kmr_match_create: the edge keys of the contigs, sorted, filtered against the spectrum, into the table
  add_read_batch  kmr_match_add_read_batch of the whole batch in one call (the extraction with MatchOp; no mates, no discard flags)
  finish          kmr_match_finish: sort, unique, sample, sort again, offsets
  compare_reads   kmr_compare_reads_dev of the same batch, for comparison: the same extraction with per-read de-duplication in LDS and
                  a lookup in the whole spectrum
Also the hits (reads of all sets before sampling), the largest set and the table's figures.  Prints one JSON line and writes it to
out.json (default profiles/match_bench.json).
usage: tools/match_bench.py [reads] [repetitions] [out.json]"""
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
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "match_bench.json")
L, K, SEED = 150, 31, 1
N_CONTIGS, CONTIG_LEN, EDGE = 25, 3000, 500
dev = torch.device("cuda", 0)
genome = 5 * n
M64 = (1 << 64) - 1


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


b, q, o = ka.synth_reads_device(torch, SEED, 0, n, L, genome, False, dev)
sp = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=n * (L - K + 1), device=0))
sp.buildKmerSpectrumDevice(b.data_ptr(), q.data_ptr(), o.data_ptr(), n, n * L)
sp.finalize(2)
stream = torch.cuda.ExternalStream(sp.stream(), device=dev)
rs = ka.ReadSet.from_arrays(sp, b[:n * L].cpu().numpy(), q[:n * L].cpu().numpy(), o[:n + 1].cpu().numpy().astype(np.uint64))
stride = (genome - CONTIG_LEN) // N_CONTIGS
contigs = [genome_bases(i * stride, CONTIG_LEN) for i in range(N_CONTIGS)]
cs = ka.ReadSet(sp, b"".join(b"@c%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(contigs)), 33)
out = torch.zeros(n * 8, dtype=torch.int64, device=dev)
torch.cuda.synchronize()


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


res = {"tool": "match_bench", "reads": n, "read_len": L, "k": K, "min_depth": 2, "contigs": N_CONTIGS, "contig_len": CONTIG_LEN, "edge": EDGE, "repetitions": reps,
       "all": {"create": [], "add_read_batch": [], "finish": [], "compare_reads": []}}
for rep in range(reps + 1):          # the first run warms up
    t_create, km = span(lambda: ka.KmerMatch(sp, cs, EDGE))
    t_add, _ = span(lambda: km.addReads(rs, 0))
    t_finish, r = span(km.finish)
    t_cmp, _ = span(lambda: sp._call("compare_reads_dev", sp.h, rs.r, C.c_void_p(out.data_ptr())))
    if rep:
        for name, t in (("create", t_create), ("add_read_batch", t_add), ("finish", t_finish), ("compare_reads", t_cmp)):
            res["all"][name].append(t)
    res.update(edge_kmers=km.n_edge_kmers, distinct_keys=km.n_distinct_keys, keys_in_spectrum=km.n_keys_in_spectrum, hits=int(r.size_before_sampling.sum()),
               largest_set=int(r.size_before_sampling.max()), reads_in_result=int(r.reads.size), sampled_contigs=r.n_sampled_contigs,
               add_attempts=sp.build_info("match_add_attempts"))
    km.close()
for name, ms in res["all"].items():
    res[name + "_ms"] = float(np.median(ms))
res["add_over_compare"] = res["add_read_batch_ms"] / res["compare_reads_ms"]
print(json.dumps(res))
with open(out_path, "w") as f:
    f.write(json.dumps(res) + "\n")
