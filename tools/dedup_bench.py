"""development tool: the duplicate-fragment stage on a C2-size batch (10 M x 150 bp as 5 M interleaved pairs, FASTQ text made on the
device, pseudo-random bases, noisy qualities; of every five fragments the fifth is emitted three times, so seven pairs hold five
fragments): kmr_dedup_fragments_dev with dedup_mode 2 and length 24, HIP-event times of kmr_build_info (kmr_tune dedup_timing): the
whole call, the key kernel, the sorts, the consensus kernel; one warm-up run, then the median of the repetitions with every value
shown.  The group count and the discard count are checked against what the layout implies.  Prints one JSON line.
usage: tools/dedup_bench.py [reads] [repetitions]"""
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
from kmernator_amd import _lib

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10_000_000
reps = int(args[1]) if len(args) > 1 else 5
n_pairs = n // 2 // 7 * 7
n = 2 * n_pairs
blocks = n_pairs // 7
L, DIGITS = 150, 10
dev = torch.device("cuda", 0)
NAME = 1 + DIGITS + 2
REC = 1 + NAME + 1 + L + 3 + L + 1


def mix(x):
    x = (x ^ (x >> 31)) * 0x7fb5d329728ea185
    x = (x ^ (x >> 27)) * 0x2545f4914f6cdd1d
    return x ^ (x >> 33)


def fastq_text():
    text = torch.empty((n, REC), dtype=torch.uint8, device=dev)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    pos = torch.arange(L, device=dev, dtype=torch.int64)
    for lo in range(0, n, 1 << 20):
        hi = min(n, lo + (1 << 20))
        idx = torch.arange(lo, hi, device=dev, dtype=torch.int64)
        pair, end = idx >> 1, idx & 1
        src = (pair // 7) * 5 + torch.clamp(pair % 7, max=4)          # slots 4, 5, 6 of a block are one fragment
        t = text[lo:hi]
        t[:, 0] = ord("@"); t[:, 1] = ord("r")
        for d in range(DIGITS):
            t[:, 2 + d] = ((pair // 10 ** (DIGITS - 1 - d)) % 10 + 48).to(torch.uint8)
        t[:, 2 + DIGITS] = ord("/"); t[:, 3 + DIGITS] = (end + 49).to(torch.uint8)
        c = 1 + NAME
        h = mix((src * 2 + end)[:, None] * 1000003 + pos[None, :])
        t[:, c] = 10; t[:, c + 1:c + 1 + L] = acgt[(h & 3)]; c += 1 + L
        q = mix(idx[:, None] * 1000033 + pos[None, :])          # qualities differ between the copies
        t[:, c] = 10; t[:, c + 1] = ord("+"); t[:, c + 2] = 10; t[:, c + 3:c + 3 + L] = (33 + ((q >> 8) & 0xffff) % 41).to(torch.uint8); t[:, c + 3 + L] = 10
    return text.view(-1)


sp = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1 << 20, device=0))
lib = sp.lib
sp.tune(dedup_timing=1)
text = fastq_text()
torch.cuda.synchronize()
r = C.c_void_p()
assert lib.kmr_ingest_fastq_dev(sp.h, text.data_ptr(), text.numel(), 33, 1, C.byref(r)) == 0, lib.kmr_last_error(sp.h)
pairs = C.c_void_p()
assert lib.kmr_identify_pairs_dev(sp.h, r, text.data_ptr(), text.numel(), 1, C.byref(pairs)) == 0, lib.kmr_last_error(sp.h)
cfg = _lib.KmrDedupConfig()
lib.kmr_dedup_config_init(C.byref(cfg))
cfg.dedup_mode, cfg.dedup_length = 2, 24
KEYS = ("dedup_ms", "dedup_key_ms", "dedup_sort_ms", "dedup_consensus_ms")
runs = []
for rep in range(reps + 1):          # the first run warms up
    out = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.kmr_dedup_fragments_dev(sp.h, r, text.data_ptr(), text.numel(), pairs, None, C.byref(cfg), C.byref(out))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kmr_last_error(sp.h)
    t = {k: sp.build_info(k) for k in KEYS}
    t["wall_ms"] = wall
    if rep:
        runs.append(t)
    if rep < reps:
        lib.kmr_dedup_free(out)
ng, nn, af = C.c_uint64(), C.c_uint64(), C.c_uint64()
sk = (C.c_uint64 * 4)()
lib.kmr_dedup_info(out, C.byref(ng), C.byref(nn), C.byref(af), sk)
disc = np.zeros(n, dtype=np.uint8)
assert lib.kmr_dedup_copy(out, disc.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == 0
cons, nt, nl = C.c_void_p(), C.c_void_p(), C.c_uint64()
lib.kmr_dedup_reads(out, C.byref(cons), C.byref(nt), C.byref(nl))
cn, ct = C.c_uint64(), C.c_uint64()
lib.kmr_reads_info(cons, C.byref(cn), C.byref(ct), None, None)
ok = ng.value == blocks and int(disc.sum()) == 6 * blocks and nn.value == 2 * blocks and af.value == 6 * blocks and ct.value == 2 * blocks * L
med = lambda k: float(np.median([t[k] for t in runs]))
# the consensus kernel reads the bases and qualities of every member and writes those of the consensus reads and their names
cons_bytes = 2 * int(af.value) * L + 2 * int(ct.value) + int(nl.value)
res = {"tool": "dedup_bench", "reads": n, "pairs": n_pairs, "read_len": L, "repetitions": reps, "dedup_mode": 2, "dedup_length": 24,
       "total_ms": med("dedup_ms"), "key_ms": med("dedup_key_ms"), "sort_ms": med("dedup_sort_ms"), "consensus_ms": med("dedup_consensus_ms"), "wall_ms": med("wall_ms"),
       "all": {k: [t[k] for t in runs] for k in KEYS + ("wall_ms",)},
       "groups": ng.value, "new_reads": nn.value, "affected": af.value, "skipped": [int(v) for v in sk], "discarded": int(disc.sum()),
       "as_the_layout_implies": bool(ok), "consensus_bytes": cons_bytes}
res["consensus_gbps"] = cons_bytes / (res["consensus_ms"] * 1e-3) / 1e9 if res["consensus_ms"] else 0.0
res["consensus_share_of_8tbps"] = res["consensus_gbps"] / 8000.0
lib.kmr_dedup_free(out); lib.kmr_pairs_free(pairs); lib.kmr_reads_free(r)
print(json.dumps(res))
assert ok, "groups / discards are not what the layout implies"
