"""development tool: the last stage of FilterReads on a C2-size batch (10 M x 150 bp, the bench's generator, noisy qualities, k = 31,
min depth 2), two routes to the same bytes:
 (i)  kmr_filter_read_batch_dev: scoring, then selection + output text on the device (HIP-event times of kmr_build_info, kmr_tune
      select_timing), and the copy of the text to the host;
 (ii) what the library offered before: kmr_score_read_batch + kmr_reads_copy to the host + a compiled, single-threaded host loop that
      formats the records (the C++ below; the reference's writePicks is a serial ostream loop too).
Prints one JSON line.  usage: tools/select_bench.py [reads] [repetitions]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmernator_amd as ka
import bench

HOST_LOOP = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
static bool passes(float len, uint32_t rl, float m) { if (len <= 1.0f) return false; return m <= 1.0f ? rl * m <= len : m <= len; }
extern "C" uint64_t format_picks(uint64_t n, const char *bases, const char *quals, const uint64_t *off, const char *text, const uint64_t *name_off,
                                 const uint32_t *name_len, const uint32_t *to, const uint32_t *tl, const float *sc, const uint8_t *wt,
                                 float min_score, float mrl, int both, int shift, int out_base, char *out) {
	char *o = out;
	for (uint64_t a = 0; a + 1 < n; a += 2) {
		bool p[2];
		for (int j = 0; j < 2; j++) p[j] = sc[a + j] >= min_score && passes((float)tl[a + j], (uint32_t)(off[a + j + 1] - off[a + j]), mrl);
		if (!(both ? (p[0] && p[1]) : (p[0] || p[1]))) continue;
		for (uint64_t i = a; i < a + 2; i++) {
			*o++ = '@';
			uint32_t nl = 0; const char *nm = text + name_off[i];
			while (nl < name_len[i] && nm[nl] != ' ' && nm[nl] != '\t') nl++;
			memcpy(o, nm, nl); o += nl;
			if (wt[i]) o += sprintf(o, " Trim:%u+%u", to[i], tl[i]);
			o += sprintf(o, " MedianScore:%d\n", (int)(sc[i] + 0.5));
			const uint32_t L = tl[i];
			if (L <= 1) { memcpy(o, "N\n+\n", 4); o += 4; *o++ = (char)(out_base + 1); *o++ = '\n'; continue; }
			memcpy(o, bases + off[i] + to[i], L); o += L; memcpy(o, "\n+\n", 3); o += 3;
			const char *q = quals + off[i] + to[i];
			for (uint32_t j = 0; j < L; j++) o[j] = (char)(q[j] + shift);
			o += L; *o++ = '\n';
		}
	}
	return (uint64_t)(o - out);
}
"""

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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

sp = ka.KmerSpectrum(ka.default_config(bench.K, estimated_raw_kmers=n * (L - bench.K + 1), device=0))
lib = sp.lib
r = C.c_void_p()
rc = lib.kmr_ingest_fastq_dev(sp.h, text.data_ptr(), text.numel(), 33, 1, C.byref(r))
assert rc == 0, lib.kmr_last_error(sp.h)
rc = lib.kmr_add_read_batch(sp.h, r, 0)
assert rc == 0, lib.kmr_last_error(sp.h)
sp.finalize(2)
mate = np.arange(n, dtype=np.int64) ^ 1
cfg = ka.KmrSelectConfig()
lib.kmr_select_config_init(C.byref(cfg))
cfg.min_read_length = 0.5
i64p = C.POINTER(C.c_int64)


sp.tune(select_timing=1)


def route_device():
    out = C.c_void_p()
    rc = lib.kmr_filter_read_batch_dev(sp.h, r, text.data_ptr(), text.numel(), mate.ctypes.data_as(i64p), None, None, None, C.byref(cfg), C.byref(out))
    assert rc == 0, lib.kmr_last_error(sp.h)
    t = {k: sp.build_info(k) for k in ("filter_score_ms", "select_ms", "select_write_ms")}
    npk, nb = C.c_uint64(), C.c_uint64()
    lib.kmr_picks_info(out, C.byref(npk), C.byref(nb))
    return out, t, npk.value, nb.value


out, _, n_picked, n_bytes = route_device()          # warm-up, and the sizes
lib.kmr_picks_free(out)
host_text = np.zeros(n_bytes + 64, dtype=np.uint8)
times, d2h = [], []
for rep in range(reps):
    out, t, _, _ = route_device()
    times.append(t)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    assert lib.kmr_picks_copy(out, host_text.ctypes.data_as(C.c_void_p), n_bytes, None) == 0
    d2h.append((time.perf_counter() - t0) * 1e3)
    lib.kmr_picks_free(out)
device_text = host_text[:n_bytes].copy()

# route (ii)
tmp = tempfile.mkdtemp()
open(os.path.join(tmp, "host_loop.cpp"), "w").write(HOST_LOOP)
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", os.path.join(tmp, "host_loop.so"), os.path.join(tmp, "host_loop.cpp")])
hl = C.CDLL(os.path.join(tmp, "host_loop.so"))
hl.format_picks.restype = C.c_uint64
vp = C.c_void_p
hl.format_picks.argtypes = [C.c_uint64] + [vp] * 10 + [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, vp]
total = n * L
hb, hq = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
ho, no, nl = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
to, tl, sc, wt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
htext = text.cpu().numpy()          # the host has the file's text anyway (names)
host_out = np.zeros(n_bytes + 4096, dtype=np.uint8)
p = lambda a: a.ctypes.data_as(vp)
host = []
for rep in range(reps + 1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    rc = lib.kmr_score_read_batch(sp.h, r, 2.0, 1, to.ctypes.data_as(C.POINTER(C.c_uint32)), tl.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0, lib.kmr_last_error(sp.h)
    t1 = time.perf_counter()
    assert lib.kmr_reads_copy(r, p(hb), p(hq), ho.ctypes.data_as(C.POINTER(C.c_uint64)), no.ctypes.data_as(C.POINTER(C.c_uint64)), nl.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    t2 = time.perf_counter()
    nb2 = hl.format_picks(n, p(hb), p(hq), p(ho), p(htext), p(no), p(nl), p(to), p(tl), p(sc), p(wt), 2.0, 0.5, 0, 0, 33, p(host_out))
    t3 = time.perf_counter()
    if rep:          # the first round warms up
        host.append({"score_ms": (t1 - t0) * 1e3, "reads_copy_ms": (t2 - t1) * 1e3, "format_ms": (t3 - t2) * 1e3})
same = bool(nb2 == n_bytes and np.array_equal(host_out[:n_bytes], device_text))

med = lambda xs: float(np.median(xs))
writer = med([t["select_write_ms"] for t in times])
# what the writer moves: the picked reads' bases and qualities and their names in, the text out
picked_in = n_bytes - 6 * n_picked
HBM_PEAK = 8.0e12
res = {
    "tool": "select_bench", "reads": n, "read_len": L, "k": bench.K, "repetitions": reps, "picked": n_picked, "output_bytes": n_bytes,
    "device_route_ms": {"scoring": med([t["filter_score_ms"] for t in times]), "select_and_write": med([t["select_ms"] for t in times]), "writer": writer, "text_to_host": med(d2h)},
    "writer_all_ms": [t["select_write_ms"] for t in times],
    "writer_bytes_per_s": (picked_in + n_bytes) / (writer * 1e-3), "writer_share_of_hbm_peak": (picked_in + n_bytes) / (writer * 1e-3) / HBM_PEAK,
    "host_route_ms": {k: med([h[k] for h in host]) for k in ("score_ms", "reads_copy_ms", "format_ms")},
    "host_route_same_bytes": same,
}
res["device_route_text_on_device_ms"] = res["device_route_ms"]["scoring"] + res["device_route_ms"]["select_and_write"]
res["device_route_total_with_copy_ms"] = res["device_route_text_on_device_ms"] + res["device_route_ms"]["text_to_host"]
res["host_route_total_ms"] = sum(res["host_route_ms"].values())
print(json.dumps(res))
assert same, "the host loop and the device disagree"
