"""development tool: what the artifact filter's report costs.  1 M reads x 150 bp of the bench's generator, as pairs (even, odd), with a
planted share of adapter reads (2 % trimmed, 1 % discarded) and PhiX reads (1 %), ingested from FASTQ text made on the device.  Timed
with HIP events on the handle's stream around each call, one warm-up round and the median of 5, the calls taking turns:
  apply          kmr_artifact_filter_apply alone (no host array asked for, the filtered batch made)
  apply_report   kmr_artifact_filter_apply_report_dev on the same batch: the same work plus the report
  reads_copy     kmr_reads_copy of the unfiltered batch, which a host route to the PhiX and Artifact files would have to pay first
for flat and for noisy qualities (noisy: most reads lose bases to the quality screen, so nearly every read is counted), with the
counters where the library puts them by default and forced to global atomics (kmr_tune artifact_report_lds).
Prints one JSON line and writes it to the path given.  usage: tools/artifact_report_bench.py [out.json] [reads]"""
import ctypes as C
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmernator_amd as ka
import bench

ROUNDS = 5
L, NAME = bench.READ_LEN, 11


def lcg_bases(n, seed):
    x, out = seed, bytearray()
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        out.append(b"ACGT"[x >> 62])
    return bytes(out)


ADAPTER, PHIX = lcg_bases(60, 11), lcg_bases(5386, 19)
FASTA = b">adapter\n" + ADAPTER + b"\n>phix\n" + PHIX + b"\n"


def plant(bases, n, dev):
    """every 100th read: adapter at 100 (100 bases kept: trimmed), at 20 (90 kept: trimmed), at 56 (56 kept: discarded), PhiX at 40"""
    rows = bases[:n * L].view(n, L)
    idx = torch.arange(n, device=dev)
    ad = torch.frombuffer(bytearray(ADAPTER[:40]), dtype=torch.uint8).to(dev)
    for residue, piece, at in ((3, ad, 100), (37, ad, 20), (61, ad, 56)):
        rows[idx % 100 == residue, at:at + 40] = piece
    sel = idx % 100 == 83
    start = (idx[sel] * 7) % (len(PHIX) - 40)
    ph = torch.frombuffer(bytearray(PHIX), dtype=torch.uint8).to(dev)
    rows[sel, 40:80] = ph[start[:, None] + torch.arange(40, device=dev)[None, :]]


def fastq_text(bases, quals, n, dev):
    rec = 1 + NAME + 1 + L + 3 + L + 1
    text = torch.empty((n, rec), dtype=torch.uint8, device=dev)
    text[:, 0] = ord("@"); text[:, 1] = ord("r")
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    for d in range(NAME - 1):
        text[:, 2 + d] = ((idx // 10 ** (NAME - 2 - d)) % 10 + 48).to(torch.uint8)
    c = 1 + NAME
    text[:, c] = 10; text[:, c + 1:c + 1 + L] = bases[:n * L].view(n, L); c += 1 + L
    text[:, c] = 10; text[:, c + 1] = ord("+"); text[:, c + 2] = 10; text[:, c + 3:c + 3 + L] = quals[:n * L].view(n, L); text[:, c + 3 + L] = 10
    return text.view(-1)


def measure(sp, flt, quality, n, dev):
    lib = sp.lib
    bases, quals, offsets = bench.gen_reads(torch, n, 5 * n, 1234, 0, dev, quality)
    plant(bases, n, dev)
    text = fastq_text(bases, quals, n, dev)
    torch.cuda.synchronize()
    del bases, quals, offsets
    r = C.c_void_p()
    rc = lib.kmr_ingest_fastq_dev(sp.h, C.c_void_p(text.data_ptr()), text.numel(), 33, 1, C.byref(r))
    assert rc == 0, lib.kmr_last_error(sp.h)
    r1, r2 = np.arange(0, n, 2, dtype=np.int64), np.arange(1, n, 2, dtype=np.int64)
    mate = np.arange(n, dtype=np.int64) ^ 1
    i64 = C.POINTER(C.c_int64)
    cfg = ka.KmrArtifactReportConfig()
    lib.kmr_artifact_report_config_init(C.byref(cfg))
    stream = torch.cuda.ExternalStream(sp.stream())
    hb, hq = np.zeros(n * L, dtype=np.uint8), np.zeros(n * L, dtype=np.uint8)
    ho, hno, hnl = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    info = {}

    def apply():
        out = C.c_void_p()
        rc = lib.kmr_artifact_filter_apply(sp.h, flt.f, r, mate.ctypes.data_as(i64), None, None, None, None, None, None, C.byref(out))
        assert rc == 0, lib.kmr_last_error(sp.h)
        return lambda: lib.kmr_reads_free(out)

    def apply_report():
        out, rep = C.c_void_p(), C.c_void_p()
        rc = lib.kmr_artifact_filter_apply_report_dev(sp.h, flt.f, r, C.c_void_p(text.data_ptr()), text.numel(), r1.ctypes.data_as(i64), r2.ctypes.data_as(i64), r1.size,
                                                      None, None, None, None, None, None, C.byref(out), None, 0, C.byref(cfg), C.byref(rep))
        assert rc == 0, lib.kmr_last_error(sp.h)
        if not info:
            pk, a, b = C.c_void_p(), C.c_uint64(), C.c_uint64()
            lib.kmr_artifact_report_picks(rep, C.byref(pk)); lib.kmr_picks_info(pk, C.byref(a), C.byref(b))
            rows = flt.n_sequences + 1
            cnt = [np.zeros(rows, dtype=np.uint64) for _ in range(3)]
            lib.kmr_artifact_report_counts(rep, *[x.ctypes.data_as(C.POINTER(C.c_uint64)) for x in cnt], rows)
            info.update(records=a.value, record_bytes=b.value, discarded=int(cnt[0].sum()), trimmed=int(cnt[1].sum()), bases_removed=int(cnt[2].sum()))
        return lambda: (lib.kmr_artifact_report_free(rep), lib.kmr_reads_free(out))

    def reads_copy():
        rc = lib.kmr_reads_copy(r, hb.ctypes.data_as(C.c_void_p), hq.ctypes.data_as(C.c_void_p), ho.ctypes.data_as(C.POINTER(C.c_uint64)),
                                hno.ctypes.data_as(C.POINTER(C.c_uint64)), hnl.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0
        return lambda: None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        done = fn()
        e1.record(stream)
        e1.synchronize()
        done()
        return e0.elapsed_time(e1)

    def report_with(knob):
        def fn():
            sp.tune(artifact_report_lds=knob)
            try:
                return apply_report()
            finally:
                sp.tune(artifact_report_lds=-1)
        return fn

    calls = {"apply": apply, "apply_report": apply_report, "apply_report_global_atomics": report_with(0), "reads_copy": reads_copy}
    times = {k: [] for k in calls}
    for rnd in range(ROUNDS + 1):
        for name in (list(calls) if rnd % 2 == 0 else reversed(list(calls))):
            ms = timed(calls[name])
            if name == "apply_report" and rnd == 0:
                info["default_counters_in_lds"] = int(sp.build_info("artifact_report_lds"))
            if rnd:
                times[name].append(ms)
    lib.kmr_reads_free(r)
    out = dict(info)
    for name, ms in times.items():
        out[name + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
    out["report_over_apply_ms"] = round(out["apply_report_ms"]["median"] - out["apply_ms"]["median"], 3)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "artifact_report.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    n -= n & 1
    dev = torch.device("cuda", 0)
    sp = ka.KmerSpectrum(ka.default_config(bench.K, estimated_raw_kmers=1 << 16, device=0))
    flt = ka.FilterKnownOddities(sp, FASTA, edit_distance=1, phix_idx=2)
    result = {"what": "kmr_artifact_filter_apply_report_dev against kmr_artifact_filter_apply alone and against kmr_reads_copy of the same batch; HIP events on the "
                      "handle's stream around each call, the calls taking turns, one warm-up round, median of %d" % ROUNDS,
              "device": torch.cuda.get_device_name(0), "reads": n, "read_length": L, "filter_sequences": flt.n_sequences, "filter_kmers": flt.n_filter_kmers}
    for quality in ("flat", "noisy"):
        result[quality] = measure(sp, flt, quality, n, dev)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    open(out_path, "w").write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
