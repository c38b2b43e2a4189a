"""development tool: throughput of kmr_ingest_fasta_dev on 16 MiB of FASTA already in device memory, Casava filter idle, in three
layouts -- one record on one line, the same record in 60-column lines, 150-base records of one line each -- with kmr_ingest_fastq_dev
on 16 MiB of FASTQ of 150-base reads in the same run as the yardstick.  HIP events on the handle's stream around each call; the
layouts take turns (forwards and backwards alternately), one warm-up round and five timed ones; the result of every layout is compared with the text once.
usage: python tools/fasta_ingest_bench.py [out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmernator_amd as ka

SIZE, ROUNDS = 16 << 20, 5
rng = np.random.default_rng(7)


def bases(n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]


def lines_of(seq, width):
    """seq in lines of `width`, each ending in a newline"""
    n = seq.size // width * width
    body = np.concatenate([seq[:n].reshape(-1, width), np.full((n // width, 1), 10, dtype=np.uint8)], axis=1).reshape(-1)
    return np.concatenate([body, seq[n:], np.array([10], dtype=np.uint8)]) if seq.size > n else body


def records_of(seq, length, marker, quals=None):
    """records of `length` bases on one line each under headers '>r0000000' ... (with quals: four-line FASTQ records)"""
    n = seq.size // length
    names = np.frombuffer(b"".join(b"%c%08d\n" % (marker, i) for i in range(n)), dtype=np.uint8).reshape(n, 10)
    nl = np.full((n, 1), 10, dtype=np.uint8)
    cols = [names, seq[:n * length].reshape(n, length), nl]
    if quals is not None:
        cols += [np.full((n, 1), ord("+"), dtype=np.uint8), nl, quals[:n * length].reshape(n, length), nl]
    return np.concatenate(cols, axis=1).reshape(-1), n


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fasta_ingest.json")
    sp = ka.KmerSpectrum(ka.default_config(21, estimated_raw_kmers=1 << 16, device=0))
    header = np.frombuffer(b">chr1\n", dtype=np.uint8)
    genome = bases(SIZE - header.size - 1)
    one_line = np.concatenate([header, genome, np.array([10], dtype=np.uint8)])
    columns = np.concatenate([header, lines_of(genome[:(SIZE - header.size) * 60 // 61], 60)])
    reads, n_reads = records_of(bases(SIZE), 150, ord(">"))
    reads = reads[:SIZE // 161 * 161]
    fastq, n_fastq = records_of(bases(SIZE), 150, ord("@"), (rng.integers(2, 41, size=SIZE) + 33).astype(np.uint8))
    fastq = fastq[:SIZE // 314 * 314]
    layouts = {"fasta_one_line": one_line, "fasta_60_columns": columns, "fasta_150_base_records": reads, "fastq_150_base_reads": fastq}
    stream = torch.cuda.ExternalStream(sp.stream())
    dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in layouts.items()}
    torch.cuda.synchronize()

    def call(name):
        r = C.c_void_p()
        t = dev[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if name.startswith("fastq"):
            rc = sp.lib.kmr_ingest_fastq_dev(sp.h, C.c_void_p(t.data_ptr()), t.numel(), 0, 1, C.byref(r))
        else:
            rc = sp.lib.kmr_ingest_fasta_dev(sp.h, C.c_void_p(t.data_ptr()), t.numel(), None, 0, 1, C.byref(r))
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, sp.lib.kmr_last_error(sp.h)
        return r, e0.elapsed_time(e1)

    # once: the result is the text's
    for name, text in layouts.items():
        r, _ = call(name)
        n, tot = C.c_uint64(), C.c_uint64()
        sp.lib.kmr_reads_info(r, C.byref(n), C.byref(tot), None, None)
        b = np.zeros(tot.value, dtype=np.uint8)
        sp.lib.kmr_reads_copy(r, b.ctypes.data_as(C.c_void_p), None, None, None, None)
        sp.lib.kmr_reads_free(r)
        raw = text.tobytes()
        if name.startswith("fastq"):
            want = b"".join(raw.split(b"\n")[1::4])
        else:
            want = b"".join(l for l in raw.split(b"\n") if not l.startswith(b">"))
        assert b.tobytes() == want, name
        print("%s: %d bytes, %d records, %d bases: equal to the text" % (name, text.size, n.value, tot.value), flush=True)
    times = {k: [] for k in layouts}
    for rnd in range(ROUNDS + 1):
        for name in (list(layouts) if rnd % 2 == 0 else reversed(list(layouts))):          # forwards and backwards in turn: no layout always follows the same one
            r, ms = call(name)
            sp.lib.kmr_reads_free(r)
            if rnd:
                times[name].append(ms)
    result = {"what": "kmr_ingest_fasta_dev / kmr_ingest_fastq_dev on text in device memory, HIP events on the handle's stream around the call, "
                      "layouts taking turns forwards and backwards, one warm-up round, GB/s = text bytes / time", "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "layouts": {}}
    for name, ms in times.items():
        size = int(layouts[name].size)
        gbs = sorted(size / (t * 1e-3) / 1e9 for t in ms)
        result["layouts"][name] = {"text_bytes": size, "ms": [round(t, 4) for t in ms], "ms_median": round(float(np.median(ms)), 4),
                                   "gb_per_s_median": round(gbs[len(gbs) // 2], 2), "gb_per_s_min": round(gbs[0], 2), "gb_per_s_max": round(gbs[-1], 2)}
        print(name, result["layouts"][name], flush=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
