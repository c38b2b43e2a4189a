"""Shared test plumbing: ctypes bindings for the oracle (oracle/libkmr_oracle.so)
and the product C-ABI (kmernator_amd/csrc/libkmernator_amd.so), a FASTQ reader and
the synthetic read generator described in SURVEY.md section 8(d).

The oracle is test infrastructure: it is loaded here, by __graft_entry__.smoke()
and by bench.py's cpu_baseline leg only.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "libkmr_oracle.so")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libref_lookup3.so")
PRODUCT_SO = os.path.join(ROOT, "kmernator_amd", "csrc", "libkmernator_amd.so")

KMR_VALUE_COUNT_DIR, KMR_VALUE_EXT = 0, 1
KMR_HASH_LOOKUP3, KMR_HASH_LOOKUP8 = 0, 1
KMR_MAP_WEAK, KMR_MAP_SINGLETON, KMR_MAP_SOLID = 0, 1, 2


class KmrConfig(C.Structure):
    """Mirror of kmr_config in include/kmernator_amd.h."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("k", C.c_uint32),
        ("num_buckets_weak", C.c_uint64), ("num_buckets_singleton", C.c_uint64),
        ("estimated_raw_kmers", C.c_uint64),
        ("value_kind", C.c_uint32), ("min_weight", C.c_float),
        ("min_quality_score", C.c_uint32), ("fastq_start_char", C.c_uint32),
        ("ext_min_quality", C.c_uint32), ("separate_singletons", C.c_uint32),
        ("kmer_subsample", C.c_uint32), ("device", C.c_int32),
        ("rank", C.c_uint32), ("world_size", C.c_uint32),
        ("estimated_depth", C.c_double), ("estimated_error_rate", C.c_double),
        ("kmers_per_bucket", C.c_uint32), ("num_parts", C.c_uint32),
        ("part_idx", C.c_uint32), ("build_mode", C.c_uint32),
        ("max_table_entries", C.c_uint64),
        ("hash_kind", C.c_uint32), ("size_tracker", C.c_uint32),
    ]


class KmrStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "raw_kmers", "raw_good_kmers", "unique_kmers", "singleton_kmers",
        "discarded", "weak_entries", "singleton_entries", "reads")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class KmrDigest(C.Structure):
    """Mirror of kmr_digest in include/kmernator_amd.h."""
    _fields_ = [(n, C.c_uint64) for n in ("entries", "count_sum", "dir_sum", "hash_sum", "hash_xor")] + [("weighted_sum", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KmrArtifactConfig(C.Structure):
    """Mirror of kmr_artifact_config in include/kmernator_amd.h."""
    _fields_ = [(n, C.c_uint32) for n in ("match_length", "edit_distance", "build_edits", "simple_repeat_begin", "simple_repeat_end",
                                          "phix_idx", "reference_begin", "min_quality", "fastq_start_char")] + [("min_read_length", C.c_float)]


def artifact_config(**kw):
    """the reference's defaults (FilterKnownOdditiesOptions, src/FilterKnownOddities.h:72-74; ReadSelectorOptions min-read-length)"""
    c = KmrArtifactConfig(24, 2, 2, 0, 0, 0, 0, 3, 33, 0.40)
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def default_config(k, **kw):
    c = KmrConfig()
    c.struct_size = C.sizeof(KmrConfig)
    c.k = k
    c.value_kind = KMR_VALUE_COUNT_DIR
    c.min_weight = 0.10
    c.min_quality_score = 3
    c.fastq_start_char = 33
    c.ext_min_quality = 20
    c.separate_singletons = 1
    c.kmer_subsample = 1
    c.device = -1
    c.rank = 0
    c.world_size = 1
    c.estimated_depth = 20.0
    c.estimated_error_rate = 0.35
    c.kmers_per_bucket = 32
    c.num_parts = 1
    c.part_idx = 0
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def build_oracle():
    if os.environ.get("KMR_ORACLE_SO"):      # a build of the oracle made elsewhere (the sanitizer run: oracle compiled with -fsanitize=address,undefined)
        return os.environ["KMR_ORACLE_SO"]
    if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(
            os.path.join(ORACLE_DIR, "kmr_oracle.cpp")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])
    return ORACLE_SO


_oracle = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(build_oracle())
        u8p, u32p, u64p, f32p, f64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float, C.c_double))
        lib.orc_create.restype = C.c_void_p
        lib.orc_create.argtypes = [C.POINTER(KmrConfig)]
        lib.orc_destroy.argtypes = [C.c_void_p]
        lib.orc_add_reads.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, u64p, C.c_uint64, C.c_uint64, u8p, C.c_int]
        lib.orc_finalize.argtypes = [C.c_void_p, C.c_uint32]
        lib.orc_get_stats.argtypes = [C.c_void_p, C.POINTER(KmrStats)]
        lib.orc_num_buckets.argtypes = [C.c_void_p, C.c_int, u64p]
        lib.orc_lookup.argtypes = [C.c_void_p, u8p, C.c_uint64, u32p]
        lib.orc_image_size.argtypes = [C.c_void_p, C.c_int, u64p]
        lib.orc_write_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
        lib.orc_load_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
        lib.orc_count_histogram.argtypes = [C.c_void_p, u64p, f64p, C.c_uint32]
        lib.orc_dump.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_int]
        lib.orc_export_entries.restype = C.c_uint64
        lib.orc_export_entries.argtypes = [C.c_void_p, u8p, u32p, u32p, f32p, u32p, C.c_uint64]
        lib.orc_quality_table.argtypes = [C.c_uint, C.c_uint, f64p]
        lib.orc_hash.restype = C.c_uint64
        lib.orc_hash.argtypes = [C.c_char_p, C.c_uint32]
        lib.orc_hashlittle2.argtypes = [C.c_char_p, C.c_uint64, u32p, u32p]
        lib.orc_size_tracker.restype = C.c_uint64
        lib.orc_size_tracker.argtypes = [C.c_void_p, C.c_int, C.c_int, u64p, C.c_uint64]
        lib.orc_hash8.restype = C.c_uint64
        lib.orc_hash8.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
        lib.orc_hash8_words.restype = C.c_uint64
        lib.orc_hash8_words.argtypes = [u64p, C.c_uint64, C.c_uint64]
        lib.orc_compress_sequence.restype = C.c_int64
        lib.orc_compress_sequence.argtypes = [C.c_char_p, C.c_uint64, u8p, u32p, C.c_char_p, C.c_uint64]
        lib.orc_reverse_complement.argtypes = [u8p, u8p, C.c_uint32]
        lib.orc_shift_left.argtypes = [u8p, u8p, C.c_uint32, C.c_uint32, C.c_int]
        lib.orc_least_complement.argtypes = [u8p, C.c_uint32, u8p]
        lib.orc_build_weighted_kmers.restype = C.c_int64
        lib.orc_build_weighted_kmers.argtypes = [C.POINTER(KmrConfig), C.c_char_p, C.c_char_p, C.c_uint32, u8p, f32p, u8p, C.c_uint64]
        lib.orc_bucket_idx.restype = C.c_uint64
        lib.orc_bucket_idx.argtypes = [C.c_uint64, C.c_uint64]
        lib.orc_local_thread_id.restype = C.c_uint32
        lib.orc_local_thread_id.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        lib.orc_distributed_thread_id.restype = C.c_uint32
        lib.orc_distributed_thread_id.argtypes = [C.c_uint64, C.c_uint32]
        lib.orc_min_power_of_2.restype = C.c_uint64
        lib.orc_min_power_of_2.argtypes = [C.c_uint64]
        lib.orc_extract_records_by_owner.restype = C.c_int64
        lib.orc_extract_records_by_owner.argtypes = [C.POINTER(KmrConfig), C.c_char_p, C.c_char_p, u64p, C.c_uint64, u8p, u8p, C.c_uint64, u64p]
        lib.orc_insert_records.argtypes = [C.c_void_p, u8p, C.c_uint64]
        lib.orc_derive_buckets.argtypes = [C.POINTER(KmrConfig), u64p, u64p]
        lib.orc_histogram.argtypes = [C.c_void_p, C.c_uint32, C.c_double, u64p, u64p, f64p]
        lib.orc_subtract_reference.argtypes = [C.c_void_p, C.c_void_p]
        lib.orc_subtracted.restype = C.c_uint64
        lib.orc_subtracted.argtypes = [C.c_void_p]
        lib.orc_parse_fastq.restype = C.c_int64
        lib.orc_parse_fastq.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, u64p, u64p, u32p,
                                        C.c_uint64, C.c_uint64, u32p]
        lib.orc_map_digest.argtypes = [C.c_void_p, C.c_int, C.POINTER(KmrDigest)]
        lib.orc_merge_add.argtypes = [C.c_void_p, C.c_void_p]
        lib.orc_synth_reads.restype = None
        lib.orc_synth_reads.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, u64p, C.c_int]
        _oracle = lib
    return _oracle


class OracleArtifactFilter:
    """oracle restatement of FilterKnownOddities (f4)"""

    def __init__(self, cfg, fasta):
        lib = oracle_lib()
        lib.orc_artifact_create.restype = C.c_void_p
        lib.orc_artifact_create.argtypes = [C.POINTER(KmrArtifactConfig), C.c_char_p, C.c_uint64]
        lib.orc_artifact_free.argtypes = [C.c_void_p]
        lib.orc_artifact_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        lib.orc_artifact_entries.restype = C.c_uint64
        lib.orc_artifact_entries.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint64]
        lib.orc_artifact_apply.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_int64)] + \
            [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_uint8)] + [C.POINTER(C.c_uint32)] * 2
        self.lib = lib
        self.cfg = cfg
        fasta = bytes(fasta)
        self.h = lib.orc_artifact_create(C.byref(cfg), fasta, len(fasta))
        assert self.h

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self.lib.orc_artifact_info(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def entries(self):
        n = self.info()[1]
        keys = np.zeros(n, dtype=np.uint64)
        vals = np.zeros(n, dtype=np.uint32)
        assert self.lib.orc_artifact_entries(self.h, _ptr(keys, C.c_uint64), _ptr(vals, C.c_uint32), n) == n
        return keys, vals

    def apply(self, rb, mate=None):
        """dict of per-read arrays: value, min_pass, max_pass, action, remnant_off, remnant_len"""
        n = rb.n
        out = {k: np.zeros(n, dtype=np.uint32) for k in ("value", "min_pass", "max_pass", "remnant_off", "remnant_len")}
        out["action"] = np.zeros(n, dtype=np.uint8)
        m = None if mate is None else _ptr(np.ascontiguousarray(mate, dtype=np.int64), C.c_int64)
        self.lib.orc_artifact_apply(self.h, rb.bases.ctypes.data_as(C.c_char_p), rb.quals.ctypes.data_as(C.c_char_p), _ptr(rb.offsets, C.c_uint64), n, m,
                                    _ptr(out["value"], C.c_uint32), _ptr(out["min_pass"], C.c_uint32), _ptr(out["max_pass"], C.c_uint32),
                                    _ptr(out["action"], C.c_uint8), _ptr(out["remnant_off"], C.c_uint32), _ptr(out["remnant_len"], C.c_uint32))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.orc_artifact_free(self.h)
            self.h = None


def apply_artifact_result(rb, res):
    """the read set after applyFilter: trimmed / emptied reads in place, remnants appended (host-side model for the tests)"""
    seqs, quals = [], []
    for i in range(rb.n):
        s, q = rb.seq(i), rb.qual(i)
        a = int(res["action"][i])
        if a == 1:
            s, q = s[int(res["min_pass"][i]):int(res["max_pass"][i])], q[int(res["min_pass"][i]):int(res["max_pass"][i])]
        elif a == 2:
            s, q = b"", b""
        seqs.append(s)
        quals.append(q)
    for i in range(rb.n):
        if res["remnant_len"][i]:
            o, l = int(res["remnant_off"][i]), int(res["remnant_len"][i])
            seqs.append(rb.seq(i)[o:o + l])
            quals.append(rb.qual(i)[o:o + l])
    return ReadBatch(seqs, quals)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class ReadBatch:
    """Flat read arrays in the layout kmr_add_reads takes."""

    def __init__(self, seqs, quals=None, discarded=None):
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        self.offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=self.offsets[1:])
        self.bases = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if len(seqs) else np.zeros(0, np.uint8)
        self.quals = None
        if quals is not None:
            self.quals = np.frombuffer(b"".join(quals), dtype=np.uint8).copy() if len(quals) else np.zeros(0, np.uint8)
            assert self.quals.size == self.bases.size
        self.discarded = None if discarded is None else np.asarray(discarded, dtype=np.uint8)
        self.n = len(seqs)

    @classmethod
    def from_arrays(cls, bases, quals, offsets):
        self = cls.__new__(cls)
        self.bases, self.quals, self.offsets = bases, quals, offsets
        self.discarded = None
        self.n = len(offsets) - 1
        return self

    def slice(self, lo, hi):
        b0, b1 = int(self.offsets[lo]), int(self.offsets[hi])
        out = ReadBatch.__new__(ReadBatch)
        out.offsets = (self.offsets[lo:hi + 1] - self.offsets[lo]).copy()
        out.bases = self.bases[b0:b1].copy()
        out.quals = None if self.quals is None else self.quals[b0:b1].copy()
        out.discarded = None if self.discarded is None else self.discarded[lo:hi].copy()
        out.n = hi - lo
        return out

    def seq(self, i):
        return self.bases[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()

    def qual(self, i):
        return self.quals[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()


def read_fastq(path):
    seqs, quals, names = [], [], []
    with open(path, "rb") as f:
        while True:
            name = f.readline()
            if not name:
                break
            seq = f.readline().rstrip(b"\r\n")
            f.readline()
            q = f.readline().rstrip(b"\r\n")
            names.append(name.rstrip(b"\r\n")[1:])
            seqs.append(seq)
            quals.append(q)
    rb = ReadBatch(seqs, quals)
    rb.names = names
    return rb


class _SpectrumCommon:
    """Method set shared by the oracle and the product wrappers so parity tests
    drive both with the same code."""

    def stats(self):
        s = KmrStats()
        self._call("get_stats", self.h, C.byref(s))
        return s.as_dict()

    def num_buckets(self, which):
        v = C.c_uint64()
        self._call("num_buckets", self.h, which, C.byref(v))
        return v.value

    def finalize(self, min_depth=2):
        self._call("finalize", self.h, min_depth)

    def lookup(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        n = keys.size // self.kb
        out = np.zeros(n, dtype=np.uint32)
        if n:
            self._call("lookup", self.h, _ptr(keys, C.c_uint8), n, _ptr(out, C.c_uint32))
        return out

    def image(self, which=KMR_MAP_WEAK):
        sz = C.c_uint64()
        self._call("image_size", self.h, which, C.byref(sz))
        buf = np.zeros(sz.value, dtype=np.uint8)
        self._call("write_image", self.h, which, buf.ctypes.data_as(C.c_void_p), sz.value)
        return buf

    def load_image(self, which, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._call("load_image", self.h, which, buf.ctypes.data_as(C.c_void_p), buf.size)

    def histogram(self, nbins=256):
        counts = np.zeros(nbins, dtype=np.uint64)
        weights = np.zeros(nbins, dtype=np.float64)
        self._call("count_histogram", self.h, _ptr(counts, C.c_uint64), _ptr(weights, C.c_double), nbins)
        return counts, weights


class OracleSpectrum(_SpectrumCommon):
    def __init__(self, cfg):
        self.lib = oracle_lib()
        self.cfg = cfg
        self.k = cfg.k
        self.kb = (cfg.k + 3) // 4
        self.h = self.lib.orc_create(C.byref(cfg))
        assert self.h

    def _call(self, name, *a):
        rc = getattr(self.lib, "orc_" + name)(*a)
        if rc != 0:
            raise RuntimeError("orc_%s -> %d" % (name, rc))

    def add_reads(self, rb, first_idx=0, threads=1):
        self._call("add_reads", self.h, rb.bases.ctypes.data_as(C.c_char_p),
                   None if rb.quals is None else rb.quals.ctypes.data_as(C.c_char_p),
                   _ptr(rb.offsets, C.c_uint64), rb.n, first_idx,
                   None if rb.discarded is None else _ptr(rb.discarded, C.c_uint8), threads)

    def insert_records(self, recs, n):
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        self._call("insert_records", self.h, _ptr(recs, C.c_uint8), n)

    def size_tracker(self, per_read=True, force_last=True):
        """the size history: the reference's own sampling (before every k-mer) or after every read; [n][4] uint64"""
        lib = oracle_lib()
        n = lib.orc_size_tracker(self.h, 1 if per_read else 0, 1 if force_last else 0, None, 0)
        el = np.zeros((n, 4), dtype=np.uint64)
        if n:
            lib.orc_size_tracker(self.h, 1 if per_read else 0, 1 if force_last else 0, el.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        return el

    def ref_histogram(self, zoom_max=256, log_base=2.0):
        nb = (1 << 16) + 2 + zoom_max
        v, c, w = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.float64)
        self._call("histogram", self.h, zoom_max, log_base, _ptr(v, C.c_uint64), _ptr(c, C.c_uint64), _ptr(w, C.c_double))
        return v, c, w

    def dump(self, path, min_depth, graph):
        self._call("dump", self.h, path.encode(), min_depth, 1 if graph else 0)

    def merge_add(self, other):
        """KmerMapByKmerArrayPair::mergeAdd of the weak maps (other's weak map is emptied)"""
        self._call("merge_add", self.h, other.h)

    def digest(self, which=KMR_MAP_WEAK):
        d = KmrDigest()
        self._call("map_digest", self.h, which, C.byref(d))
        return d.as_dict()

    def entries(self):
        n = self.stats()["weak_entries"]
        keys = np.zeros(n * self.kb, dtype=np.uint8)
        count = np.zeros(n, dtype=np.uint32)
        dirb = np.zeros(n, dtype=np.uint32)
        w = np.zeros(n, dtype=np.float32)
        ext = np.zeros(n * 12, dtype=np.uint32)
        got = self.lib.orc_export_entries(self.h, _ptr(keys, C.c_uint8), _ptr(count, C.c_uint32), _ptr(dirb, C.c_uint32),
                                          _ptr(w, C.c_float), _ptr(ext, C.c_uint32), n)
        assert got == n
        return keys.reshape(n, self.kb), count, dirb, w, ext.reshape(n, 12)

    def close(self):
        if self.h:
            self.lib.orc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def oracle_weighted_kmers(cfg, seq, qual):
    lib = oracle_lib()
    kb = (cfg.k + 3) // 4
    n = max(0, len(seq) - cfg.k + 1)
    keys = np.zeros(max(n, 1) * kb, dtype=np.uint8)
    w = np.zeros(max(n, 1), dtype=np.float32)
    ext = np.zeros(max(n, 1) * 4, dtype=np.uint8)
    got = lib.orc_build_weighted_kmers(C.byref(cfg), seq, qual, len(seq), _ptr(keys, C.c_uint8), _ptr(w, C.c_float),
                                       _ptr(ext, C.c_uint8), max(n, 1))
    assert got == n, (got, n)
    return keys[:n * kb].reshape(n, kb), w[:n], ext[:n * 4].reshape(n, 4)


# ---------------------------------------------------------------- synthetic reads
def synth_reads(n_reads, read_len=150, genome_len=None, seed=1, err=0.01, quality="flat", n_rate=0.0):
    """Synthetic reads per SURVEY.md 8(d): uniform random genome, uniform start, random
    strand, per-base substitution with probability err, Phred-33 quals.  quality:
    'flat' ('I' everywhere) or 'noisy' (Q in {40,30,20,10,2} with probs
    {.80,.10,.05,.04,.01}, substituted bases forced to Q10).  n_rate adds N bases."""
    rng = np.random.default_rng(seed)
    if genome_len is None:
        genome_len = max(read_len * 2, n_reads * read_len // 30)
    genome = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - read_len + 1, size=n_reads)
    idx = starts[:, None] + np.arange(read_len)[None, :]
    codes = genome[idx]
    strand = rng.integers(0, 2, size=n_reads).astype(bool)
    codes[strand] = (3 - codes[strand])[:, ::-1]
    errs = rng.random(codes.shape) < err
    shift = rng.integers(1, 4, size=codes.shape, dtype=np.uint8)
    codes = np.where(errs, (codes + shift) & 3, codes).astype(np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    bases = lut[codes]
    if quality == "flat":
        quals = np.full(codes.shape, ord("I"), dtype=np.uint8)
    else:
        qv = np.array([40, 30, 20, 10, 2], dtype=np.uint8)
        pick = rng.choice(5, size=codes.shape, p=[0.80, 0.10, 0.05, 0.04, 0.01])
        quals = (qv[pick] + 33).astype(np.uint8)
        quals[errs] = 10 + 33
    if n_rate > 0:
        ns = rng.random(codes.shape) < n_rate
        bases = np.where(ns, ord("N"), bases).astype(np.uint8)
        quals = np.where(ns, 33 + 2, quals).astype(np.uint8)
    offsets = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len))
    return ReadBatch.from_arrays(np.ascontiguousarray(bases.reshape(-1)), np.ascontiguousarray(quals.reshape(-1)), offsets)


def noisy_ragged_reads(k, n, seed):
    """synth_reads with noisy qualities and a few N, a quarter of the reads cut to k .. read length bases and one in twenty to fewer
    than k + 3 (some shorter than k, some empty)"""
    rl = max(100, k + 40)
    rb = synth_reads(n, read_len=rl, seed=seed, quality="noisy", n_rate=0.003)
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for i in range(rb.n):
        L = rl
        r = rng.random()
        if r < 0.05:
            L = int(rng.integers(0, k + 3))        # shorter than k, some empty
        elif r < 0.3:
            L = int(rng.integers(k, rl + 1))
        seqs.append(rb.seq(i)[:L])
        quals.append(rb.qual(i)[:L])
    return ReadBatch(seqs, quals)


def synth_reads_8d(seed, first_read, n_reads, read_len=150, genome_len=None, noisy=False, threads=8):
    """SURVEY.md 8(d)'s generator, CPU statement (orc_synth_reads): the same bytes as kmr_synth_reads_dev for the same arguments"""
    lib = oracle_lib()
    bases = np.zeros(n_reads * read_len, dtype=np.uint8)
    quals = np.zeros(n_reads * read_len, dtype=np.uint8)
    offsets = np.zeros(n_reads + 1, dtype=np.uint64)
    lib.orc_synth_reads(seed, first_read, n_reads, read_len, genome_len, 1 if noisy else 0, bases.ctypes.data_as(C.c_void_p),
                        quals.ctypes.data_as(C.c_void_p), _ptr(offsets, C.c_uint64), threads)
    return ReadBatch.from_arrays(bases, quals, offsets)


def parse_image(buf, kb, vsize):
    """Decode the reference on-disk map layout (src/Kmer.h:3143-3159) into
    (num_buckets, mask, [(keys[n,kb], values[n,vsize])...])."""
    hdr = np.frombuffer(buf[:16].tobytes(), dtype=np.uint64)
    nb, mask = int(hdr[0]), int(hdr[1])
    offs = np.frombuffer(buf[16:16 + 8 * nb].tobytes(), dtype=np.uint64)
    buckets = []
    for i in range(nb):
        o = int(offs[i])
        n = int(np.frombuffer(buf[o:o + 4].tobytes(), dtype=np.uint32)[0])
        keys = buf[o + 4:o + 4 + n * kb].reshape(n, kb)
        vals = buf[o + 4 + n * kb:o + 4 + n * (kb + vsize)].reshape(n, vsize)
        buckets.append((keys, vals))
    return nb, mask, buckets


def _dmix(x):
    """mix() of include/kmernator_amd.h's digest, on uint64 arrays"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def digest_of_image(buf, kb, ext=False, singleton=False):
    """kmr_digest as include/kmernator_amd.h defines it, computed from the bytes of a stored map (numpy restatement: what
    kmr_map_digest and orc_map_digest are both held to)"""
    vsize = (5 if ext else 1) if singleton else (60 if ext else 12)
    _, _, buckets = parse_image(buf, kb, vsize)
    keys = np.concatenate([b[0] for b in buckets]) if buckets else np.zeros((0, kb), np.uint8)
    vals = np.concatenate([b[1] for b in buckets]) if buckets else np.zeros((0, vsize), np.uint8)
    n = keys.shape[0]
    W = (kb + 7) // 8
    padded = np.zeros((n, 8 * W), dtype=np.uint8)
    padded[:, :kb] = keys
    words = padded.reshape(n, W, 8)[:, :, ::-1].copy().view(np.uint64).reshape(n, W)      # big-endian words
    out = {"entries": n}
    if singleton:
        w8 = vals[:, 0].astype(np.uint64)
        x = np.uint64(1 << 32) | w8
        if ext:
            x = x | (np.ascontiguousarray(vals[:, 1:5]).view(np.uint32).reshape(n).astype(np.uint64) << np.uint64(40))
        out["count_sum"] = int((w8 != 0).sum())
        out["dir_sum"] = 0
        out["weighted_sum"] = float(np.where(w8 != 0, (w8.astype(np.float64) - 1.0) / 254.0, 0.0).sum())
    else:
        count = np.ascontiguousarray(vals[:, 0:2]).view(np.uint16).reshape(n).astype(np.uint64)
        dirb = np.ascontiguousarray(vals[:, 8:10]).view(np.uint16).reshape(n).astype(np.uint64)
        x = count | (dirb << np.uint64(16))
        out["count_sum"] = int(count.sum())
        out["dir_sum"] = int(dirb.sum())
        out["weighted_sum"] = float(np.ascontiguousarray(vals[:, 4:8]).view(np.float32).reshape(n).astype(np.float64).sum())
    for j in range(W):
        x = _dmix(x ^ words[:, j])
    if ext and not singleton:
        t = np.ascontiguousarray(vals[:, 12:60]).view(np.uint32).reshape(n, 12).astype(np.uint64)
        for j in range(0, 12, 2):
            x = _dmix(x ^ (t[:, j] | (t[:, j + 1] << np.uint64(32))))
    with np.errstate(over="ignore"):
        out["hash_sum"] = int(x.sum(dtype=np.uint64)) if n else 0
    out["hash_xor"] = int(np.bitwise_xor.reduce(x)) if n else 0
    return out


def digests_agree(a, b, rel=1e-6):
    """two kmr_digests: integers equal, weighted_sum within rel (a float accumulation whose order is not part of the contract)"""
    for key in ("entries", "count_sum", "dir_sum", "hash_sum", "hash_xor"):
        if int(a[key]) != int(b[key]):
            return False
    return abs(a["weighted_sum"] - b["weighted_sum"]) <= rel * max(1.0, abs(a["weighted_sum"]))


def add_digests(a, b):
    """part / rank digests combine into the whole map's (a may be None)"""
    if a is None:
        return dict(b)
    out = {key: a[key] + b[key] for key in ("entries", "count_sum", "dir_sum", "weighted_sum")}
    out["hash_sum"] = (a["hash_sum"] + b["hash_sum"]) & 0xFFFFFFFFFFFFFFFF
    out["hash_xor"] = a["hash_xor"] ^ b["hash_xor"]
    return out


def full_size_golden(name):
    """tests/golden/full_size_digests.json[name] (written by tests/golden/make_full_size_digests.py from the oracle)"""
    import json
    with open(os.path.join(GOLDEN, "full_size_digests.json")) as f:
        return dict(json.load(f)[name], name=name)


def oracle_extract_by_owner(cfg, rb, seg_capacity):
    """(records uint8 [world*seg_capacity*rec_bytes], counts uint64 [world])"""
    lib = oracle_lib()
    W = (((cfg.k + 3) // 4) + 7) // 8
    recb = 8 * W + (8 if cfg.value_kind == KMR_VALUE_EXT else 4)
    recs = np.zeros(cfg.world_size * seg_capacity * recb, dtype=np.uint8)
    counts = np.zeros(cfg.world_size, dtype=np.uint64)
    n = lib.orc_extract_records_by_owner(C.byref(cfg), rb.bases.ctypes.data_as(C.c_char_p),
                                         None if rb.quals is None else rb.quals.ctypes.data_as(C.c_char_p),
                                         _ptr(rb.offsets, C.c_uint64), rb.n,
                                         None if rb.discarded is None else _ptr(rb.discarded, C.c_uint8),
                                         _ptr(recs, C.c_uint8), seg_capacity, _ptr(counts, C.c_uint64))
    assert n >= 0
    return recs, counts


def oracle_parse_fastq(text, start_char=33, input_base=33, store_comment=True):
    """oracle restatement of the reference's FASTQ stream parser: (ReadBatch with .names, final input base) or None
    where the reference throws"""
    lib = oracle_lib()
    text = bytes(text)
    cap_reads = text.count(b"\n") // 4 + 2
    bases = np.zeros(len(text) + 1, dtype=np.uint8)
    quals = np.zeros(len(text) + 1, dtype=np.uint8)
    offsets = np.zeros(cap_reads + 1, dtype=np.uint64)
    noff = np.zeros(cap_reads, dtype=np.uint64)
    nlen = np.zeros(cap_reads, dtype=np.uint32)
    fb = C.c_uint32()
    n = lib.orc_parse_fastq(text, len(text), start_char, input_base, 1 if store_comment else 0, bases.ctypes.data_as(C.c_void_p),
                            quals.ctypes.data_as(C.c_void_p), _ptr(offsets, C.c_uint64), _ptr(noff, C.c_uint64), _ptr(nlen, C.c_uint32),
                            cap_reads, len(text), C.byref(fb))
    if n < 0:
        return None
    tot = int(offsets[n])
    rb = ReadBatch.from_arrays(bases[:tot].copy(), quals[:tot].copy(), offsets[:n + 1].copy())
    rb.names = [text[int(noff[i]):int(noff[i]) + int(nlen[i])] for i in range(n)]
    return rb, fb.value


# ---------------------------------------------------------------- weight profiles
# weightedCount is a float sum whose order of addition the reference does not fix, so the map digest above leaves it out and
# sums it over the whole map, where per-entry errors vanish in the slack.  A weight profile holds it per key-hash bin and per
# sampled entry instead (tests/golden/full_size_weights.npz, written by tests/golden/make_full_size_weights.py).
PROFILE_BINS = 2048          # chosen by the top 11 bits of key_mix
PROFILE_SAMPLE = 2048        # the entries whose keys mix to the smallest values
_BIN_SHIFT = np.uint64(64 - 11)


def key_words(keys):
    """packed keys [n, kb] -> big-endian uint64 words [n, W], zero padded (the word layout of digest_of_image)"""
    n, kb = keys.shape
    W = (kb + 7) // 8
    padded = np.zeros((n, 8 * W), dtype=np.uint8)
    padded[:, :kb] = keys
    return padded.reshape(n, W, 8)[:, :, ::-1].copy().view(np.uint64).reshape(n, W)


def key_mix(keys):
    """x = 0; x = _dmix(x ^ word) over the key's big-endian words: depends on the key alone"""
    words = key_words(np.asarray(keys, dtype=np.uint8))
    x = np.zeros(words.shape[0], dtype=np.uint64)
    for j in range(words.shape[1]):
        x = _dmix(x ^ words[:, j])
    return x


def profile_bin(x):
    """the bin of a key_mix value: its top 11 bits"""
    return (x >> _BIN_SHIFT).astype(np.int64)


def empty_profile(kb):
    return {"entries": np.zeros(PROFILE_BINS, np.int64), "count_sum": np.zeros(PROFILE_BINS, np.int64),
            "wsum": np.zeros(PROFILE_BINS, np.float64), "nwsum": np.zeros(PROFILE_BINS, np.float64),
            "sample_keys": np.zeros((0, kb), np.uint8), "sample_count": np.zeros(0, np.uint32), "sample_w": np.zeros(0, np.float32)}


def _profile_piece(keys, counts, weights):
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    counts = np.asarray(counts).astype(np.int64)
    w = np.asarray(weights, dtype=np.float32)
    x = key_mix(keys)
    b = profile_bin(x)
    w64 = w.astype(np.float64)
    p = {"entries": np.bincount(b, minlength=PROFILE_BINS).astype(np.int64),
         "count_sum": np.bincount(b, weights=counts, minlength=PROFILE_BINS).astype(np.int64),
         "wsum": np.bincount(b, weights=w64, minlength=PROFILE_BINS),
         "nwsum": np.bincount(b, weights=(counts + 2) * w64, minlength=PROFILE_BINS)}
    take = np.argpartition(x, PROFILE_SAMPLE)[:PROFILE_SAMPLE] if x.size > PROFILE_SAMPLE else np.arange(x.size)
    take = take[np.argsort(x[take], kind="stable")]
    p.update(sample_keys=keys[take], sample_count=counts[take].astype(np.uint32), sample_w=w[take])
    return p


def add_profiles(a, b):
    """profiles of disjoint key sets (parts, pieces of an image) combine into the union's: bins add, samples merge by smallest key_mix"""
    out = {key: a[key] + b[key] for key in ("entries", "count_sum", "wsum", "nwsum")}
    keys = np.concatenate([a["sample_keys"], b["sample_keys"]])
    take = np.argsort(key_mix(keys), kind="stable")[:PROFILE_SAMPLE]
    out["sample_keys"] = keys[take]
    out["sample_count"] = np.concatenate([a["sample_count"], b["sample_count"]])[take]
    out["sample_w"] = np.concatenate([a["sample_w"], b["sample_w"]])[take]
    return out


def weight_profile(keys, counts, weights):
    """the weight profile of a weak map given as entries (OracleSpectrum.entries(): keys [n, kb], counts, f32 weightedCount)"""
    return add_profiles(empty_profile(keys.shape[1]), _profile_piece(keys, counts, weights))


def image_pieces(buf, kb, vsize, cols=None, buckets_per_piece=1 << 16):
    """(keys [m, kb], values [m, cols]) of a stored map (parse_image's layout), a run of buckets at a time, without a Python loop
    over buckets: what parse_image gives, for images of any size at a few hundred MB of working memory"""
    cols = vsize if cols is None else cols
    buf = np.asarray(buf, dtype=np.uint8)
    nb = int(buf[:8].view(np.uint64)[0])
    offs = buf[16:16 + 8 * nb].view(np.uint64).astype(np.int64)
    for lo in range(0, nb, buckets_per_piece):
        o = offs[lo:lo + buckets_per_piece]
        n = buf[o[:, None] + np.arange(4)].copy().view(np.uint32).reshape(-1).astype(np.int64)
        m = int(n.sum())
        if m == 0:
            continue
        bi = np.repeat(np.arange(o.size), n)
        i = np.arange(m) - np.repeat(np.cumsum(n) - n, n)
        kstart = o[bi] + 4 + i * kb
        vstart = o[bi] + 4 + n[bi] * kb + i * vsize
        yield buf[kstart[:, None] + np.arange(kb)], buf[vstart[:, None] + np.arange(cols)]


def weight_profile_of_image(buf, kb, ext=False, buckets_per_piece=1 << 16):
    """the weight profile of a weak map from the bytes of its stored image (12- or 60-byte values: count u16 at 0, f32 at 4)"""
    vsize = 60 if ext else 12
    prof = empty_profile(kb)
    for keys, vals in image_pieces(buf, kb, vsize, cols=8, buckets_per_piece=buckets_per_piece):
        counts = np.ascontiguousarray(vals[:, 0:2]).view(np.uint16).reshape(-1)
        w = np.ascontiguousarray(vals[:, 4:8]).view(np.float32).reshape(-1)
        prof = add_profiles(prof, _profile_piece(keys, counts, w))
    return prof


def read_cut_keys(cfg, seed, reads, read_len, genome, noisy, n_end=256):
    """canonical k-mers cut from positions 0, 60 and the last of the job's first and last n_end reads (duplicates dropped)"""
    k = cfg.k
    last = read_len - k
    pos = sorted({0, min(60, last), last})
    out = []
    for first in (0, reads - n_end):
        rb = synth_reads_8d(seed, first, n_end, read_len, genome, noisy, threads=1)
        for i in range(rb.n):
            kk, _, _ = oracle_weighted_kmers(cfg, rb.seq(i), rb.qual(i))
            out.append(kk[pos])
    keys = np.concatenate(out)
    _, first_at = np.unique(keys_as_void(keys), return_index=True)
    return np.ascontiguousarray(keys[np.sort(first_at)])


def keys_as_void(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    return keys.view(np.dtype((np.void, keys.shape[1]))).reshape(-1)


def match_keys(want, have):
    """index into `have` of every row of `want`, -1 where absent (both [n, kb] uint8)"""
    idx = np.full(want.shape[0], -1, np.int64)
    if have.shape[0] == 0 or want.shape[0] == 0:
        return idx
    hv, wv = keys_as_void(have), keys_as_void(want)
    order = np.argsort(hv, kind="stable")
    pos = np.searchsorted(hv[order], wv)
    pos = np.minimum(pos, hv.size - 1)
    hit = hv[order][pos] == wv
    idx[hit] = order[pos[hit]]
    return idx


RC_ABSENT, RC_SINGLETON, RC_WEAK = 0, 1, 2


def weighted_answers(keys, weak_keys, weak_counts, weak_w, sing_keys, sing_w8):
    """(kind, count, f64 answer) of getCount(keys) / getCount(keys, useWeights=True) against a weak map and a singleton map given as
    entries: a weak entry answers its count and f32 weightedCount, a singleton count (w8 != 0) and (w8 - 1) / 254, an absent key 0"""
    n = keys.shape[0]
    kind = np.zeros(n, np.uint8)
    cnt = np.zeros(n, np.uint32)
    ans = np.zeros(n, np.float64)
    iw = match_keys(keys, weak_keys)
    hit = iw >= 0
    kind[hit], cnt[hit], ans[hit] = RC_WEAK, weak_counts[iw[hit]], weak_w[iw[hit]].astype(np.float64)
    isg = match_keys(keys, sing_keys)
    hs = (isg >= 0) & ~hit
    w8 = sing_w8[isg[hs]].astype(np.float64)
    kind[hs], cnt[hs], ans[hs] = RC_SINGLETON, (w8 != 0), np.where(w8 != 0, (w8 - 1.0) / 254.0, 0.0)
    return kind, cnt, ans


def singleton_entries(buf, kb, ext=False):
    """keys [n, kb] and _weight bytes of a stored singleton map"""
    pieces = list(image_pieces(buf, kb, 5 if ext else 1, cols=1))
    if not pieces:
        return np.zeros((0, kb), np.uint8), np.zeros(0, np.uint8)
    return np.concatenate([p[0] for p in pieces]), np.concatenate([p[1][:, 0] for p in pieces])


def full_size_weights(name):
    """the committed weight profile of full_size_digests.json[name] (tests/golden/full_size_weights.npz), None if there is none"""
    path = os.path.join(GOLDEN, "full_size_weights.npz")
    with np.load(path) as z:
        pre = name + "/"
        got = {key[len(pre):]: z[key] for key in z.files if key.startswith(pre)}
    return got or None


SK_ORDERED_FROM = 256          # kmernator_amd/csrc/kmr_superkmer.hpp: the default build redoes such k-mers' weights in input order


def weight_bin_bound(want):
    """what |wsum_got - wsum_want| of a bin may be: both sides add the same positive f32 weights on top of the same quantised first
    sighting; the reference adds in order, each addition off by at most 2^-24 of a partial sum <= w, the product rounds once, so
    |d| <= (n + 1) 2^-24 w per entry and the bin's sum of (n + 2) 2^-24 w leaves one term of slack (a theorem)"""
    return 2.0 ** -24 * want["nwsum"] * (1.0 + 1e-6) + 1e-12 * np.abs(want["wsum"])


def weight_entry_bound(count, w, build_mode):
    """what |weightedCount_got - weightedCount_want| of one weak entry of `count` sightings may be: (n + 2) 2^-24 w; the super-k-mer
    build (modes 0 and 3) is held to 1e-5 n below SK_ORDERED_FROM too, and bit for bit from there on (it adds in input order)"""
    n = np.asarray(count, np.float64)
    b = (n + 2.0) * 2.0 ** -24 * np.abs(np.asarray(w, np.float64))
    if build_mode in (0, 3):
        b = np.where(n >= SK_ORDERED_FROM, 0.0, np.minimum(1e-5 * n, b))
    return b


def _ratio(d, bound):
    d = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def weight_bin_ratio(got, want):
    """largest |d wsum| / weight_bin_bound over the bins (<= 1 passes); entries and count_sum of every bin must be equal"""
    assert np.array_equal(np.asarray(got["entries"], np.int64), np.asarray(want["entries"], np.int64)), "entries per bin differ"
    assert np.array_equal(np.asarray(got["count_sum"], np.int64), np.asarray(want["count_sum"], np.int64)), "count_sum per bin differs"
    return _ratio(np.asarray(got["wsum"]) - want["wsum"], weight_bin_bound(want))


def weight_entry_ratio(count, w, want_count, want_w, build_mode):
    """largest |d weightedCount| / weight_entry_bound over entries (<= 1 passes); the counts must be equal"""
    assert np.array_equal(np.asarray(count, np.int64), np.asarray(want_count, np.int64)), "counts differ"
    return _ratio(np.asarray(w, np.float64) - np.asarray(want_w, np.float64), weight_entry_bound(want_count, want_w, build_mode))


def weight_profile_agrees(got, want, build_mode=1):
    """the bins, the sample's keys and counts and the sample's weights of two profiles within their bounds"""
    try:
        if "entries" in want and weight_bin_ratio(got, want) > 1.0:
            return False
        if not np.array_equal(got["sample_keys"], want["sample_keys"]):
            return False
        return weight_entry_ratio(got["sample_count"], got["sample_w"], want["sample_count"], want["sample_w"], build_mode) <= 1.0
    except AssertionError:
        return False
