"""Host-side mirror of the reference's KmerSpectrum / KmerMap interface for the
spectrum-build path, over the C-ABI (include/kmernator_amd.h).

Method names follow the reference (src/KmerSpectrum.h): buildKmerSpectrum (:2081-2115),
purgeMinDepth (:1805), getCount (:701), storeMmap / restoreMmap (:476-518), getRawKmers...
(:455-459); MeraculousDistributedKmerSpectrum::dumpCounts/dumpGraphs (src/Meraculous.h:107-134).
Errors surface as KmerSpectrumError (the reference throws LoggedException, src/Log.h:442-484).
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import KMR_MAP_SINGLETON, KMR_MAP_WEAK, KmrStats


class KmerSpectrumError(RuntimeError):
    pass


class SizeTracker:
    """KmerSpectrum::SizeTracker (src/KmerSpectrum.h:812-900): elements[i] = (rawKmers, rawGoodKmers, uniqueKmers, singletonKmers)"""

    def __init__(self, elements):
        self.elements = np.asarray(elements, dtype=np.uint64).reshape(-1, 4)

    def getLastElement(self):
        return tuple(int(v) for v in self.elements[-1]) if len(self.elements) else (0, 0, 0, 0)

    def toString(self):
        """SizeTracker::toString (:873-878): the header, then one tab-separated line per element"""
        return "rawKmers\trawGoodKmers\tuniqueKmers\tsingletonKmers\n" + "".join("%d\t%d\t%d\t%d\n" % tuple(int(v) for v in e) for e in self.elements)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ok(rc, what):
    """a status of the library that has no handle error text behind it"""
    if rc != 0:
        raise KmerSpectrumError("%s: %s" % (what, _lib.STATUS.get(rc, rc)))


class _DeviceObject:
    """A device object of the library owned through a handle (the attribute named _HANDLE) and given back with the library's
    function _FREE: by close(), which may be called again, at the end of a `with` block, and when the object is collected."""
    _HANDLE = _FREE = None

    def _live(self):
        h = getattr(self, self._HANDLE, None)
        if not h:
            raise KmerSpectrumError("%s: closed" % type(self).__name__)
        return h

    def close(self):
        h = getattr(self, self._HANDLE, None)
        if h:
            getattr(self.sp.lib, self._FREE)(h)
            setattr(self, self._HANDLE, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# one kmr_compare_counts
COMPARE_DTYPE = np.dtype([(n, np.uint64) for n in ("size1", "size2", "common", "common_count1", "common_count2", "total_count1", "total_count2", "saturated")])
COMPARE_HEADER = b"\nSet 1\tSet 2\tCommon\t%Uniq1\t%Tot1\t%Uniq2\t%Tot2\n"      # apps/CompareSpectrums.cpp:211-212


def compare_line(counts, label=b""):
    """one line of CompareSpectrums' table (apps/CompareSpectrums.cpp:234-241) as bytes, through kmr_compare_line: `counts` is a
    dict or a COMPARE_DTYPE record.  A zero denominator prints as -nan, as the reference's x86-64 glibc build does."""
    lib = _lib.load()
    c = _lib.KmrCompareCounts(*[int(counts[n]) for n in COMPARE_DTYPE.names])
    label = bytes(label)
    buf = C.create_string_buffer(160 + len(label))
    nb = C.c_uint64()
    _ok(lib.kmr_compare_line(C.byref(c), label, len(label), buf, len(buf), C.byref(nb)), "kmr_compare_line")
    return buf.raw[:nb.value]


def CompareSpectrums(spectrum2, set1, per_read=False, circular_reference=False, spectrum1=None):
    """apps/CompareSpectrums.cpp's output as bytes: the header and one line for set 1 as a whole against `spectrum2`, or with
    `per_read` one line per read of the ReadSet `set1`, labelled with the read's name.  `circular_reference` runs
    ReadSet::circularize(k) over set 1 first.  The whole form compares `spectrum1` if given (the finalized spectrum of set 1),
    else builds one of spectrum2's configuration from `set1` (solid-only: finalized with min_depth 1)."""
    reads = set1.circularize() if circular_reference and set1 is not None else set1
    out = [COMPARE_HEADER]
    try:
        if per_read:
            rec = spectrum2.compareReads(reads)
            names = reads.arrays()[3]
            out += [compare_line(rec[i], names[i]) for i in range(reads.n)]
        else:
            sp1, own = spectrum1, False
            if sp1 is None:
                sp1, own = KmerSpectrum(spectrum2.cfg), True
                sp1.buildKmerSpectrumFromReadSet(reads)
                sp1.purgeMinDepth(1)
            try:
                out.append(compare_line(sp1.countCommonKmers(spectrum2)))
            finally:
                if own:
                    sp1.close()
    finally:
        if reads is not set1:
            reads.close()
    return b"".join(out)


class KmerSpectrum:
    """One spectrum (weak + singleton maps) resident on one MI355X."""

    def __init__(self, cfg):
        self.lib = _lib.load()
        self.cfg = cfg
        self.k = cfg.k
        self.kb = (cfg.k + 3) // 4
        h = C.c_void_p()
        rc = self.lib.kmr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise KmerSpectrumError("kmr_create: %s: %s" % (_lib.STATUS.get(rc, rc), self.lib.kmr_last_error(None).decode()))
        self.h = h

    # -- plumbing
    def _check(self, rc, what):
        if rc != 0:
            raise KmerSpectrumError("%s: %s: %s" % (what, _lib.STATUS.get(rc, rc), self.lib.kmr_last_error(self.h).decode()))

    def _call(self, name, *a):
        self._check(getattr(self.lib, "kmr_" + name)(*a), "kmr_" + name)

    def close(self):
        if getattr(self, "h", None):
            self.lib.kmr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tune(self, **knobs):
        """kmr_tune: implementation knobs of this handle (none changes a result)"""
        for name, v in knobs.items():
            self._call("tune", self.h, name.encode(), float(v))
        return self

    # -- build
    def build_info(self, what):
        """kmr_build_info: a figure of the current build ("lists", "uniform_count", "chunk_pool_chunks")"""
        v = C.c_double()
        self._call("build_info", self.h, what.encode(), C.byref(v))
        return v.value

    def buildKmerSpectrum(self, bases, quals, offsets, first_read_idx=0, discarded=None):
        """KmerSpectrum::buildKmerSpectrum(const ReadSet&) on flat host arrays."""
        bases = _u8(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        q = None if quals is None else _u8(quals)
        d = None if discarded is None else _u8(discarded)
        self._call("add_reads", self.h, bases.ctypes.data_as(C.c_void_p), None if q is None else q.ctypes.data_as(C.c_void_p),
                   offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n, first_read_idx,
                   None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint8)))

    def buildKmerSpectrumDevice(self, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx=0, discarded_ptr=None):
        """Same, device pointers (torch tensor .data_ptr()); asynchronous, see sync()."""
        self._call("add_reads_dev", self.h, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx, discarded_ptr)

    def buildKmerSpectrumTwoBit(self, twobit, twobit_offsets, offsets, quals=None, uniform_quality=0, markups=None, first_read_idx=0, discarded=None):
        """KmerSpectrum::buildKmerSpectrum(const ReadSet&) on reads kept as the reference's Read keeps them: 2-bit packed bases (every read on
        bytes of its own) + markups (positions, chars, offsets[n+1]) + qualities (an array, or one character for all, or none)
        -- kmr_add_reads_twobit, host arrays"""
        tw = _u8(twobit)
        to = np.ascontiguousarray(twobit_offsets, dtype=np.uint64)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        q = None if quals is None else _u8(quals)
        d = None if discarded is None else _u8(discarded)
        mp = mc = mo = None
        if markups is not None:
            mp = np.ascontiguousarray(markups[0], dtype=np.uint32); mc = _u8(markups[1]); mo = np.ascontiguousarray(markups[2], dtype=np.uint64)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._call("add_reads_twobit", self.h, vp(tw), vp(to), vp(offsets), vp(mo), vp(mp), vp(mc), vp(q), int(uniform_quality), n, first_read_idx, vp(d))

    def buildKmerSpectrumTwoBitDevice(self, twobit_ptr, twobit_offsets_ptr, offsets_ptr, n_reads, total_bases, quals_ptr=None, uniform_quality=0,
                                      markup_offsets_ptr=None, markup_pos_ptr=None, markup_char_ptr=None, first_read_idx=0, discarded_ptr=None):
        """Same, device pointers (kmr_add_reads_twobit_dev); asynchronous, see sync().  quals_ptr points at the quality of the call's first base."""
        self._call("add_reads_twobit_dev", self.h, twobit_ptr, twobit_offsets_ptr, offsets_ptr, markup_offsets_ptr, markup_pos_ptr, markup_char_ptr,
                   quals_ptr, int(uniform_quality), n_reads, total_bases, first_read_idx, discarded_ptr)

    def buildKmerSpectrumFromReadSet(self, read_set, first_read_idx=0):
        """KmerSpectrum::buildKmerSpectrum(const ReadSet&) on a device-resident ReadSet (kmr_add_read_batch)."""
        self._call("add_read_batch", self.h, read_set.r, first_read_idx)

    def subtractReference(self, other):
        """KmerSpectrum::subtractReference: k-mers of the finalized spectrum `other` are skipped by later builds"""
        self._subtracting = other          # keep it alive
        self._call("subtract_reference", self.h, None if other is None else other.h)

    def getSubtracted(self):
        v = C.c_uint64()
        self._call("subtracted", self.h, C.byref(v))
        return v.value

    def reset(self):
        """weak.reset(false); singleton.reset(false) of buildKmerSpectrum (src/KmerSpectrum.h:2091-2096)"""
        self._call("reset", self.h)

    def release_table(self):
        self._call("release_table", self.h)

    def sync(self):
        self._call("sync", self.h)

    def purgeMinDepth(self, min_depth=2):
        """purgeMinDepth + optimize(); the maps become immutable (kmr_finalize)."""
        self._call("finalize", self.h, min_depth)

    finalize = purgeMinDepth

    # -- owner-partitioned pieces (one process per GPU)
    def extractByOwnerDevice(self, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx,
                             records_ptr, seg_capacity, seg_counts_ptr, discarded_ptr=None):
        self._call("extract_by_owner_dev", self.h, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx,
                   discarded_ptr, records_ptr, seg_capacity, seg_counts_ptr)

    def insertRecordsDevice(self, records_ptr, n):
        self._call("insert_records_dev", self.h, records_ptr, n)

    # the whole owner exchange inside the library (kmr_exchange_*): RCCL called from C++, or a transport the host supplies
    @staticmethod
    def exchange_unique_id():
        """rank 0: the job's RCCL id (KMR_EXCHANGE_ID_BYTES bytes) to hand to every rank"""
        buf = (C.c_uint8 * 128)()
        lib = _lib.load()
        rc = lib.kmr_exchange_unique_id(C.cast(buf, C.c_void_p))
        if rc:
            raise KmerSpectrumError("kmr_exchange_unique_id failed (%d): %s" % (rc, lib.kmr_last_error(None).decode()))
        return bytes(buf)

    def exchange_init(self, unique_id):
        """collective: ncclCommInitRank(world_size, id, rank) on the handle's device (kmr_exchange_init)"""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._call("exchange_init", self.h, C.cast(buf, C.c_void_p))

    def exchange_init_transport(self, allgather_u64, alltoallv_dev):
        """kmr_exchange_init_transport with Python callables (tests: gloo).  allgather_u64(mine: list[int]) -> list of world rows;
        alltoallv_dev(send_ptr, send_off, send_bytes, recv_ptr, recv_off, recv_bytes, stream) with lists of world ints."""
        world = self.cfg.world_size
        u64p = C.POINTER(C.c_uint64)
        AG = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, C.c_uint64, u64p)
        AV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, u64p, u64p, C.c_void_p, u64p, u64p, C.c_void_p)

        def ag(user, mine, n, out):
            try:
                rows = allgather_u64([int(mine[i]) for i in range(n)])
                for r in range(world):
                    for j in range(n):
                        out[r * n + j] = int(rows[r][j])
                return 0
            except Exception:          # noqa: BLE001 -- the exception cannot cross the C frame
                import traceback
                traceback.print_exc()
                return -1

        def av(user, send, soff, sbytes, recv, roff, rbytes, stream):
            try:
                alltoallv_dev(send, [int(soff[r]) for r in range(world)], [int(sbytes[r]) for r in range(world)],
                              recv, [int(roff[r]) for r in range(world)], [int(rbytes[r]) for r in range(world)], stream)
                return 0
            except Exception:          # noqa: BLE001
                import traceback
                traceback.print_exc()
                return -1

        class Transport(C.Structure):
            _fields_ = [("user", C.c_void_p), ("allgather_u64", AG), ("alltoallv_dev", AV)]
        self._transport = Transport(None, AG(ag), AV(av))          # keeps the callbacks alive as long as the handle
        self._call("exchange_init_transport", self.h, C.cast(C.pointer(self._transport), C.c_void_p))

    def exchange_add_reads(self, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx=0, discarded_ptr=None):
        """collective: one batch of this rank's reads through extract -> all-to-all -> insert at the owner (kmr_exchange_add_reads_dev)"""
        self._call("exchange_add_reads_dev", self.h, bases_ptr, quals_ptr, offsets_ptr, n_reads, total_bases, first_read_idx, discarded_ptr)

    def exchange_stats(self):
        b = C.c_uint64()
        ms = C.c_double()
        self._call("exchange_stats", self.h, C.byref(b), C.byref(ms))
        return {"bytes_to_peers": b.value, "alltoall_ms": ms.value}

    def set_stream_origin(self, ordinal):
        """position in the whole input of the next base this handle is fed (kmr_set_stream_origin)"""
        self._call("set_stream_origin", self.h, int(ordinal))

    # owner exchange of super-k-mer lists (build_mode 3; kmernator_amd.distributed.build_partitioned_superkmers)
    def sk_exchange_begin(self):
        """from here on the handle's reads go through the list exchange: every owner's k-mers are kept (kmr_sk_exchange_begin)"""
        self._call("sk_exchange_begin", self.h)

    def sk_exchange_counts(self):
        world = self.cfg.world_size
        chunks = np.zeros(world, dtype=np.uint64)
        granules = np.zeros(world, dtype=np.uint64)
        self._call("sk_exchange_counts", self.h, chunks.ctypes.data_as(C.POINTER(C.c_uint64)), granules.ctypes.data_as(C.POINTER(C.c_uint64)))
        return chunks, granules

    def sk_exchange_pack(self, data_ptr, meta_ptr, granule_offset, chunk_offset):
        go = np.ascontiguousarray(granule_offset, dtype=np.uint64)
        co = np.ascontiguousarray(chunk_offset, dtype=np.uint64)
        self._call("sk_exchange_pack_dev", self.h, data_ptr, meta_ptr, go.ctypes.data_as(C.POINTER(C.c_uint64)), co.ctypes.data_as(C.POINTER(C.c_uint64)))

    def sk_exchange_uniform(self):
        """kmr_sk_exchange_uniform: kind << 32 | weight bits of this rank's records (what a sender tells the owners)"""
        v = C.c_uint64()
        self._call("sk_exchange_uniform", self.h, C.byref(v))
        return v.value

    def sk_exchange_peer_uniform(self, state):
        """kmr_sk_exchange_peer_uniform: fold a sender's state in, before adopting its chunks"""
        self._call("sk_exchange_peer_uniform", self.h, int(state))

    def sk_exchange_range(self, list_lo=0, list_hi=0xFFFFFFFFFFFFFFFF):
        """kmr_sk_exchange_range: the lists the next sk_exchange_counts / sk_exchange_pack are about"""
        self._call("sk_exchange_range", self.h, int(list_lo), int(list_hi))

    def count_lists_prefix(self, min_depth, list_hi):
        """kmr_count_lists_prefix: count this handle's lists below list_hi now (asynchronously); finalize(min_depth) does the rest"""
        self._call("count_lists_prefix", self.h, int(min_depth), int(list_hi))

    def sk_exchange_adopt(self, data_ptr, meta_ptr, n_chunks, n_granules):
        self._call("sk_exchange_adopt_dev", self.h, data_ptr, meta_ptr, n_chunks, n_granules)

    # the device steps of the distributed scoreAndTrimReads (kmernator_amd.distributed.score_partitioned); tensors are torch
    # tensors on this handle's device
    def lookup_requests(self, bases, offsets, lo, hi, total_bases, keys, pos, seg_capacity, seg_counts):
        self._call("lookup_requests_dev", self.h, bases.data_ptr(), offsets.data_ptr() + 8 * lo, hi - lo, total_bases,
                   keys.data_ptr(), pos.data_ptr(), seg_capacity, seg_counts.data_ptr())

    def lookup_keys(self, keys, n, counts):
        self._call("lookup_keys_dev", self.h, keys.data_ptr(), n, counts.data_ptr())

    def lookup_keys_weighted(self, keys, n, weights):
        """lookup_keys answered as KmerSpectrum::getCount(kmer, true): weights (f64) from the weak map, else the singleton map."""
        self._call("lookup_keys_weighted_dev", self.h, keys.data_ptr(), n, weights.data_ptr())

    def scatter_counts(self, counts, pos, n, position_counts):
        self._call("scatter_counts_dev", self.h, counts.data_ptr(), pos.data_ptr(), n, position_counts.data_ptr())

    def score_counts(self, bases, offsets, n_reads, position_counts, minimum_kmer_score, scoring_type="MEDIAN", bimodal_sigmas=-1.0):
        """kmr_score_counts_dev; bimodal_sigmas as scoreAndTrimReads takes it (the default leaves the handle's setting, which is
        how the distributed scoring picks it up)"""
        to = np.zeros(n_reads, dtype=np.uint32)
        tl = np.zeros(n_reads, dtype=np.uint32)
        sc = np.zeros(n_reads, dtype=np.float32)
        wt = np.zeros(n_reads, dtype=np.uint8)
        if n_reads:
            with self._bimodal_for(bimodal_sigmas, n_reads):
                self._call("score_counts_dev", self.h, bases.data_ptr(), offsets.data_ptr(), n_reads, position_counts.data_ptr(), float(minimum_kmer_score),
                           self.SCORING[scoring_type], to.ctypes.data_as(C.POINTER(C.c_uint32)), tl.ctypes.data_as(C.POINTER(C.c_uint32)),
                           sc.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_uint8)))
        return to, tl, sc, wt.astype(bool)

    def stream(self):
        return self.lib.kmr_stream(self.h)

    # -- queries
    def stats(self):
        s = KmrStats()
        self._call("get_stats", self.h, C.byref(s))
        return s.as_dict()

    def getRawKmers(self):
        return self.stats()["raw_kmers"]

    def getRawGoodKmers(self):
        return self.stats()["raw_good_kmers"]

    def getUniqueKmers(self):
        return self.stats()["unique_kmers"]

    def getSingletonKmers(self):
        return self.stats()["singleton_kmers"]

    def num_buckets(self, which):
        v = C.c_uint64()
        self._call("num_buckets", self.h, which, C.byref(v))
        return v.value

    def getCount(self, packed_kmers, useWeights=False):
        """KmerSpectrum::getCount(kmer, useWeights) for packed canonical k-mers [n, kb]: u32 counts, or with useWeights f64
        weighted counts (weak weightedCount, else the singleton's (_weight - 1) / 254, else 0).  The reference's own default
        is the weighted form (TrackingData::useWeightedByDefault); this wrapper's has always been the count."""
        keys = _u8(packed_kmers)
        n = keys.size // self.kb
        if useWeights:
            out = np.zeros(n, dtype=np.float64)
            if n:
                self._call("lookup_weighted", self.h, keys.ctypes.data_as(C.POINTER(C.c_uint8)), n, out.ctypes.data_as(C.POINTER(C.c_double)))
            return out
        out = np.zeros(n, dtype=np.uint32)
        if n:
            self._call("lookup", self.h, keys.ctypes.data_as(C.POINTER(C.c_uint8)), n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    lookup = getCount

    def getCountsForReads(self, bases, offsets, useWeights=False):
        """Per-position counts of every read (ReadSelector::setKmerValues); with useWeights the f64 weighted counts of
        getCount(kmer, true) at the same positions (KmerSpectrum::getCounts(KmerWeights&, true), the reference's default)."""
        bases = _u8(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
        nk = np.maximum(lens - self.k + 1, 0).astype(np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(nk, out=out_off[1:])
        name, dt, ct = ("lookup_reads_weighted", np.float64, C.c_double) if useWeights else ("lookup_reads", np.uint32, C.c_uint32)
        out = np.zeros(int(out_off[-1]), dtype=dt)
        if n:
            self._call(name, self.h, bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                       out.ctypes.data_as(C.POINTER(ct)), out_off.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out, out_off

    SCORING = {"SUM": 0, "MEDIAN": 1, "MIN": 2, "MAX": 3, "AVG": 4}

    # -- bimodal trimming (ReadSelector --bimodal-sigmas)
    bimodal_sigmas = -1.0          # the handle's setting, as kmr_create leaves it
    _scored_reads = None           # the number of reads of the last scoring call made through this object
    bimodal_active = False         # ... and whether the bimodal cut was on in it

    def setBimodalSigmas(self, sigmas):
        """kmr_set_bimodal_sigmas: --bimodal-sigmas for every scoring call of this handle from now on (negative = off, the default).
        With it on, a run of >= 3 k-mers is cut where its two halves differ most in mean depth, if the means lie more than
        sigmas x max("stdDev") apart (include/kmernator_amd.h has the exact rule); bimodal() tells which reads were cut."""
        self._call("set_bimodal_sigmas", self.h, float(sigmas))
        self.bimodal_sigmas = float(sigmas)
        return self

    @contextlib.contextmanager
    def _bimodal_for(self, sigmas, n_reads):
        """one scoring call of n_reads reads: with sigmas >= 0 (or NaN, which the library refuses) under that setting, the handle's
        own restored afterwards; the default, a negative value, leaves the handle's setting"""
        sigmas = float(sigmas)
        override = not sigmas < 0
        if override:
            self._call("set_bimodal_sigmas", self.h, sigmas)
        try:
            self.bimodal_active = override or self.bimodal_sigmas >= 0
            self._scored_reads = int(n_reads)
            yield
        finally:
            if override:
                self._call("set_bimodal_sigmas", self.h, self.bimodal_sigmas)

    def bimodal(self, n_reads=None):
        """kmr_bimodal_copy: one u64 per read of the last scoring call (n_reads defaults to that call's): 0 = not cut, else
        p + k in bits 0-31, (int)first.mean in bits 32-47, (int)second.mean in bits 48-63; all zero if the option was off"""
        n = self._scored_reads if n_reads is None else int(n_reads)
        if n is None:
            raise KmerSpectrumError("bimodal: no scoring call yet")
        words = np.zeros(max(1, n), dtype=np.uint64)
        self._call("bimodal_copy", self.h, words.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        return words[:n]

    @staticmethod
    def bimodal_tag(word):
        """the label part of one word of bimodal(): b"Bimodal@<pos>:<m1>/<m2>", b"InvBimodal@..." or b"" for 0"""
        word = int(word)
        if not word:
            return b""
        m1, m2 = (word >> 32) & 0xffff, word >> 48
        return b"%sBimodal@%d:%d/%d" % (b"Inv" if m1 < m2 else b"", word & 0xffffffff, m1, m2)

    def scoreAndTrimReads(self, bases, offsets, minimum_kmer_score, scoring_type="MEDIAN", bimodal_sigmas=-1.0):
        """ReadSelector::scoreAndTrimReads: (trim_offset, trim_length, score, was_trimmed) per read.  bimodal_sigmas >= 0 turns
        the bimodal cut on for this call; the default leaves the handle's setting (setBimodalSigmas; off unless set)."""
        bases = _u8(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        to = np.zeros(n, dtype=np.uint32)
        tl = np.zeros(n, dtype=np.uint32)
        sc = np.zeros(n, dtype=np.float32)
        wt = np.zeros(n, dtype=np.uint8)
        if n:
            with self._bimodal_for(bimodal_sigmas, n):
                self._call("score_reads", self.h, bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                           float(minimum_kmer_score), self.SCORING[scoring_type], to.ctypes.data_as(C.POINTER(C.c_uint32)),
                           tl.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_uint8)))
        return to, tl, sc, wt.astype(bool)

    def scoreAndTrimReadSet(self, read_set, minimum_kmer_score, scoring_type="MEDIAN", bimodal_sigmas=-1.0):
        """scoreAndTrimReads on a device-resident ReadSet (kmr_score_read_batch)"""
        n = read_set.n
        to = np.zeros(n, dtype=np.uint32)
        tl = np.zeros(n, dtype=np.uint32)
        sc = np.zeros(n, dtype=np.float32)
        wt = np.zeros(n, dtype=np.uint8)
        if n:
            with self._bimodal_for(bimodal_sigmas, n):
                self._call("score_read_batch", self.h, read_set.r, float(minimum_kmer_score), self.SCORING[scoring_type], to.ctypes.data_as(C.POINTER(C.c_uint32)),
                           tl.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_uint8)))
        return to, tl, sc, wt.astype(bool)

    def histogram(self, nbins=256):
        counts = np.zeros(nbins, dtype=np.uint64)
        weights = np.zeros(nbins, dtype=np.float64)
        self._call("count_histogram", self.h, counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                   weights.ctypes.data_as(C.POINTER(C.c_double)), nbins)
        return counts, weights

    def digest(self, which=KMR_MAP_WEAK):
        """kmr_map_digest: order-independent digest of a finalized map (sums of rank / part digests = the whole spectrum's)"""
        d = _lib.KmrDigest()
        self._call("map_digest", self.h, which, C.byref(d))
        return d.as_dict()

    def getHistogram(self, zoom_max=256, log_base=2.0):
        """KmerSpectrum::getHistogram (src/KmerSpectrum.h:1066-1071): Histogram(256).set(*this) -> Histogram"""
        nb = self.lib.kmr_histogram_bins(zoom_max)
        visits = np.zeros(nb, dtype=np.uint64)
        vcount = np.zeros(nb, dtype=np.uint64)
        vweight = np.zeros(nb, dtype=np.float64)
        self._call("histogram", self.h, zoom_max, log_base, visits.ctypes.data_as(C.POINTER(C.c_uint64)),
                   vcount.ctypes.data_as(C.POINTER(C.c_uint64)), vweight.ctypes.data_as(C.POINTER(C.c_double)), nb)
        return Histogram(zoom_max, log_base, visits, vcount, vweight)

    def getSizeTracker(self, force_last=True):
        """KmerSpectrum::getSizeTracker (src/KmerSpectrum.h:902-904) after trackSpectrum(force_last): the size history, sampled at
        read boundaries (kmr_size_tracker; needs kmr_config.size_tracker = 1)"""
        n = C.c_uint64()
        self._call("size_tracker", self.h, 1 if force_last else 0, None, 0, C.byref(n))
        el = np.zeros((n.value, 4), dtype=np.uint64)
        if n.value:
            self._call("size_tracker", self.h, 1 if force_last else 0, el.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n))
        return SizeTracker(el)

    # -- export / restore in the reference's mmap format
    def image(self, which=KMR_MAP_WEAK):
        sz = C.c_uint64()
        self._call("image_size", self.h, which, C.byref(sz))
        buf = np.zeros(sz.value, dtype=np.uint8)
        self._call("write_image", self.h, which, buf.ctypes.data_as(C.c_void_p), sz.value)
        return buf

    def load_image(self, which, buf):
        buf = _u8(buf)
        self._call("load_image", self.h, which, buf.ctypes.data_as(C.c_void_p), buf.size)

    def merge_image(self, which, buf):
        """restore-and-merge of one stored part (KmerSpectrum::buildKmerSpectrumInParts, src/KmerSpectrum.h:1871-1884)"""
        buf = _u8(buf)
        self._call("merge_image", self.h, which, buf.ctypes.data_as(C.c_void_p), buf.size)

    def storeMmap(self, filename, min_depth=2):
        """KmerSpectrum::storeMmap: <filename> (weak) and <filename>-singleton when min_depth <= 1."""
        self.image(KMR_MAP_WEAK).tofile(filename)
        if min_depth <= 1:
            self.image(KMR_MAP_SINGLETON).tofile(filename + "-singleton")

    def restoreMmap(self, filename):
        """KmerSpectrum::restoreMmap"""
        loaded = False
        if os.path.exists(filename) and os.path.getsize(filename) > 0:
            self.load_image(KMR_MAP_WEAK, np.fromfile(filename, dtype=np.uint8))
            loaded = True
        s = filename + "-singleton"
        if os.path.exists(s) and os.path.getsize(s) > 0:
            self.load_image(KMR_MAP_SINGLETON, np.fromfile(s, dtype=np.uint8))
            loaded = True
        if not loaded:
            raise KmerSpectrumError("Terribly sorry but there were no kmer spectrum mmap files at: %s*" % filename)

    def dumpCounts(self, filename, min_depth):
        self._call("dump_mercount", self.h, filename.encode(), min_depth)

    def dumpGraphs(self, filename, min_depth):
        self._call("dump_mergraph", self.h, filename.encode(), min_depth)

    DUMP_KIND = {"mercount": 0, "mergraph": 1}

    def dumpTextSize(self, kind, min_depth, lo=0, hi=None):
        """(kept entries, bytes) of the text kmr_dump_text would make for the weak entries [lo, hi) (kmr_dump_text_size); kind: "mercount" / "mergraph" or 0 / 1"""
        kept, nbytes = C.c_uint64(), C.c_uint64()
        self._call("dump_text_size", self.h, self.DUMP_KIND.get(kind, kind), min_depth, lo, _U64_MAX if hi is None else hi, C.byref(kept), C.byref(nbytes))
        return kept.value, nbytes.value

    def _dump_text(self, kind, min_depth, lo, hi):
        out = C.c_void_p()
        self._call("dump_text", self.h, kind, min_depth, lo, _U64_MAX if hi is None else hi, C.byref(out))
        return DumpText(self, out)

    def dumpCountsText(self, min_depth, lo=0, hi=None):
        """dumpCounts' text (src/Meraculous.h:107-120) for the weak entries [lo, hi) in map order, left in device memory: a DumpText"""
        return self._dump_text(0, min_depth, lo, hi)

    def dumpGraphsText(self, min_depth, lo=0, hi=None):
        """dumpGraphs' text (src/Meraculous.h:121-133) likewise; needs KMR_VALUE_EXT"""
        return self._dump_text(1, min_depth, lo, hi)

    # -- CompareSpectrums (apps/CompareSpectrums.cpp)
    def countCommonKmers(self, other):
        """countCommonKmers / evaluate (apps/CompareSpectrums.cpp:146-162, :225-242) of this spectrum as map 1 against `other` as
        map 2 (kmr_compare_spectrums): a dict of size1, size2, common, common_count1, common_count2, total_count1, total_count2 and
        saturated -- the entries read whose stored count is 65535; the figures are the reference's while that is 0, lower bounds
        otherwise."""
        c = _lib.KmrCompareCounts()
        other._call("compare_spectrums", self.h, other.h, C.byref(c))
        return c.as_dict()

    def compareReads(self, read_set):
        """evaluatePerRead (:243-257): every read of `read_set` on its own as map 1 against this spectrum as map 2
        (kmr_compare_reads): a structured array of one COMPARE_DTYPE record per read, in read order"""
        out = np.zeros(read_set.n, dtype=COMPARE_DTYPE)
        self._call("compare_reads", self.h, read_set._live(), out.ctypes.data_as(C.c_void_p) if read_set.n else None)
        return out

    def kernel_time(self, which=0):
        ms, n = C.c_double(), C.c_uint64()
        self._call("kernel_time", self.h, which, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def kernel_time_reset(self):
        self._call("kernel_time_reset", self.h)


_U64_MAX = (1 << 64) - 1


class DumpText(_DeviceObject):
    """A mercount / mergraph text in device memory (kmr_text): .kept entries, .bytes; numpy() copies it to the host,
    device_tensor() is a torch uint8 view of it where it lies, valid until close()."""
    _HANDLE, _FREE = "_t", "kmr_text_free"

    def __init__(self, sp, handle):
        self.sp, self._t = sp, handle
        kept, nbytes = C.c_uint64(), C.c_uint64()
        sp._call("text_info", handle, C.byref(kept), C.byref(nbytes))
        self.kept, self.bytes = kept.value, nbytes.value

    def numpy(self):
        buf = np.zeros(self.bytes, dtype=np.uint8)
        _ok(self.sp.lib.kmr_text_copy(self._live(), buf.ctypes.data_as(C.c_void_p) if self.bytes else None, self.bytes), "kmr_text_copy")
        return buf

    def device_ptr(self):
        p = C.c_void_p()
        self.sp._call("text_device_ptr", self._live(), C.byref(p))
        return p.value or 0

    def device_tensor(self):
        import torch
        ptr = self.device_ptr()
        if not self.bytes:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        view = type("_DeviceBytes", (), {"__cuda_array_interface__": {"shape": (self.bytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}})()
        return torch.as_tensor(view, device="cuda")



class Histogram:
    """KmerSpectrum::Histogram (src/KmerSpectrum.h:909-1057): buckets filled on the device, finish()/toString() here."""

    def __init__(self, zoom_max, log_base, visits, visited_count, visited_weight):
        import math
        self.zoomMax, self.logBase = zoom_max, log_base
        self.logFactor = math.log(log_base)
        self.zoomLogSkip = int(math.log(zoom_max + 1.0) / self.logFactor - 1.0)
        self.visits, self.visitedCount, self.visitedWeight = visits, visited_count, visited_weight
        self.finish()

    def getBucketValue(self, idx):
        return idx if idx <= self.zoomMax else int(self.logBase ** float(idx + self.zoomLogSkip - self.zoomMax))

    def finish(self):
        """:986-1001"""
        self.cumulativeVisits = np.cumsum(self.visits[::-1])[::-1].copy()
        self.count = int(self.visits.sum())
        nz = np.nonzero(self.visits)[0]
        self.lastBucket = int(nz[-1]) if nz.size else 0
        self.totalCount = float(self.visitedCount[nz].astype(np.float64).sum()) if nz.size else 0.0
        # the reference sums from the last bucket down
        tw = 0.0
        for i in nz[::-1]:
            tw += float(self.visitedWeight[i])
        self.totalWeightedCount = tw

    def toString(self):
        """:1002-1035, std::fixed << std::setprecision(3)"""
        f = lambda x: "%.3f" % x
        div = lambda a, b: (a / b) if b else float("nan")
        out = ["Counts, Weights and Directions",
               "Counts:\t%d\t%s\t%s\t" % (self.count, f(self.totalCount), f(div(self.totalCount, self.count))),
               "Weights:\t%d\t%s\t%s\t%s" % (self.count, f(self.totalWeightedCount), f(div(self.totalWeightedCount, self.count)),
                                                f(div(self.totalWeightedCount, self.totalCount))),
               "",
               "Bucket\tCumulative\tUnique\t%Unique\tCount\t%Count\tWeight\tQualProb\t%Weight"]
        for i in range(1, self.lastBucket + 1):
            v, c, w = int(self.visits[i]), int(self.visitedCount[i]), float(self.visitedWeight[i])
            out.append("%d\t%d\t%d\t%s\t%d\t%s\t\t%s\t%s\t%s\t" % (
                self.getBucketValue(i), int(self.cumulativeVisits[i]), v, f(div(100.0 * v, self.count)), c,
                f(div(100.0 * c, self.totalCount)), f(w), f(div(w, c)), f(div(100.0 * w, self.totalWeightedCount))))
        return "\n".join(out) + "\n"


class ReadSet(_DeviceObject):
    """Device-resident reads parsed from FASTQ text on the GPU: the reference's ReadSet::appendFastq path
    (src/ReadSet.cpp:311-345 over FastqStreamParser, src/ReadFileReader.h:768-835) incl. the Casava-1.8 filter and the
    quality-base detection of validateFastqStart (src/ReadSet.h:171-209).  Bound to the device of `spectrum`."""
    _HANDLE, _FREE = "r", "kmr_reads_free"

    def __init__(self, spectrum, text, input_quality_base=0, store_comment=True):
        self.sp = spectrum
        self.text = bytes(text)
        self.store_comment = bool(store_comment)
        r = C.c_void_p()
        buf = np.frombuffer(self.text, dtype=np.uint8)
        spectrum._call("ingest_fastq", spectrum.h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size,
                       input_quality_base, 1 if store_comment else 0, C.byref(r))
        self.r = r
        n, tot, qb, nf = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        spectrum.lib.kmr_reads_info(self.r, C.byref(n), C.byref(tot), C.byref(qb), C.byref(nf))
        self.n, self.total_bases, self.input_quality_base, self.filtered = n.value, tot.value, qb.value, nf.value

    @classmethod
    def _adopt(cls, spectrum, text, handle, store_comment=True):
        """wrap a kmr_reads the library produced from another batch (names still point into `text`)"""
        self = cls.__new__(cls)
        self.sp, self.text, self.r = spectrum, text, handle
        self.store_comment = bool(store_comment)
        n, tot, qb, nf = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        spectrum.lib.kmr_reads_info(self.r, C.byref(n), C.byref(tot), C.byref(qb), C.byref(nf))
        self.n, self.total_bases, self.input_quality_base, self.filtered = n.value, tot.value, qb.value, nf.value
        return self

    @classmethod
    def from_fasta(cls, spectrum, text, qual_text=None, store_comment=True):
        """reads parsed on the device from FASTA text (every quality Read::REF_QUAL) or, with `qual_text`, from a FASTA + QUAL pair
        (FastaStreamParser / FastaQualStreamParser, src/ReadFileReader.h:844-1006): kmr_ingest_fasta.  A record may have any number
        of lines and any length; names point into `text`, which the set keeps."""
        text = bytes(text)
        buf = np.frombuffer(text, dtype=np.uint8)
        qbuf = None if qual_text is None else np.frombuffer(bytes(qual_text) + b"\n", dtype=np.uint8)      # never empty: NULL means no qual text
        r = C.c_void_p()
        spectrum._call("ingest_fasta", spectrum.h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size,
                       None if qbuf is None else qbuf.ctypes.data_as(C.c_void_p), 0 if qbuf is None else qbuf.size - 1, 1 if store_comment else 0, C.byref(r))
        return cls._adopt(spectrum, text, r, store_comment)

    @classmethod
    def from_arrays(cls, spectrum, bases, quals, offsets):
        """reads the host already holds (uint8 bases / quals scaled to the spectrum's quality base, uint64 offsets[n+1])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        r = C.c_void_p()
        spectrum._call("reads_from_host", spectrum.h, bases.ctypes.data_as(C.c_void_p), quals.ctypes.data_as(C.c_void_p),
                       offsets.ctypes.data_as(C.POINTER(C.c_uint64)), offsets.size - 1, C.byref(r))
        return cls._adopt(spectrum, b"", r)

    @classmethod
    def from_twobit(cls, spectrum, twobit, twobit_offsets, offsets, quals=None, uniform_quality=0, markups=None):
        """reads the host keeps as the reference's Read does (2-bit packed bases, every read on bytes of its own; markups = (positions, chars,
        offsets[n+1]); qualities an array, one character for all, or none): kmr_reads_from_twobit"""
        tw = np.ascontiguousarray(twobit, dtype=np.uint8)
        to = np.ascontiguousarray(twobit_offsets, dtype=np.uint64)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        q = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
        mp = mc = mo = None
        if markups is not None:
            mp = np.ascontiguousarray(markups[0], dtype=np.uint32); mc = np.ascontiguousarray(markups[1], dtype=np.uint8); mo = np.ascontiguousarray(markups[2], dtype=np.uint64)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        r = C.c_void_p()
        spectrum._call("reads_from_twobit", spectrum.h, vp(tw), vp(to), vp(offsets), vp(mo), vp(mp), vp(mc), vp(q), int(uniform_quality), offsets.size - 1, C.byref(r))
        return cls._adopt(spectrum, b"", r)

    def twobit(self):
        """(packed bases, offsets[n+1], markup positions, markup chars, markup offsets[n+1]): every read as
        TwoBitSequence::compressSequence packs it (src/TwoBitSequence.cpp:242-269), on the device"""
        nb, nm = C.c_uint64(), C.c_uint64()
        u64 = C.POINTER(C.c_uint64)
        self.sp._call("reads_twobit", self.sp.h, self.r, None, 0, None, None, None, 0, None, C.byref(nb), C.byref(nm))
        tw = np.zeros(max(1, nb.value), dtype=np.uint8)
        to = np.zeros(self.n + 1, dtype=np.uint64)
        mp = np.zeros(max(1, nm.value), dtype=np.uint32)
        mc = np.zeros(max(1, nm.value), dtype=np.uint8)
        mo = np.zeros(self.n + 1, dtype=np.uint64)
        self.sp._call("reads_twobit", self.sp.h, self.r, tw.ctypes.data_as(C.c_void_p), tw.size, to.ctypes.data_as(u64), mp.ctypes.data_as(C.POINTER(C.c_uint32)),
                      mc.ctypes.data_as(C.c_void_p), mp.size, mo.ctypes.data_as(u64), C.byref(nb), C.byref(nm))
        return tw[:nb.value], to, mp[:nm.value], mc[:nm.value], mo

    def getSize(self):
        return self.n

    def arrays(self):
        """(bases, quals, offsets, names) on the host"""
        b = np.zeros(self.total_bases, dtype=np.uint8)
        q = np.zeros(self.total_bases, dtype=np.uint8)
        o = np.zeros(self.n + 1, dtype=np.uint64)
        no = np.zeros(max(1, self.n), dtype=np.uint64)
        nl = np.zeros(max(1, self.n), dtype=np.uint32)
        _ok(self.sp.lib.kmr_reads_copy(self.r, b.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        no.ctypes.data_as(C.POINTER(C.c_uint64)), nl.ctypes.data_as(C.POINTER(C.c_uint32))), "kmr_reads_copy")
        names = [self.text[int(no[i]):int(no[i]) + int(nl[i])] for i in range(self.n)]
        return b, q, o, names

    def circularize(self, extra=None):
        """ReadSet::circularize (src/ReadSet.cpp:120-130) as a new set: every read becomes bases + bases[0 : min(extra, L)], its
        qualities extended alike, its name kept (kmr_reads_circularize).  `extra` defaults to k, which CompareSpectrums
        --circular-reference passes: the first k-mer of a circular sequence is then counted twice, as in the reference."""
        r = C.c_void_p()
        self.sp._call("reads_circularize", self.sp.h, self._live(), self.sp.k if extra is None else int(extra), C.byref(r))
        return ReadSet._adopt(self.sp, self.text, r, self.store_comment)

    # -- TnfDistance (apps/TnfDistance.cpp)
    @staticmethod
    def _starts(input_starts):
        if input_starts is None:
            return None, 0
        s = np.ascontiguousarray(input_starts, dtype=np.uint64)
        return s, s.size - 1

    def tnf(self, input_starts=None):
        """buildTnfs (:462-484): one vector of canonical k-mer counts per sequence, k the spectrum's (kmr_tnf_reads): a TnfVectors
        whose groups are the inputs (`input_starts`: n_inputs + 1 ascending sequence indices; None = one input)"""
        s, n = self._starts(input_starts)
        out = C.c_void_p()
        self.sp._call("tnf_reads", self.sp.h, self._live(), None if s is None else s.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(out))
        return TnfVectors(self.sp, out)

    def tnfWindows(self, window, step, min_count=None, input_starts=None):
        """shredReadByWindow and purgeShortTNFS (:486-518): one vector per window of `window` bases every `step` bases that holds at
        least `min_count` k-mers (default window * 3 // 4, what the tool passes), in input order (kmr_tnf_windows)"""
        s, n = self._starts(input_starts)
        out = C.c_void_p()
        self.sp._call("tnf_windows", self.sp.h, self._live(), None if s is None else s.ctypes.data_as(C.POINTER(C.c_uint64)), n, int(window), int(step),
                      int(window) * 3 // 4 if min_count is None else int(min_count), C.byref(out))
        return TnfVectors(self.sp, out)

    def tnfLikelihoods(self, input_starts=None, window=10000, step=1000, window2=0, step2=1000, bins=100, formula=0, max_samples=(1 << 63) - 1):
        """the four histograms of --intra-inter-file (:664-902; kmr_tnf_likelihoods): a uint64 array [4][bins + 2] of intra, inter,
        intra-vs-whole and inter-vs-whole, outlier bins first and last"""
        s, n = self._starts(input_starts)
        cfg = _lib.KmrTnfLikelihoodConfig()
        _ok(self.sp.lib.kmr_tnf_likelihood_config_init(C.byref(cfg)), "kmr_tnf_likelihood_config_init")
        cfg.window, cfg.step, cfg.window2, cfg.step2, cfg.bins, cfg.formula, cfg.max_samples = int(window), int(step), int(window2), int(step2), int(bins), int(formula), int(max_samples)
        out = np.zeros((4, int(bins) + 2), dtype=np.uint64)
        self.sp._call("tnf_likelihoods", self.sp.h, self._live(), None if s is None else s.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def identifyPairs(self, store_comment=None, device_text=None):
        """ReadSet::identifyPairs (src/ReadSet.cpp:446-570) of this batch as a fresh set, on the device (kmr_identify_pairs): a
        ReadPairs.  `store_comment` defaults to what the batch was ingested with; `device_text` = device pointer of the FASTQ
        text if the caller holds it there (kmr_identify_pairs_dev)."""
        sc = self.store_comment if store_comment is None else bool(store_comment)
        out = C.c_void_p()
        if device_text is not None:
            self.sp._call("identify_pairs_dev", self.sp.h, self.r, C.c_void_p(device_text), len(self.text), 1 if sc else 0, C.byref(out))
        else:
            buf = np.frombuffer(self.text, dtype=np.uint8)
            self.sp._call("identify_pairs", self.sp.h, self.r, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, 1 if sc else 0, C.byref(out))
        return ReadPairs(self.sp, out)



def tnf_dims(k):
    """D(k), the number of canonical k-mers (kmr_tnf_dims)"""
    d = C.c_uint32()
    _ok(_lib.load().kmr_tnf_dims(int(k), C.byref(d)), "kmr_tnf_dims")
    return d.value


def tnf_columns(k, hash_kind=0):
    """column -> 2k-bit code of its canonical k-mer, in the iteration order of the reference's TNF::stdMap (kmr_tnf_columns)"""
    codes = np.zeros(tnf_dims(k), dtype=np.uint16)
    _ok(_lib.load().kmr_tnf_columns(int(k), int(hash_kind), codes.ctypes.data_as(C.POINTER(C.c_uint16))), "kmr_tnf_columns")
    return codes


def tnf_header(k, hash_kind=0):
    """TNF::toHeader (:295-303) as bytes (kmr_tnf_header)"""
    buf = C.create_string_buffer(16 + (int(k) + 1) * tnf_dims(k))
    nb = C.c_uint64()
    _ok(_lib.load().kmr_tnf_header(int(k), int(hash_kind), buf, len(buf), C.byref(nb)), "kmr_tnf_header")
    return buf.raw[:nb.value]


class TnfVectors(_DeviceObject):
    """Vectors of canonical k-mer counts on the device (kmr_tnf): .n vectors of .dims columns in .n_groups groups; .inexact = the
    columns above 2^24, where the reference's float no longer holds the count (its figures are followed while that is 0)."""
    _HANDLE, _FREE = "_t", "kmr_tnf_free"

    def __init__(self, sp, handle):
        self.sp, self._t = sp, handle
        n, d, g, bad = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _ok(sp.lib.kmr_tnf_info(handle, C.byref(n), C.byref(d), C.byref(g), C.byref(bad)), "kmr_tnf_info")
        self.n, self.dims, self.n_groups, self.inexact = n.value, d.value, g.value, bad.value

    def _copy(self, counts=None, lengths=None, origin=None, groups=None):
        p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
        _ok(self.sp.lib.kmr_tnf_copy(self._live(), p(counts, C.c_uint64), p(lengths, C.c_float), p(origin, C.c_uint64), p(groups, C.c_uint64)), "kmr_tnf_copy")

    def counts(self):
        """uint64 [n][dims], columns in tnf_columns order"""
        a = np.zeros((self.n, self.dims), dtype=np.uint64)
        self._copy(counts=a)
        return a

    def lengths(self):
        """float32 [n]: buildLength (:396-416)"""
        a = np.zeros(self.n, dtype=np.float32)
        self._copy(lengths=a)
        return a

    def origin(self):
        """uint64 [n][3]: the sequence a vector came from, its first base, its bases"""
        a = np.zeros((self.n, 3), dtype=np.uint64)
        self._copy(origin=a)
        return a

    def groups(self):
        """uint64 [n_groups + 1]: group g holds the vectors [groups[g], groups[g + 1])"""
        a = np.zeros(self.n_groups + 1, dtype=np.uint64)
        self._copy(groups=a)
        return a

    def groupSums(self):
        """one vector per group, its vectors added (wholeTnfs, :717; kmr_tnf_group_sums)"""
        out = C.c_void_p()
        self.sp._call("tnf_group_sums", self.sp.h, self._live(), C.byref(out))
        return TnfVectors(self.sp, out)

    def distances(self, other=None, formula=0, first_row=0, n_rows=None):
        """getDistance (:434-446) of rows [first_row, first_row + n_rows) of this set, to the reference's bits (kmr_tnf_distances):
        against every vector of `other` as a float32 [n_rows][other.n], or with other None the strict lower triangle, row i holding
        j < i, as one packed float32 array.  formula 0 = Euclidean, 1 = Spearman."""
        n_rows = self.n - first_row if n_rows is None else int(n_rows)
        if other is not None:
            out = np.zeros((n_rows, other.n), dtype=np.float32)
        else:
            e = first_row + n_rows
            out = np.zeros(e * (e - 1) // 2 - first_row * (first_row - 1) // 2 if e else 0, dtype=np.float32)
        self.sp._call("tnf_distances", self.sp.h, self._live(), None if other is None else other._live(), int(formula), int(first_row), n_rows,
                      out.ctypes.data_as(C.POINTER(C.c_float)) if out.size else None)
        return out


def _ostream(x):
    """a float or double as an ostream prints it by default: %g of the value widened to double (a NaN with its sign, as glibc does)"""
    x = float(x)
    if x != x:
        return b"-nan" if np.signbit(x) else b"nan"
    return ("%g" % x).encode()


def TnfDistance(read_set, input_starts=None, reference=None, inter_distance=False, intra_inter=None, formula=0):
    """apps/TnfDistance.cpp's texts as a dict of bytes, computed on the device and formatted here:
      "output"          the default table ("Label\\t" + header, then name, count, length and value / length per sequence, :636-646) or, with a
                        ReadSet `reference`, the distance of every sequence to the reference's one vector as "distance\\tname" lines ordered by
                        distance, then by sequence (:621-634; the reference's std::sort leaves ties open)
      "inter_distance"  with inter_distance: the lower triangle of distances, one line per sequence (:649-662)
      "intra_inter"     with intra_inter = dict(window, step, window2, step2, bins, max_samples), all optional: the likelihood table (:664-902)
    Not built: --cluster-file, the .data files, the five-part labels of sequences within 0.20 of the reference, subsampling."""
    sp = read_set.sp
    hash_kind = int(sp.cfg.hash_kind)
    names = read_set.arrays()[3]
    out = {}
    with read_set.tnf(input_starts) as t:
        if reference is not None:
            with reference.tnf() as rt, rt.groupSums() as ref:
                d = t.distances(ref, formula)[:, 0] if t.n else np.zeros(0, dtype=np.float32)
            order = sorted(range(t.n), key=lambda i: (float(d[i]), i))
            out["output"] = b"".join(_ostream(d[i]) + b"\t" + names[i] + b"\n" for i in order)
        else:
            cnt, ln = t.counts(), t.lengths()
            lines = [b"Label\t" + tnf_header(sp.k, hash_kind) + b"\n"]
            for i in range(t.n):
                v = cnt[i].astype(np.float32)
                lines.append(names[i] + b"\t" + _ostream(np.float64(v.astype(np.float64).sum())) + b"\t" + _ostream(ln[i]) + b"".join(b"\t" + _ostream(x) for x in v / ln[i]) + b"\n")
            out["output"] = b"".join(lines)
        if inter_distance:
            tri = t.distances(None, formula)
            out["inter_distance"] = b"".join(names[i] + b"".join(b"\t" + _ostream(x) for x in tri[i * (i - 1) // 2:i * (i + 1) // 2]) + b"\n" for i in range(t.n))
    if intra_inter is not None:
        o = dict(window=10000, step=1000, window2=0, step2=1000, bins=100, max_samples=(1 << 63) - 1)
        o.update(intra_inter)
        h = read_set.tnfLikelihoods(input_starts, formula=formula, **o)
        window2 = o["window"] if o["window2"] < o["window"] else o["window2"]
        bins = int(o["bins"])
        end = np.float32(np.sqrt(2.0)) if formula == 0 else np.float32(1.0)
        step = np.float32(end / np.float32(bins))
        tot = [float(int(h[j, 1:bins + 1].sum())) for j in range(4)]
        lines = [b"Distance\twindow\twindow2\tIntraLikelihood\tInterLikelihood\tIntraVsWholeLikelihood\tInterVsWholeLikelihood\n"]
        for i in range(bins):
            start = np.float32(np.float32(0.0) + np.float32(i) * step)
            lines.append(_ostream(start) + b"\t%d\t%d" % (int(o["window"]), int(window2)) + b"".join(b"\t" + (_ostream(int(h[j, i + 1]) / tot[j]) if tot[j] else b"-nan") for j in range(4)) + b"\n")
        out["intra_inter"] = b"".join(lines)
    return out


class ReadPairs(_DeviceObject):
    """What ReadSet.identifyPairs found (kmr_pairs), kept on the device until close(): .mate[i] = the read paired with i or -1 (what
    FilterKnownOddities.applyFilter(mate=) and ReadSelector(mate=) take), .pairs = the reference's pair list as an (n_pairs, 2)
    int64 array of (read1, read2) with -1 for a missing side, and the counts n_reads, n_pairs, n_full, n_sequential, n_conflicts."""
    _HANDLE, _FREE = "_p", "kmr_pairs_free"

    def __init__(self, sp, handle):
        self.sp, self._p = sp, handle
        v = [C.c_uint64() for _ in range(5)]
        hp = C.c_int()
        _ok(sp.lib.kmr_pairs_info(handle, *[C.byref(x) for x in v], C.byref(hp)), "kmr_pairs_info")
        self.n_reads, self.n_pairs, self.n_full, self.n_sequential, self.n_conflicts = [x.value for x in v]
        self._has_pairs = bool(hp.value)
        self._host = None

    def _copy(self):
        if self._host is None:
            i64 = C.POINTER(C.c_int64)
            mate = np.zeros(max(1, self.n_reads), dtype=np.int64)
            r1 = np.zeros(max(1, self.n_pairs), dtype=np.int64)
            r2 = np.zeros(max(1, self.n_pairs), dtype=np.int64)
            _ok(self.sp.lib.kmr_pairs_copy(self._live(), mate.ctypes.data_as(i64), r1.ctypes.data_as(i64), r2.ctypes.data_as(i64)), "kmr_pairs_copy")
            self._host = (mate[:self.n_reads], np.stack([r1[:self.n_pairs], r2[:self.n_pairs]], axis=1))
        return self._host

    @property
    def mate(self):
        return self._copy()[0]

    @property
    def pairs(self):
        return self._copy()[1]

    def getPairSize(self):
        return self.n_pairs

    def hasPairs(self):
        """ReadSet::hasPairs (src/ReadSet.h:526-529): 0 < pairs < reads"""
        return self._has_pairs

    def device_ptrs(self):
        """device pointers of (mate[n_reads], read1[n_pairs], read2[n_pairs]), int64 each; valid until close()"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _ok(self.sp.lib.kmr_pairs_device_ptrs(self._live(), C.byref(a), C.byref(b), C.byref(c)), "kmr_pairs_device_ptrs")
        return a.value or 0, b.value or 0, c.value or 0


class MatchResults:
    """What KmerMatch.finish() answers: for contig i the ascending global read indices reads[offsets[i]:offsets[i + 1]] (= self[i]),
    and per contig the size of its hit set before the sampling and after it (before the mates join)."""

    def __init__(self, offsets, reads, size_before_sampling, size_after_sampling, n_sampled_contigs=0):
        self.offsets, self.reads = offsets, reads
        self.size_before_sampling, self.size_after_sampling, self.n_sampled_contigs = size_before_sampling, size_after_sampling, n_sampled_contigs

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        return self.reads[int(self.offsets[i]):int(self.offsets[i + 1])]


class KmerMatch(_DeviceObject):
    """KmerMatch (src/KmerMatch.h:93-185, src/MatcherInterface.h): for every contig of the ReadSet `contigs` the reads that share a
    k-mer with the first or last `match_max_positions_from_edge` bases of the contig (kmr_match_*).  `spectrum` is the finalized
    spectrum of exactly the reads that are then streamed with addReads; sets of more than 2 * max_read_matches reads are sampled
    (0 = never), the random numbers a function of (seed, global read index, contig) alone; with `include_mate` the mates of the reads
    that stay join, where addReads is given the batch's ReadPairs."""
    _HANDLE, _FREE = "_m", "kmr_match_free"

    def __init__(self, spectrum, contigs, match_max_positions_from_edge=500, max_read_matches=450, include_mate=True, seed=0):
        self.sp = spectrum
        cfg = _lib.KmrMatchConfig()
        _ok(spectrum.lib.kmr_match_config_init(C.byref(cfg)), "kmr_match_config_init")
        cfg.max_positions_from_edge, cfg.max_read_matches, cfg.include_mate, cfg.seed = int(match_max_positions_from_edge), int(max_read_matches), 1 if include_mate else 0, int(seed)
        m = C.c_void_p()
        spectrum._call("match_create", spectrum.h, contigs._live(), C.byref(cfg), C.byref(m))
        self._m = m
        v = [C.c_uint64() for _ in range(4)]
        _ok(spectrum.lib.kmr_match_edge_info(m, *[C.byref(x) for x in v]), "kmr_match_edge_info")
        self.n_contigs, self.n_edge_kmers, self.n_distinct_keys, self.n_keys_in_spectrum = [x.value for x in v]

    def addReads(self, read_set, first_global_read_idx=0, pairs=None, discarded=None):
        """stream one batch of the target reads; `pairs`: the batch's ReadPairs (None: no mates), `discarded`: one flag per read"""
        d = None if discarded is None else _u8(discarded)
        if d is not None and d.size != read_set.n:
            raise KmerSpectrumError("KmerMatch.addReads: one discard flag per read")
        self.sp._call("match_add_read_batch", self._live(), read_set._live(), int(first_global_read_idx), None if pairs is None else pairs._live(),
                      None if d is None or not d.size else d.ctypes.data_as(C.POINTER(C.c_uint8)))
        return self

    def finish(self):
        """sample, add the mates, sort, drop the discarded reads: a MatchResults"""
        m = self._live()
        self.sp._call("match_finish", m)
        v = [C.c_uint64() for _ in range(3)]
        self.sp._call("match_info", m, *[C.byref(x) for x in v])
        nc, nr, ns = [x.value for x in v]
        off, ids = np.zeros(nc + 1, dtype=np.uint64), np.zeros(nr, dtype=np.uint64)
        before, after = np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        self.sp._call("match_copy", m, off.ctypes.data_as(u64), ids.ctypes.data_as(u64) if nr else None, before.ctypes.data_as(u64) if nc else None, after.ctypes.data_as(u64) if nc else None)
        return MatchResults(off, ids, before, after, ns)

    def device_ptrs(self):
        """device pointers of (offsets, reads, size_before_sampling, size_after_sampling), uint64 each; after finish(), valid until close()"""
        p = [C.c_void_p() for _ in range(4)]
        self.sp._call("match_device_ptrs", self._live(), *[C.byref(x) for x in p])
        return tuple(x.value or 0 for x in p)


# one kmr_extend_stop: why a side of a contig stopped and the f64 values of the last step it tried
EXTEND_STOP_DTYPE = np.dtype([("reason", np.uint32), ("reserved", np.uint32), ("edge", np.float64), ("ext", np.float64, (4,)), ("total", np.float64)])
MAX_KMER_SIZE = 128      # the library's longest k-mer
_FASTA = bytes((c & 0xDF) if chr(c) in "acgt" else (ord("N") if c == ord(".") else c) for c in range(256))      # Read::getFasta of a stored base


def _sequences(read_set):
    b, _, o, _ = read_set.arrays()
    return [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(read_set.n)]


class ExtendResults(_DeviceObject):
    """What ContigExtender.extendContigs answers (kmr_extend), kept on the device until close(): .read_set = the new sequences, every
    quality Read::REF_QUAL, as a ReadSet that KmerMatch and a further extendContigs take (it lives as long as this object);
    .names (ContigExtender.getNewName of the names handed in), .left / .right = bases added per contig, .new_len, .stops = an
    (n, 2) array of EXTEND_STOP_DTYPE, left and right; .n_extended, .bases_added."""
    _HANDLE, _FREE = "_e", "kmr_extend_free"

    def __init__(self, sp, handle, names):
        self.sp, self._e = sp, handle
        v = [C.c_uint64() for _ in range(3)]
        _ok(sp.lib.kmr_extend_info(handle, *[C.byref(x) for x in v]), "kmr_extend_info")
        self.n, self.n_extended, self.bases_added = [x.value for x in v]
        n1 = max(1, self.n)
        nl, lt, rt = np.zeros(n1, dtype=np.uint32), np.zeros(n1, dtype=np.uint32), np.zeros(n1, dtype=np.uint32)
        st = np.zeros((n1, 2), dtype=EXTEND_STOP_DTYPE)
        u32 = C.POINTER(C.c_uint32)
        _ok(sp.lib.kmr_extend_copy(handle, nl.ctypes.data_as(u32), lt.ctypes.data_as(u32), rt.ctypes.data_as(u32), st.ctypes.data_as(C.POINTER(_lib.KmrExtendStop))), "kmr_extend_copy")
        self.new_len, self.left, self.right, self.stops = nl[:self.n], lt[:self.n], rt[:self.n], st[:self.n]
        r = C.c_void_p()
        _ok(sp.lib.kmr_extend_reads(handle, C.byref(r)), "kmr_extend_reads")
        self.read_set = ConsensusReadSet._borrow(self, sp, b"", r)
        self.names = None if names is None else [ContigExtender.getNewName(nm, int(l), int(r_)) for nm, l, r_ in zip(names, self.left, self.right)]

    def sequences(self):
        """the new sequences as a list of bytes"""
        return _sequences(self.read_set)

    def close(self):
        if getattr(self, "_e", None):
            self.read_set.r = None
        super().close()


class ContigExtender:
    """ContigExtender<KS>::extendContigs at one k-mer size (src/ContigExtender.h:157-247 with minKmerSize == maxKmerSize, over
    KmerSpectrum::extendContig, src/KmerSpectrum.h:2311-2373), every contig with its own pool of reads, all at once on the device
    (kmr_extend_*).  `spectrum` supplies k and the build's config -- min_weight, qualities, separate_singletons -- and need not have
    been fed.  Options: max_extend (50), minimum_consensus in percent (85), minimum_coverage (4.8), maximum_delta_ratio (0.33),
    use_weights (True)."""

    def __init__(self, spectrum, max_extend=50, minimum_consensus=85.0, minimum_coverage=4.8, maximum_delta_ratio=0.33, use_weights=True):
        self.sp = spectrum
        cfg = _lib.KmrExtendConfig()
        _ok(spectrum.lib.kmr_extend_config_init(C.byref(cfg)), "kmr_extend_config_init")
        cfg.max_extend, cfg.minimum_consensus, cfg.minimum_coverage = int(max_extend), float(minimum_consensus), float(minimum_coverage)
        cfg.maximum_delta_ratio, cfg.use_weights = float(maximum_delta_ratio), 1 if use_weights else 0
        self.cfg = cfg

    @staticmethod
    def _pools(pools, first_global_read_idx):
        if isinstance(pools, MatchResults):
            return np.ascontiguousarray(pools.offsets, dtype=np.uint64), np.ascontiguousarray(pools.reads, dtype=np.uint64) - np.uint64(first_global_read_idx)
        off, idx = pools
        return np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(idx, dtype=np.uint64)

    def extendContigs(self, contigs, read_set, pools, names=None, active=None, first_global_read_idx=0):
        """`pools`: a MatchResults (its global read indices less `first_global_read_idx` index `read_set`) or an (offsets, indices)
        pair; `names`: the contigs' names, for ExtendResults.names; `active`: one flag per contig, 0 = leave it as it is"""
        off, idx = self._pools(pools, first_global_read_idx)
        if off.size != contigs.n + 1:
            raise KmerSpectrumError("ContigExtender.extendContigs: one pool per contig")
        a = None if active is None else _u8(active)
        if a is not None and a.size != contigs.n:
            raise KmerSpectrumError("ContigExtender.extendContigs: one active flag per contig")
        u64 = C.POINTER(C.c_uint64)
        e = C.c_void_p()
        self.sp._call("extend_contigs", self.sp.h, contigs._live(), read_set._live(), off.ctypes.data_as(u64), idx.ctypes.data_as(u64) if idx.size else None,
                      None if a is None or not a.size else a.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(self.cfg), C.byref(e))
        return ExtendResults(self.sp, e, names)

    def extendContigsDevice(self, contigs, read_set, dev_offsets, dev_indices, names=None, dev_active=0):
        """the same with the pools (uint64 offsets, uint64 indices into `read_set`) and the flags as device pointers, e.g. KmerMatch.device_ptrs()"""
        e = C.c_void_p()
        self.sp._call("extend_contigs_dev", self.sp.h, contigs._live(), read_set._live(), C.c_void_p(dev_offsets), C.c_void_p(dev_indices or None), C.c_void_p(dev_active or None),
                      C.byref(self.cfg), C.byref(e))
        return ExtendResults(self.sp, e, names)

    @staticmethod
    def getNewName(old_name, left_total, right_total):
        """ContigExtender::getNewName (src/ContigExtender.h:249-268) through kmr_extend_new_name; bytes in, bytes out"""
        old = old_name.encode() if isinstance(old_name, str) else bytes(old_name)
        buf = C.create_string_buffer(len(old) + 48)
        _ok(_lib.load().kmr_extend_new_name(old, int(left_total), int(right_total), buf, len(buf)), "kmr_extend_new_name")
        return buf.value

    @staticmethod
    def getMinMaxKmerSize(kmer_size, max_sequence_length, base_count, n_reads, max_steps=6):
        """ContigExtender::getMinMaxKmerSize (:269-279): (min_kmer_size, max_kmer_size, kmer_step)"""
        v = [C.c_uint32() for _ in range(3)]
        _ok(_lib.load().kmr_extend_min_max_kmer_size(int(kmer_size), int(max_sequence_length), int(base_count), int(n_reads), int(max_steps), *[C.byref(x) for x in v]),
            "kmr_extend_min_max_kmer_size")
        return tuple(x.value for x in v)


class ExtendRound(tuple):
    """(changed, final, log text) of extendContigsWithContigExtender -- changed and final are lists of (name, sequence) --, and
    .skipped_k: the k-mer sizes of the sweep that the library does not reach"""

    def __new__(cls, changed, final, log, skipped_k):
        self = super().__new__(cls, (changed, final, log))
        self.skipped_k = skipped_k
        return self


def extendContigsWithContigExtender(make_spectrum, contigs, names, read_set, pools, min_kmer_size, max_kmer_size, kmer_step, minimum_coverage=4.8, max_extend=50,
                                    first_global_read_idx=0, **options):
    """extendContigsWithContigExtender (apps/DistributedNucleatingAssembler.cpp:230-275): every contig whose pool holds more than
    `minimum_coverage` reads is extended at min_kmer_size, and again at the next k-mer size -- from its original sequence -- while it
    has not grown and the size is not above max_kmer_size.  One never-fed spectrum per k-mer size comes from make_spectrum(k); a pass
    works on all contigs that have not grown at once, the others are switched off through `active`.  Sizes above 128, the library's
    longest k-mer, are skipped (ExtendRound.skipped_k): for 150-base reads the reference's sweep would reach 142.
    Returns (changed, final, log text) as the reference fills and logs them."""
    off, _ = ContigExtender._pools(pools, first_global_read_idx)
    nc = contigs.n
    names = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in names]
    seqs = _sequences(contigs)
    pool_size = [int(off[i + 1]) - int(off[i]) for i in range(nc)]
    old_len = [len(s) for s in seqs]
    new_len = [0] * nc
    new_seq, new_name, used_k = list(seqs), list(names), [0] * nc
    active = np.array([1 if pool_size[i] > minimum_coverage else 0 for i in range(nc)], dtype=np.uint8)
    skipped = []
    k = int(min_kmer_size)
    while k <= max_kmer_size and active.any():
        if k > MAX_KMER_SIZE:
            skipped.append(k)
        else:
            sp = make_spectrum(k)
            with ContigExtender(sp, max_extend=max_extend, minimum_coverage=minimum_coverage, **options).extendContigs(
                    contigs, read_set, pools, names=names, active=active, first_global_read_idx=first_global_read_idx) as res:
                rs = res.sequences()
                for i in range(nc):
                    if active[i]:
                        new_len[i], new_seq[i], new_name[i], used_k[i] = len(rs[i]), rs[i], res.names[i], k
                        if new_len[i] > old_len[i]:
                            active[i] = 0
        k += int(kmer_step)
    changed, final, log = [], [], []
    for i in range(nc):
        delta = new_len[i] - old_len[i]
        if delta > 0:
            log.append(b"\nKmer Extended %s %d bases to %d: %s with %d reads in the pool K %d" % (names[i], delta, new_len[i], new_name[i], pool_size[i], used_k[i]))
            changed.append((new_name[i], new_seq[i]))
        else:
            log.append(b"\nDid not extend %s with %d reads in the pool" % (names[i], pool_size[i]))
            final.append((names[i], seqs[i].translate(_FASTA)))
    return ExtendRound(changed, final, b"".join(log), skipped)


def finishLongContigs(max_contig_length, changed, final):
    """finishLongContigs (apps/DistributedNucleatingAssembler.cpp:277-288): the changed contigs of at least max_contig_length bases move
    to the end of `final`; returns the (changed, final) lists that remain"""
    keep = []
    final = list(final)
    for name, seq in changed:
        (final if len(seq) >= max_contig_length else keep).append((name, seq))
    return keep, final


class FilterKnownOddities(_DeviceObject):
    """The artifact filter FilterReads runs before the spectrum build (src/FilterKnownOddities.h, apps/FilterReads.cpp:107-118):
    quality-run trimming plus a screen of every 4th 24-mer of a read against the artifact sequences (and their substitution
    neighbours), on the device.  `fasta` = the sequences as FASTA text (the reference embeds its own table); keyword
    arguments are the fields of kmr_artifact_config (edit_distance, min_quality, fastq_start_char, min_read_length, ...)."""
    _HANDLE, _FREE = "f", "kmr_artifact_filter_free"

    def __init__(self, spectrum, fasta, **kw):
        self.sp = spectrum
        cfg = _lib.KmrArtifactConfig()
        spectrum.lib.kmr_artifact_config_init(C.byref(cfg))
        cfg.fastq_start_char = spectrum.cfg.fastq_start_char
        cfg.min_quality = spectrum.cfg.min_quality_score
        for name, v in kw.items():
            if not hasattr(cfg, name):
                raise TypeError("unknown artifact filter option %r" % name)
            setattr(cfg, name, v)
        self.cfg = cfg
        fasta = bytes(fasta)
        f = C.c_void_p()
        spectrum._call("artifact_filter_create", spectrum.h, C.byref(cfg), fasta, len(fasta), C.byref(f))
        self.f = f
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        spectrum.lib.kmr_artifact_filter_info(self.f, C.byref(a), C.byref(b), C.byref(c))
        self.n_sequences, self.n_filter_kmers, self.remaining_edits = a.value, b.value, c.value

    def entries(self):
        keys = np.zeros(self.n_filter_kmers, dtype=np.uint64)
        vals = np.zeros(self.n_filter_kmers, dtype=np.uint32)
        _ok(self.sp.lib.kmr_artifact_filter_entries(self.f, keys.ctypes.data_as(C.POINTER(C.c_uint64)), vals.ctypes.data_as(C.POINTER(C.c_uint32)), keys.size), "kmr_artifact_filter_entries")
        return keys, vals

    def applyFilter(self, reads, mate=None, want_reads=True, report=False, pairs=None, **report_options):
        """applyFilter(ReadSet&) (:663-733).  Returns (results, filtered ReadSet): results = dict of per-read arrays value,
        min_pass, max_pass, action (0 untouched / 1 trimmed / 2 discarded), remnant_off, remnant_len; the new ReadSet holds the
        trimmed reads in place and the rescued remnants behind them.  report=True: the fused form (applyFilterReport) over the
        pair list `pairs` in place of `mate`, with its options; returns (results, filtered ReadSet, FilterReport)."""
        if report:
            if mate is not None:
                raise KmerSpectrumError("applyFilter(report=True) takes the pair list (pairs=), not mate")
            return self.applyFilterReport(reads, pairs=pairs, want_reads=want_reads, **report_options)
        n = reads.n
        res = {k: np.zeros(max(1, n), dtype=np.uint32) for k in ("value", "min_pass", "max_pass", "remnant_off", "remnant_len")}
        res["action"] = np.zeros(max(1, n), dtype=np.uint8)
        u32 = C.POINTER(C.c_uint32)
        m = None
        if mate is not None:
            mate = np.ascontiguousarray(mate, dtype=np.int64)
            assert mate.size == n
            m = mate.ctypes.data_as(C.POINTER(C.c_int64))
        out = C.c_void_p()
        self.sp._call("artifact_filter_apply", self.sp.h, self.f, reads.r, m, res["value"].ctypes.data_as(u32), res["min_pass"].ctypes.data_as(u32),
                      res["max_pass"].ctypes.data_as(u32), res["action"].ctypes.data_as(C.POINTER(C.c_uint8)), res["remnant_off"].ctypes.data_as(u32),
                      res["remnant_len"].ctypes.data_as(u32), C.byref(out) if want_reads else None)
        res = {k: v[:n] for k, v in res.items()}
        return res, (ReadSet._adopt(self.sp, reads.text, out, getattr(reads, "store_comment", True)) if want_reads else None)

    def getFilterName(self, idx):
        """getFilterName (:543-550): the header name of sequence idx in [1, n_sequences), "MinQualityTrim<q>" for n_sequences"""
        buf = C.create_string_buffer(4096)
        _ok(self.sp.lib.kmr_artifact_filter_name(self._live(), int(idx), buf, len(buf)), "kmr_artifact_filter_name")
        return buf.value.decode()

    def _report_config(self, artifact_output, phix_output, output_quality_base, print_bases):
        cfg = _lib.KmrArtifactReportConfig()
        self.sp.lib.kmr_artifact_report_config_init(C.byref(cfg))
        cfg.artifact_output, cfg.phix_output = (1 if artifact_output else 0), (1 if phix_output else 0)
        cfg.output_quality_base, cfg.print_bases = int(output_quality_base), (1 if print_bases else 0)
        return cfg

    @staticmethod
    def _pair_args(pairs):
        """pairs (a ReadPairs, or (read1, read2) arrays with -1 for a missing side, or None) as (the arrays, their pointers, n_pairs)"""
        if pairs is None:
            return None, (None, None), 0
        if isinstance(pairs, ReadPairs):
            pairs = (pairs.pairs[:, 0], pairs.pairs[:, 1])
        r1, r2 = (np.ascontiguousarray(x, dtype=np.int64) for x in pairs)
        assert r1.size == r2.size
        i64 = C.POINTER(C.c_int64)
        return (r1, r2), (r1.ctypes.data_as(i64), r2.ctypes.data_as(i64)), r1.size

    def _report_call(self, name, reads, pairs, input_starts, device_text, cfg, *mid):
        """the arguments every reporting entry point shares around its own `mid`: returns the FilterReport"""
        keep, (p1, p2), n_pairs = self._pair_args(pairs)
        starts = None if input_starts is None else np.ascontiguousarray(input_starts, dtype=np.uint64)
        sp = None if starts is None else starts.ctypes.data_as(C.POINTER(C.c_uint64))
        buf = np.frombuffer(reads.text, dtype=np.uint8)
        text = C.c_void_p(device_text) if device_text is not None else (buf.ctypes.data_as(C.c_void_p) if buf.size else None)
        rep = C.c_void_p()
        self.sp._call(name + ("_dev" if device_text is not None else ""), self.sp.h, self._live(), reads.r, text, buf.size, p1, p2, n_pairs, *mid,
                      sp, 0 if starts is None else starts.size - 1, C.byref(cfg), C.byref(rep))
        return FilterReport(self, rep, reads.n)

    def report(self, read_set, results, pairs=None, input_starts=None, artifact_output=True, phix_output=None, output_quality_base=33, print_bases=False,
               device_text=None):
        """What the reference's Recorder makes of applyFilter's `results` for the batch `read_set` they were computed from
        (kmr_artifact_filter_report): a FilterReport with the -Artifact.fastq / -PhiX.fastq records and the per-sequence counters.
        pairs = the pair list (a ReadPairs or (read1, read2) arrays; None: every read on its own), input_starts as
        ReadSelector.selectReads takes them; phix_output defaults to whether the filter knows a PhiX sequence; print_bases writes
        the read's bases where the reference writes N; device_text = device pointer of the name text."""
        cfg = self._report_config(artifact_output, self.cfg.phix_idx != 0 if phix_output is None else phix_output, output_quality_base, print_bases)
        n = read_set.n
        arr = {k: np.ascontiguousarray(results[k], dtype=t) for k, t in (("value", np.uint32), ("action", np.uint8), ("min_pass", np.uint32), ("max_pass", np.uint32))}
        for a in arr.values():
            assert a.size == n
        u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        return self._report_call("artifact_filter_report", read_set, pairs, input_starts, device_text, cfg, arr["value"].ctypes.data_as(u32), arr["action"].ctypes.data_as(u8),
                                 arr["min_pass"].ctypes.data_as(u32), arr["max_pass"].ctypes.data_as(u32))

    def applyFilterReport(self, reads, pairs=None, input_starts=None, want_reads=True, want_results=True, artifact_output=True, phix_output=None, output_quality_base=33,
                          print_bases=False, device_text=None):
        """applyFilter and its report in one call that keeps the decisions on the device (kmr_artifact_filter_apply_report): returns
        (results, filtered ReadSet, FilterReport) with results and the ReadSet as applyFilter gives them (None where not wanted);
        the mate of every read follows from `pairs`."""
        cfg = self._report_config(artifact_output, self.cfg.phix_idx != 0 if phix_output is None else phix_output, output_quality_base, print_bases)
        n = reads.n
        res = None
        ptrs = [None] * 6
        if want_results:
            res = {k: np.zeros(max(1, n), dtype=np.uint32) for k in ("value", "min_pass", "max_pass", "remnant_off", "remnant_len")}
            res["action"] = np.zeros(max(1, n), dtype=np.uint8)
            u32 = C.POINTER(C.c_uint32)
            ptrs = [res["value"].ctypes.data_as(u32), res["min_pass"].ctypes.data_as(u32), res["max_pass"].ctypes.data_as(u32), res["action"].ctypes.data_as(C.POINTER(C.c_uint8)),
                    res["remnant_off"].ctypes.data_as(u32), res["remnant_len"].ctypes.data_as(u32)]
        out = C.c_void_p()
        rep = self._report_call("artifact_filter_apply_report", reads, pairs, input_starts, device_text, cfg, *ptrs, C.byref(out) if want_reads else None)
        if res is not None:
            res = {k: v[:n] for k, v in res.items()}
        return res, (ReadSet._adopt(self.sp, reads.text, out, getattr(reads, "store_comment", True)) if want_reads else None), rep


class FilterReport(_DeviceObject):
    """The artifact filter's report (kmr_artifact_report): .counts() = (discarded, trimmed, bases) per sequence index, .toString()
    the table applyFilter logs (:714-725), .files(output, input_prefixes) the (name, bytes) of every -Artifact.fastq / -PhiX.fastq
    file that holds a record, .device_text() the records where they were written.  .segments and .read_segment as a ReadSelector
    holds them: two rows (0 Artifact, 1 PhiX) times the inputs."""
    _HANDLE, _FREE = "_rep", "kmr_artifact_report_free"
    ROWS = ("-Artifact.fastq", "-PhiX.fastq")

    def __init__(self, flt, handle, n_reads):
        self.sp, self.filter, self._rep, self.n_reads = flt.sp, flt, handle, n_reads
        pk = C.c_void_p()
        _ok(self.sp.lib.kmr_artifact_report_picks(handle, C.byref(pk)), "kmr_artifact_report_picks")
        self._picks = pk
        n, b = C.c_uint64(), C.c_uint64()
        _ok(self.sp.lib.kmr_picks_info(pk, C.byref(n), C.byref(b)), "kmr_picks_info")
        self.n_records, self.bytes = n.value, b.value
        self._text = self._counts = None
        nr, ni = C.c_uint32(), C.c_uint32()
        _ok(self.sp.lib.kmr_picks_segments_info(pk, C.byref(nr), C.byref(ni)), "kmr_picks_segments_info")
        nr, ni = nr.value, ni.value
        cols = [np.zeros(max(1, nr * ni), dtype=np.uint64) for _ in range(4)]
        rseg = np.full(max(1, n_reads), -1, dtype=np.int32)
        p = ReadSelector._p
        _ok(self.sp.lib.kmr_picks_segments_copy(pk, None, None, *[p(c, C.c_uint64) for c in cols], p(rseg, C.c_int32)), "kmr_picks_segments_copy")
        self.segments = {k: c[:nr * ni].reshape(nr, ni) for k, c in zip(("first_pick", "picks", "first_byte", "bytes"), cols)}
        self.read_segment = rseg[:n_reads]

    def counts(self):
        """(discarded, trimmed, bases): uint64 arrays of n_sequences + 1 entries"""
        if self._counts is None:
            rows = self.filter.n_sequences + 1
            a = [np.zeros(rows, dtype=np.uint64) for _ in range(3)]
            _ok(self.sp.lib.kmr_artifact_report_counts(self._live(), *[ReadSelector._p(x, C.c_uint64) for x in a], rows), "kmr_artifact_report_counts")
            self._counts = tuple(a)
        return self._counts

    def toString(self):
        """the text applyFilter logs (:714-725)"""
        d, t, b = self.counts()
        s = "Final Filter Matches to reads:%d\nDiscarded Reads:%d\nTrimmed Reads:%d\nDiscarded/Trimmed Bases:%d\n\n\tDiscarded\tAffected\tBasesRemoved\tMatch\n" % (
            int(t.sum()), int(d.sum()), int(t.sum()), int(b.sum()))
        for i in range(d.size):
            if b[i] > 0:
                s += "\t%d\t%d\t%d\t%s\n" % (int(d[i]), int(t[i]), int(b[i]), self.filter.getFilterName(i))
        return s

    def text(self):
        """all records: the Artifact files input by input, then the PhiX files"""
        if self._text is None:
            buf = np.zeros(max(1, self.bytes), dtype=np.uint8)
            _ok(self.sp.lib.kmr_picks_copy(self._picks, buf.ctypes.data_as(C.c_void_p), self.bytes, None), "kmr_picks_copy")
            self._text = buf[:self.bytes].tobytes()
        return self._text

    def files(self, output="", input_prefixes=None):
        """(file name, bytes) as the reference's OfstreamMaps name them (:670-677): output + "-" + the input's prefix +
        "-Artifact.fastq" / "-PhiX.fastq", the Artifact files first; a file without a record is left out"""
        seg, text = self.segments, self.text()
        n_inputs = seg["picks"].shape[1]
        prefixes = list(input_prefixes) if input_prefixes is not None else ["transformed-%d" % (j + 1) for j in range(n_inputs)]
        if len(prefixes) != n_inputs:
            raise KmerSpectrumError("FilterReport.files: %d input_prefixes for %d inputs" % (len(prefixes), n_inputs))
        first, size = seg["first_byte"], seg["bytes"]
        return [("%s-%s%s" % (output, prefixes[j], self.ROWS[r]), text[int(first[r, j]):int(first[r, j]) + int(size[r, j])])
                for r in range(2) for j in range(n_inputs) if seg["picks"][r, j]]

    def device_text(self):
        """(device pointer, bytes) of the records (kmr_picks_device_ptr); valid until close()"""
        p = C.c_void_p()
        _ok(self.sp.lib.kmr_picks_device_ptr(self._picks, C.byref(p)), "kmr_picks_device_ptr")
        return p.value, self.bytes

    def close(self):
        self._picks = None      # borrowed from the report
        super().close()



class ReadSelector(_DeviceObject):
    """ReadSelector over a device-resident ReadSet (src/ReadSelector.h): scoreAndTrimReads (:1182-1207), pickAllPassingReads /
    pickAllPassingPairs (:576-596) and writePicks (:1242-1262), selection and text produced on the device (kmr_select_reads,
    kmr_filter_read_batch).  `mate` = index of each read's pair or -1 (None: every read is single); `filter_results` = the dict
    FilterKnownOddities.applyFilter returned for the batch `read_set` was made from (the remnants it appended count as single,
    untouched reads).  `pairs` = the pair list coverage normalization decides over (pickCoverageNormalizedSubset, selectReads with
    max_kmer_output_depth): a ReadPairs, or (read1, read2) arrays with -1 for a missing side; without it the list is the pairs of
    `mate`, and every read no pair names is a half pair.  The output text stays on the device until writePicks copies it."""

    _HANDLE, _FREE = "_picks", "kmr_picks_free"
    FORMAT = {"fastq": 0, "fasta": 1}

    def __init__(self, spectrum, read_set, mate=None, filter_results=None, pairs=None):
        self.sp, self.reads = spectrum, read_set
        n = read_set.n
        self.pairs, self.has_pairs = None, False
        if pairs is not None:
            found = pairs if isinstance(pairs, ReadPairs) else None
            if found is not None:
                pairs = (found.pairs[:, 0], found.pairs[:, 1])
            r1, r2 = (np.ascontiguousarray(x, dtype=np.int64) for x in pairs)
            assert r1.size == r2.size
            self.pairs = (r1, r2)
            self.has_pairs = found.hasPairs() if found is not None else 0 < r1.size < n      # ReadSet::hasPairs (src/ReadSet.h:526-529)
        elif mate is not None:
            m = np.full(n, -1, dtype=np.int64)
            m[:np.size(mate)] = np.asarray(mate, dtype=np.int64)
            first = np.nonzero(m > np.arange(n))[0].astype(np.int64)
            self.pairs = (first, np.ascontiguousarray(m[first]))
            self.has_pairs = first.size > 0
        self.mate = None
        if mate is not None:
            self.mate = np.full(n, -1, dtype=np.int64)
            m = np.ascontiguousarray(mate, dtype=np.int64)
            assert m.size <= n
            self.mate[:m.size] = m
        self.af = None
        if filter_results is not None:
            act = np.zeros(n, dtype=np.uint8); lo = np.zeros(n, dtype=np.uint32); hi = np.zeros(n, dtype=np.uint32)
            k = filter_results["action"].size
            assert k <= n
            act[:k] = filter_results["action"]; lo[:k] = filter_results["min_pass"]; hi[:k] = filter_results["max_pass"]
            self.af = (act, lo, hi)
        self.trims = None
        self.bimodal_words = None      # bimodal() of the scoreAndTrimReads that left the trims, if it ran with the option on
        self.scoring = "MEDIAN"
        self.device_text_of_reads = None      # set to (device pointer, bytes) of a copy of read_set.text: pickAllPassing* / writePicks read the names there
        self._picks = None
        self._sel = None
        self.picked_flags = np.zeros(n, dtype=bool)
        self.segments, self.read_segment = None, np.full(n, -1, dtype=np.int32)

    @staticmethod
    def _p(a, ct):
        return None if a is None else a.ctypes.data_as(C.POINTER(ct))

    def _config(self, min_score, min_read_length, both_pass, output_quality_base, format, scoring):
        cfg = _lib.KmrSelectConfig()
        self.sp.lib.kmr_select_config_init(C.byref(cfg))
        cfg.minimum_score = float(min_score)
        if min_read_length is not None:
            cfg.min_read_length = float(min_read_length)
        cfg.both_pass = 1 if both_pass else 0
        cfg.output_quality_base = int(output_quality_base)
        cfg.format = self.FORMAT[format] if isinstance(format, str) else int(format)
        cfg.scoring_type = KmerSpectrum.SCORING[scoring]
        return cfg

    def _text_args(self):
        buf = np.frombuffer(self.reads.text, dtype=np.uint8)
        return buf, (buf.ctypes.data_as(C.c_void_p) if buf.size else None), buf.size

    def _af_args(self):
        a = self.af or (None, None, None)
        return self._p(a[0], C.c_uint8), self._p(a[1], C.c_uint32), self._p(a[2], C.c_uint32)

    def _trim_args(self):
        """the trims scoreAndTrimReads left as the four array arguments of the unfused entry points: (the arrays, their pointers)"""
        keep = [np.ascontiguousarray(a, dtype=t) for a, t in zip(self.trims, (np.uint32, np.uint32, np.float32, np.uint8))]
        return keep, [self._p(a, ct) for a, ct in zip(keep, (C.c_uint32, C.c_uint32, C.c_float, C.c_uint8))]

    def _starts_args(self, input_starts):
        """input_starts (n_inputs + 1 read indices, or None) as (the array, its pointer, n_inputs)"""
        starts = None if input_starts is None else np.ascontiguousarray(input_starts, dtype=np.uint64)
        return starts, self._p(starts, C.c_uint64), 0 if starts is None else starts.size - 1

    def _files(self, text, seg, round_names, input_prefixes, suffix):
        """(file name, bytes) of every segment that holds a pick, round-major: round_names[r] + "-" + the input's prefix + suffix"""
        n_rounds, n_inputs = seg["picks"].shape
        prefixes = list(input_prefixes) if input_prefixes is not None else ["transformed-%d" % (j + 1) for j in range(n_inputs)]
        if len(prefixes) != n_inputs:
            raise KmerSpectrumError("selectReads: %d input_prefixes for %d inputs" % (len(prefixes), n_inputs))
        first, size = seg["first_byte"], seg["bytes"]
        return [(round_names[r] + "-" + prefixes[j] + suffix, text[int(first[r, j]):int(first[r, j]) + int(size[r, j])])
                for r in range(n_rounds) for j in range(n_inputs) if seg["picks"][r, j]]

    def _adopt(self, handle):
        self.close()
        self._picks = handle
        n, b = C.c_uint64(), C.c_uint64()
        self.sp.lib.kmr_picks_info(handle, C.byref(n), C.byref(b))
        self.n_picked, self.bytes = n.value, b.value
        self._text = None

    def scoreAndTrimReads(self, min_score, scoring="MEDIAN", bimodal_sigmas=-1.0):
        """ReadSelector::scoreAndTrimReads(minimumKmerScore): (trim_offset, trim_length, score, was_trimmed) per read.  With the
        bimodal cut on (bimodal_sigmas >= 0, or the spectrum's setBimodalSigmas) .bimodal_words keeps the tags for the selection
        that follows."""
        self.scoring = scoring
        self.trims = self.sp.scoreAndTrimReadSet(self.reads, min_score, scoring, bimodal_sigmas)
        self.bimodal_words = self.sp.bimodal(self.reads.n) if self.reads.n and self.sp.bimodal_active else None
        return self.trims

    def _tag_args(self):
        """hand the tags of the trims to the next host-array selection (kmr_select_bimodal); without tags, take back what is left"""
        w = self.bimodal_words
        self.sp._call("select_bimodal", self.sp.h, self._p(w, C.c_uint64), 0 if w is None else w.size)

    def _select(self, min_score, min_read_length, both_pass, by_pair=True):
        if self.trims is None:
            raise KmerSpectrumError("pickAllPassing*: scoreAndTrimReads has not run")
        self._sel = (min_score, min_read_length, both_pass, by_pair)
        return self._run(33, "fastq")

    def _run(self, output_quality_base, format):
        min_score, min_read_length, both_pass, by_pair = self._sel
        mate = self.mate if by_pair else None      # writePicks in another format selects again, as the pick did
        cfg = self._config(min_score, min_read_length, both_pass, output_quality_base, format, self.scoring)
        keep, tp, tn = self._text_args()
        trims, trim_ptrs = self._trim_args()
        self._tag_args()
        out = C.c_void_p()
        entry = "select_reads"
        if self.device_text_of_reads is not None:      # (device pointer, bytes) of the text the names point into: kmr_select_reads_dev
            entry, (tp, tn) = "select_reads_dev", self.device_text_of_reads
            tp = tp or None
        self.sp._call(entry, self.sp.h, self.reads.r, tp, tn, self._p(mate, C.c_int64), *self._af_args(), *trim_ptrs, C.byref(cfg), C.byref(out))
        self._adopt(out)
        self._fmt = (output_quality_base, cfg.format)
        return self.n_picked

    def pickAllPassingReads(self, min_score=0.0, min_read_length=None):
        """every read on its own, whatever `mate` says (:576-583); returns the number of picks"""
        return self._select(min_score, min_read_length, False, by_pair=False)

    def pickAllPassingPairs(self, min_score=0.0, min_read_length=None, both_pass=False):
        """:585-596 over the pairs of `mate`; returns the number of picked reads"""
        return self._select(min_score, min_read_length, both_pass)

    def filterReads(self, min_score=2.0, min_read_length=None, both_pass=False, scoring="MEDIAN", output_quality_base=33, format="fastq", bimodal_sigmas=-1.0):
        """scoreAndTrimReads + pickAllPassingPairs + writePicks in one call that keeps the trims on the device
        (kmr_filter_read_batch); returns the text.  bimodal_sigmas as scoreAndTrimReads takes it."""
        cfg = self._config(min_score, min_read_length, both_pass, output_quality_base, format, scoring)
        keep, tp, tn = self._text_args()
        out = C.c_void_p()
        with self.sp._bimodal_for(bimodal_sigmas, self.reads.n):
            self.sp._call("filter_read_batch", self.sp.h, self.reads.r, tp, tn, self._p(self.mate, C.c_int64), *self._af_args(), C.byref(cfg), C.byref(out))
        self._adopt(out)
        self._sel, self._fmt = None, (output_quality_base, cfg.format)
        return self._copy()

    SUFFIX = {0: ".fastq", 1: ".fasta"}

    def selectReads(self, min_depth, partition_by_depth=0, remainder_trim=-1.0, min_read_length=None, both_pass=False, scoring="MEDIAN",
                    output_quality_base=33, format="fastq", input_starts=None, input_prefixes=None, output="", separate_outputs=True,
                    max_kmer_output_depth=0, normalization_method="RANDOM", seed=0, first_read_idx=0, by_pair=None, bimodal_sigmas=-1.0):
        """selectReads (apps/FilterReads.h:159-279).  With --max-kmer-output-depth off: the rounds of --partition-by-depth and
        --remainder-trim over the reads of `input_starts` (n_inputs + 1 ascending read indices; None = one input), on the device
        (kmr_partition_read_batch, or kmr_partition_reads over the trims scoreAndTrimReads left).  Returns the ordered list of
        (file name, bytes) the reference writes: with separate_outputs `output` + "-MinDepth<min_depth>" + "-PartitionDepth<depth>"
        or "-Remainder" (only when partitioned) + "-" + the input's prefix + ".fastq" / ".fasta", round-major and by input inside
        a round, a file nothing was written to left out (the reference opens a file at its first read); without, one entry named
        `output` that holds the concatenation.  input_prefixes default to "transformed-<j + 1>", the reference's name for reads
        that came from no input file (src/ReadSet.cpp:376-382).  .segments and .read_segment hold the tables.
        With max_kmer_output_depth > 0 (:178-206): coverage normalization over `pairs` (kmr_normalize_*), one round whose files
        are named `output` + "-MinDepth<min_depth>" + "-MaxDepth<depth>" + "-" + prefix + suffix; by_pair defaults to the pairs'
        hasPairs, as the reference passes it; normalization_method "RANDOM" only; together with partition_by_depth it raises, as
        the reference's option check does (src/ReadSelector.h:137).
        bimodal_sigmas: as scoreAndTrimReads takes it, for the scoring a fused call does; where scoreAndTrimReads has run, its
        trims and tags are what is selected from."""
        if max_kmer_output_depth > 0:
            if partition_by_depth > 0:
                raise KmerSpectrumError("selectReads: max_kmer_output_depth and partition_by_depth exclude each other")
            if normalization_method not in ("RANDOM", "OPTIMAL"):
                raise KmerSpectrumError("selectReads: normalization_method %r" % (normalization_method,))
            cfg = self._normalize(max_kmer_output_depth, min_depth, min_read_length, self.has_pairs if by_pair is None else by_pair, both_pass, seed, first_read_idx,
                                  scoring, output_quality_base, format, input_starts, method=0 if normalization_method == "RANDOM" else 1, bimodal_sigmas=bimodal_sigmas)
            text = self._copy()
            seg = self._segments()
            if not separate_outputs:
                return [(output, text)]
            return self._files(text, seg, ["%s-MinDepth%d-MaxDepth%d" % (output, int(min_depth), int(max_kmer_output_depth))], input_prefixes, self.SUFFIX[cfg.select.format])
        fused = self.trims is None
        cfg = _lib.KmrPartitionConfig()
        self.sp.lib.kmr_partition_config_init(C.byref(cfg))
        cfg.select = self._config(min_depth, min_read_length, both_pass, output_quality_base, format, scoring if fused else self.scoring)
        cfg.partition_by_depth, cfg.remainder_trim = int(partition_by_depth), float(remainder_trim)
        starts, starts_p, n_inputs = self._starts_args(input_starts)
        keep, tp, tn = self._text_args()
        out = C.c_void_p()
        head = (self.sp.h, self.reads.r, tp, tn, self._p(self.mate, C.c_int64)) + tuple(self._af_args())
        tail = (starts_p, n_inputs, C.byref(cfg), C.byref(out))
        if fused:
            with self.sp._bimodal_for(bimodal_sigmas, self.reads.n):
                self.sp._call("partition_read_batch", *head, *tail)
        else:
            trims, trim_ptrs = self._trim_args()
            self._tag_args()
            self.sp._call("partition_reads", *head, *trim_ptrs, *tail)
        self._adopt(out)
        self._sel, self._fmt = None, (output_quality_base, cfg.select.format)
        text = self._copy()
        seg = self._segments()
        if not separate_outputs:
            return [(output, text)]
        names = []
        for r in range(seg["picks"].shape[0]):
            name = "%s-MinDepth%d" % (output, int(min_depth))
            if partition_by_depth > 0:      # lexical_cast<string>(float tmpMinDepth): 16, not 16.0
                name += "-Remainder" if seg["round_is_remainder"][r] else ("-PartitionDepth%.9g" % seg["round_depth"][r] if seg["round_depth"][r] > 0 else "")
            names.append(name)
        return self._files(text, seg, names, input_prefixes, self.SUFFIX[cfg.select.format])

    def _normalize(self, target_depth, min_score, min_read_length, by_pair, both_pass, seed, first_read_idx, scoring, output_quality_base, format,
                   input_starts=None, method=0, use_logscale=False, bimodal_sigmas=-1.0):
        """kmr_normalize_reads over the trims scoreAndTrimReads left, or kmr_normalize_read_batch without them"""
        fused = self.trims is None
        cfg = _lib.KmrNormalizeConfig()
        self.sp.lib.kmr_normalize_config_init(C.byref(cfg))
        cfg.select = self._config(min_score, min_read_length, both_pass, output_quality_base, format, scoring if fused else self.scoring)
        cfg.target_depth, cfg.seed, cfg.first_global_read_idx = int(target_depth), int(seed), int(first_read_idx)
        cfg.by_pair, cfg.method, cfg.use_logscale = (1 if by_pair else 0), int(method), (1 if use_logscale else 0)
        starts, starts_p, n_inputs = self._starts_args(input_starts)
        r1, r2 = self.pairs if self.pairs is not None else (None, None)
        keep, tp, tn = self._text_args()
        out = C.c_void_p()
        head = (self.sp.h, self.reads.r, tp, tn, self._p(r1, C.c_int64), self._p(r2, C.c_int64), 0 if r1 is None else r1.size) + tuple(self._af_args())
        tail = (starts_p, n_inputs, C.byref(cfg), C.byref(out))
        if fused:
            with self.sp._bimodal_for(bimodal_sigmas, self.reads.n):
                self.sp._call("normalize_read_batch", *head, *tail)
        else:
            trims, trim_ptrs = self._trim_args()
            self._tag_args()
            self.sp._call("normalize_reads", *head, *trim_ptrs, *tail)
        self._adopt(out)
        self._sel, self._fmt = None, (output_quality_base, cfg.select.format)
        v = [C.c_uint64() for _ in range(3)]
        _ok(self.sp.lib.kmr_normalize_info(self._picks, *[C.byref(x) for x in v]), "kmr_normalize_info")
        self.normalize_info = dict(zip(("n_picks", "n_candidates", "n_draws"), (x.value for x in v)))
        return cfg

    def pickCoverageNormalizedSubset(self, target_depth, min_score=0.0, min_read_length=None, by_pair=False, both_pass=False, seed=0, first_read_idx=0,
                                     output_quality_base=33, format="fastq", bimodal_sigmas=-1.0):
        """ReadSelector::pickCoverageNormalizedSubset (:673-749), RANDOM, over `pairs`, on the device (kmr_normalize_reads, or
        kmr_normalize_read_batch if scoreAndTrimReads has not run): a pair or read of score s above target_depth is kept if
        draw % s <= target_depth, draw = Philox4x32-10 of (seed, first_read_idx + read index).  Returns the number of picks as the
        reference counts them (pairs; n_picked counts records); .normalize_info holds them with the chooseRead calls and the draws."""
        self._normalize(target_depth, min_score, min_read_length, by_pair, both_pass, seed, first_read_idx, "MEDIAN", output_quality_base, format, bimodal_sigmas=bimodal_sigmas)
        return self.normalize_info["n_picks"]

    def _segments(self):
        """the segment table (kmr_picks_segments_copy) into .segments -- round_depth and round_is_remainder per round, first_pick,
        picks, first_byte and bytes as (n_rounds, n_inputs) arrays -- and .read_segment: round * n_inputs + input per read, -1 = not
        picked"""
        nr, ni = C.c_uint32(), C.c_uint32()
        _ok(self.sp.lib.kmr_picks_segments_info(self._picks, C.byref(nr), C.byref(ni)), "kmr_picks_segments_info")
        nr, ni = nr.value, ni.value
        depth, rem = np.zeros(33, dtype=np.float32), np.zeros(33, dtype=np.uint8)
        cols = [np.zeros(max(1, nr * ni), dtype=np.uint64) for _ in range(4)]
        rseg = np.full(max(1, self.reads.n), -1, dtype=np.int32)
        _ok(self.sp.lib.kmr_picks_segments_copy(self._picks, self._p(depth, C.c_float), self._p(rem, C.c_uint8), *[self._p(c, C.c_uint64) for c in cols],
                                                self._p(rseg, C.c_int32)), "kmr_picks_segments_copy")
        self.segments = dict(round_depth=depth[:nr], round_is_remainder=rem[:nr].astype(bool),
                             **{k: c[:nr * ni].reshape(nr, ni) for k, c in zip(("first_pick", "picks", "first_byte", "bytes"), cols)})
        self.read_segment = rseg[:self.reads.n]
        return self.segments

    def _copy(self):
        buf = np.zeros(max(1, self.bytes), dtype=np.uint8)
        flags = np.zeros(max(1, self.reads.n), dtype=np.uint8)
        _ok(self.sp.lib.kmr_picks_copy(self._picks, buf.ctypes.data_as(C.c_void_p), self.bytes, flags.ctypes.data_as(C.POINTER(C.c_uint8))), "kmr_picks_copy")
        self.picked_flags = flags[:self.reads.n].astype(bool)
        self._text = buf[:self.bytes].tobytes()
        return self._text

    def writePicks(self, output_quality_base=33, format="fastq"):
        """the text of the picks (Read::toFastq / toFasta per picked read, ascending read index) as bytes"""
        if self._picks is None:
            raise KmerSpectrumError("writePicks: nothing has been picked")
        fmt = (output_quality_base, self.FORMAT[format] if isinstance(format, str) else int(format))
        if fmt != self._fmt:
            if self._sel is None:
                raise KmerSpectrumError("writePicks: filterReads fixed the format; call it again with the other one")
            self._run(output_quality_base, format)
        return self._text if self._text is not None else self._copy()

    @property
    def picks(self):
        """indices of the picked reads, ascending"""
        if self._picks is not None and self._text is None:
            self._copy()
        return np.nonzero(self.picked_flags)[0]

    def device_text(self):
        """(device pointer, bytes) of the output text (kmr_picks_device_ptr); valid until the next pick or close()"""
        p = C.c_void_p()
        self.sp._call("picks_device_ptr", self._picks, C.byref(p))
        return p.value, self.bytes



class ConsensusReadSet(ReadSet):
    """The consensus reads of one duplicate-fragment pass: a ReadSet whose names point into a name text of its own.  The batch
    belongs to the DedupPass it came from and lives until that is closed."""

    @classmethod
    def _borrow(cls, owner, spectrum, name_text, handle):
        self = cls._adopt(spectrum, name_text, handle, True)
        self._owner = owner
        return self

    def close(self):
        self.r = None          # the DedupPass frees it


class DedupPass(_DeviceObject):
    """What one kmr_dedup_fragments* call left (kmr_dedup), kept on the device until close(): .discarded (uint8 per read: the
    flags handed in OR the new discards), .affected, .skipped = (discarded, too short, unpaired, invalid), .groups = (n_groups, 2)
    int64 array of (pair-list position of the first member, member count), .consensus = the new reads as a ConsensusReadSet,
    .consensus_mate = the mate of each of them (2g <-> 2g + 1 in the paired pass, -1 in the single pass); .single = the
    --dedup-single pass that followed, or None."""
    _HANDLE, _FREE = "_d", "kmr_dedup_free"

    def __init__(self, sp, handle, paired, n_reads):
        self.sp, self._d, self.paired, self.single, self.n_reads = sp, handle, bool(paired), None, n_reads
        ng, nn, af = C.c_uint64(), C.c_uint64(), C.c_uint64()
        sk = (C.c_uint64 * 4)()
        _ok(sp.lib.kmr_dedup_info(handle, C.byref(ng), C.byref(nn), C.byref(af), sk), "kmr_dedup_info")
        self.n_groups, self.n_new_reads, self.affected, self.skipped = ng.value, nn.value, af.value, tuple(int(v) for v in sk)
        r, nt, nl = C.c_void_p(), C.c_void_p(), C.c_uint64()
        sp.lib.kmr_dedup_reads(handle, C.byref(r), C.byref(nt), C.byref(nl))
        names = np.zeros(max(1, nl.value), dtype=np.uint8)
        _ok(sp.lib.kmr_dedup_names_copy(handle, names.ctypes.data_as(C.c_void_p), nl.value), "kmr_dedup_names_copy")
        self.device_name_text = (nt.value or 0, nl.value)
        self.consensus = ConsensusReadSet._borrow(self, sp, names[:nl.value].tobytes(), r)
        m = np.arange(self.n_new_reads, dtype=np.int64)
        self.consensus_mate = (m ^ 1) if self.paired else np.full(self.n_new_reads, -1, dtype=np.int64)
        self._host = None

    def _copy(self):
        if self._host is None:
            disc = np.zeros(max(1, self.n_reads), dtype=np.uint8)
            gf = np.zeros(max(1, self.n_groups), dtype=np.uint64)
            gs = np.zeros(max(1, self.n_groups), dtype=np.uint32)
            _ok(self.sp.lib.kmr_dedup_copy(self._live(), disc.ctypes.data_as(C.POINTER(C.c_uint8)), gf.ctypes.data_as(C.POINTER(C.c_uint64)), gs.ctypes.data_as(C.POINTER(C.c_uint32))), "kmr_dedup_copy")
            self._host = (disc[:self.n_reads], np.stack([gf[:self.n_groups].astype(np.int64), gs[:self.n_groups].astype(np.int64)], axis=1))
        return self._host

    @property
    def discarded(self):
        return self._copy()[0]

    @property
    def groups(self):
        return self._copy()[1]

    def device_ptrs(self):
        """device pointers of (discarded[n_reads] uint8, group_first[n_groups] uint64, group_size[n_groups] uint32); valid until close()"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _ok(self.sp.lib.kmr_dedup_device_ptrs(self._live(), C.byref(a), C.byref(b), C.byref(c)), "kmr_dedup_device_ptrs")
        return a.value or 0, b.value or 0, c.value or 0

    def close(self):
        if self.single is not None:
            self.single.close()
        if getattr(self, "_d", None):
            self.consensus.r = None
        super().close()


class DuplicateFragmentFilter:
    """DuplicateFragmentFilter::filterDuplicateFragments (src/DuplicateFragmentFilter.h:561-620) with edit distance 0 and consensus
    on, over a device-resident ReadSet and the ReadPairs identifyPairs found for it (kmr_dedup_fragments): fragments whose first
    dedup_length bases of both reads (from start_offset) agree collapse to consensus reads; dedup_mode 2 also folds a fragment read
    from the other strand (B, A) onto (A, B)."""

    def __init__(self, spectrum, dedup_mode=1, dedup_length=24, start_offset=0):
        self.sp = spectrum
        cfg = _lib.KmrDedupConfig()
        spectrum.lib.kmr_dedup_config_init(C.byref(cfg))
        cfg.dedup_mode, cfg.dedup_length, cfg.start_offset = int(dedup_mode), int(dedup_length), int(start_offset)
        self.cfg = cfg

    def _pass(self, read_set, pairs, discarded, paired, device_text):
        cfg = _lib.KmrDedupConfig.from_buffer_copy(self.cfg)
        cfg.paired = 1 if paired else 0
        d = None
        if discarded is not None:
            d = np.ascontiguousarray(np.asarray(discarded) != 0, dtype=np.uint8)
            assert d.size == read_set.n
        dp = None if d is None or d.size == 0 else d.ctypes.data_as(C.POINTER(C.c_uint8))
        out = C.c_void_p()
        if device_text is not None:
            self.sp._call("dedup_fragments_dev", self.sp.h, read_set.r, C.c_void_p(device_text), len(read_set.text), pairs._live(), dp, C.byref(cfg), C.byref(out))
        else:
            buf = np.frombuffer(read_set.text, dtype=np.uint8)
            self.sp._call("dedup_fragments", self.sp.h, read_set.r, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, pairs._live(), dp, C.byref(cfg), C.byref(out))
        return DedupPass(self.sp, out, paired, read_set.n)

    def filterDuplicateFragments(self, read_set, pairs, discarded=None, dedup_single=False, device_text=None):
        """The paired pass and, with dedup_single, the pass over single reads behind it (:587-616), which is given the first pass's
        discards.  `discarded` = per read, non-zero = discarded (FilterKnownOddities' action == 2); `device_text` = device pointer
        of the FASTQ text if the caller holds it there.  Returns the paired pass's DedupPass, the single pass as its .single."""
        res = self._pass(read_set, pairs, discarded, True, device_text)
        if dedup_single:
            res.single = self._pass(read_set, pairs, res.discarded, False, device_text)
        return res


def synth_reads_device(torch, seed, first_read, n_reads, read_len, genome_len, noisy, device):
    """kmr_synth_reads_dev into torch tensors on `device`: (bases u8, quals u8, offsets i64).  The buffers carry 64 spare bytes behind
    the last read, as the device entry points of the build ask for."""
    lib = _lib.load()
    with torch.cuda.device(device):
        bases = torch.zeros(n_reads * read_len + 64, dtype=torch.uint8, device=device)
        quals = torch.zeros(n_reads * read_len + 64, dtype=torch.uint8, device=device)
        offsets = torch.empty(n_reads + 1, dtype=torch.int64, device=device)
        torch.cuda.synchronize()
        _ok(lib.kmr_synth_reads_dev(seed, first_read, n_reads, read_len, genome_len, 1 if noisy else 0, bases.data_ptr(), quals.data_ptr(), offsets.data_ptr()), "kmr_synth_reads_dev")
    return bases, quals, offsets
