"""ContigExtender on the device (kmr_extend_*; kmernator_amd/csrc/kmr_extend.hpp) held to the restatement of tests/refextend.py over the
directed contigs and pools of tests/extendcases.py.  Every figure is an integer, a string or an f64 compared by its bits: sequences,
totals, names, log text, stop reasons and stop values equal the restatement's."""
import ctypes as C
import functools

import numpy as np
import pytest

import extendcases as ec
import kmernator_amd as ka
import refextend as rx
from helpers import default_config
from kmernator_amd import _lib
from refmatch import Matcher

pytestmark = pytest.mark.gpu

CASES = ec.all_cases()
IDS = ["%s-k%d" % (c["name"], c["k"]) for c in CASES]


# ------------------------------------------------------------------------------------------------------------------- reference side
@functools.lru_cache(maxsize=None)
def want_of(i):
    c = CASES[i]
    return want(c)


def want(c, contigs=None, pools=None):
    contigs = c["contigs"] if contigs is None else contigs
    pools = [ec.pool_of(c, j) for j in range(len(contigs))] if pools is None else pools
    return rx.Extender(default_config(c["k"], **c["cfg"]), **c["options"]).extend(contigs, pools, c["active"])


# ---------------------------------------------------------------------------------------------------------------------- device side
def spectrum_of(c, k=None):
    """a handle that is never fed: it supplies k and the build's config"""
    return ka.KmerSpectrum(ka.default_config(c["k"] if k is None else k, device=0, estimated_raw_kmers=4096, **c["cfg"]))


def batch(sp, seqs, quals=None):
    """sequences as a device batch, byte for byte (no parser in between); quals None: Read::REF_QUAL"""
    b = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
    q = np.frombuffer((b"".join(quals) if quals is not None else bytes([rx.REF_QUAL]) * (b.size - 1)) + b"\0", dtype=np.uint8)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return ka.ReadSet.from_arrays(sp, b, q, off)


def csr(pools):
    off = np.zeros(len(pools) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pools], out=off[1:])
    return off, np.array([j for p in pools for j in p], dtype=np.uint64)


def same(res, wanted, names):
    """an ExtendResults against the restatement's list"""
    assert res.n == len(wanted)
    assert res.sequences() == [w[0] for w in wanted]
    assert list(res.left) == [w[1] for w in wanted] and list(res.right) == [w[2] for w in wanted]
    assert list(res.new_len) == [len(w[0]) for w in wanted]
    assert res.names == [rx.new_name(nm, w[1], w[2]) for nm, w in zip(names, wanted)]
    assert res.n_extended == sum(1 for w in wanted if w[1] + w[2]) and res.bases_added == sum(w[1] + w[2] for w in wanted)
    for i, w in enumerate(wanted):
        for side in (0, 1):
            reason, vals = w[3][side]
            st = res.stops[i, side]
            got = [st["edge"]] + list(st["ext"]) + [st["total"]]
            assert int(st["reason"]) == reason, (i, side, int(st["reason"]), reason, got, vals)
            assert [rx.bits(v) for v in got] == [rx.bits(v) for v in vals], (i, side, got, vals)
    b, q, o, _ = res.read_set.arrays()
    assert b.tobytes() == b"".join(w[0] for w in wanted) and (q == rx.REF_QUAL).all()


def device(sp, c, cs, rs, dev=False):
    off, idx = csr(c["pools"])
    ex = ka.ContigExtender(sp, **c["options"])
    act = None if c["active"] is None else np.array(c["active"], dtype=np.uint8)
    if not dev:
        return ex.extendContigs(cs, rs, (off, idx), names=c["names"], active=act)
    import torch
    d = torch.device("cuda:0")
    t_off, t_idx = torch.from_numpy(off.view(np.int64)).to(d), torch.from_numpy(np.append(idx, np.uint64(0)).view(np.int64)).to(d)
    t_act = None if act is None else torch.from_numpy(act).to(d)
    torch.cuda.synchronize()
    return ex.extendContigsDevice(cs, rs, t_off.data_ptr(), t_idx.data_ptr(), names=c["names"], dev_active=0 if t_act is None else t_act.data_ptr())


# ----------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_families_equal_the_restatement(i):
    """host arrays and device arrays, through the Python classes over the C entry points"""
    c = CASES[i]
    sp = spectrum_of(c)
    try:
        for knob, v in c["tune"].items():
            sp.tune(**{knob: v})
        with batch(sp, c["contigs"]) as cs, batch(sp, [s for s, _ in c["reads"]], [q for _, q in c["reads"]]) as rs:
            with device(sp, c, cs, rs) as res:
                same(res, want_of(i), c["names"])
            if c["tune"]:
                assert sp.build_info("extend_runs") > 1
            with device(sp, c, cs, rs, dev=True) as res:
                same(res, want_of(i), c["names"])
    finally:
        sp.close()


@pytest.mark.parametrize("k", ec.KS)
def test_c_abi_directly(k):
    """the entry points without the classes: info, copy, the borrowed batch"""
    c = ec.several(k)[0]
    w = want(c)
    sp = spectrum_of(c)
    lib = sp.lib
    try:
        with batch(sp, c["contigs"]) as cs, batch(sp, [s for s, _ in c["reads"]], [q for _, q in c["reads"]]) as rs:
            off, idx = csr(c["pools"])
            cfg = _lib.KmrExtendConfig()
            assert lib.kmr_extend_config_init(C.byref(cfg)) == 0
            cfg.max_extend = c["options"]["max_extend"]
            e = C.c_void_p()
            u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
            assert lib.kmr_extend_contigs(sp.h, cs.r, rs.r, off.ctypes.data_as(u64), idx.ctypes.data_as(u64), None, C.byref(cfg), C.byref(e)) == 0, lib.kmr_last_error(sp.h)
            try:
                n, nx, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
                assert lib.kmr_extend_info(e, C.byref(n), C.byref(nx), C.byref(nb)) == 0
                assert (n.value, nx.value, nb.value) == (len(w), sum(1 for x in w if x[1] + x[2]), sum(x[1] + x[2] for x in w))
                nl, lt, rt = (np.zeros(len(w), dtype=np.uint32) for _ in range(3))
                st = (_lib.KmrExtendStop * (2 * len(w)))()
                assert lib.kmr_extend_copy(e, nl.ctypes.data_as(u32), lt.ctypes.data_as(u32), rt.ctypes.data_as(u32), st) == 0
                assert list(nl) == [len(x[0]) for x in w] and list(lt) == [x[1] for x in w] and list(rt) == [x[2] for x in w]
                for i, x in enumerate(w):
                    for side in (0, 1):
                        s = st[2 * i + side]
                        assert s.reason == x[3][side][0] and [rx.bits(v) for v in [s.edge] + list(s.ext) + [s.total]] == [rx.bits(v) for v in x[3][side][1]]
                r = C.c_void_p()
                assert lib.kmr_extend_reads(e, C.byref(r)) == 0 and r.value
                nr, tb = C.c_uint64(), C.c_uint64()
                assert lib.kmr_reads_info(r, C.byref(nr), C.byref(tb), None, None) == 0 and (nr.value, tb.value) == (len(w), sum(len(x[0]) for x in w))
                assert lib.kmr_extend_copy(e, None, None, None, None) == 0
            finally:
                lib.kmr_extend_free(e)
    finally:
        sp.close()


@pytest.mark.parametrize("k", [21, 65])
def test_second_round_through_kmer_match(k):
    """the result batch is what the next round takes: KmerMatch over the new contigs gives the pools (a MatchResults with
    first_global_read_idx), extendContigs grows them again, and both rounds equal the restatement"""
    c = ec.clean(k)[1]                     # two bases on either side per round
    first = 1000
    reads = c["reads"]
    w1 = want(c)
    sp = spectrum_of(c)
    fed = ka.KmerSpectrum(ka.default_config(k, device=0, estimated_raw_kmers=1 << 16))
    try:
        with batch(sp, c["contigs"]) as cs, batch(sp, [s for s, _ in reads], [q for _, q in reads]) as rs:
            b, q, o, _ = rs.arrays()
            fed.buildKmerSpectrum(np.append(b, np.uint8(0)), np.append(q, np.uint8(0)), o)
            fed.finalize(1)
            with device(sp, c, cs, rs) as r1:
                same(r1, w1, c["names"])
                contigs2 = [x[0] for x in w1]
                with ka.KmerMatch(fed, r1.read_set, k + 3, 0, False, 0) as km:
                    km.addReads(rs, first)
                    pools = km.finish()
                m = Matcher(default_config(k), min_depth=1, max_positions_from_edge=k + 3, max_read_matches=0, include_mate=False)
                mw = m.match(contigs2, [dict(first=first, reads=reads, mate=None, discarded=[0] * len(reads))])
                assert np.array_equal(pools.offsets, mw["offsets"]) and np.array_equal(pools.reads, mw["reads"]) and len(pools.reads) > 0
                with ka.ContigExtender(sp, **c["options"]).extendContigs(r1.read_set, rs, pools, names=r1.names, first_global_read_idx=first) as r2:
                    w2 = want(c, contigs2, [[reads[int(j) - first] for j in pools[i]] for i in range(len(contigs2))])
                    same(r2, w2, r1.names)
                    assert r2.names == [b"c0-l4r4"] and r2.bases_added == 4
    finally:
        fed.close()
        sp.close()


@pytest.mark.parametrize("k", ec.KS)
def test_driver_equals_the_restatement(k):
    """extendContigsWithContigExtender over the sizes k and k + 2: lists and log text"""
    c = ec.driver_case(k)
    pools = [ec.pool_of(c, i) for i in range(len(c["contigs"]))]
    w = rx.extend_with_contig_extender(lambda kk: rx.Extender(default_config(kk), **c["options"]), c["contigs"], c["names"], pools, k, k + 2, 2)
    made = {}

    def make(kk):
        made[kk] = spectrum_of(c, kk)
        return made[kk]
    sp = spectrum_of(c)
    try:
        with batch(sp, c["contigs"]) as cs, batch(sp, [s for s, _ in c["reads"]], [q for _, q in c["reads"]]) as rs:
            got = ka.extendContigsWithContigExtender(make, cs, c["names"], rs, csr(c["pools"]), k, k + 2, 2, **c["options"])
            assert tuple(got) == w and got.skipped_k == [] and sorted(made) == [k, k + 2]
            changed, final, log = got
            assert ka.finishLongContigs(0, changed, final) == ([], final + changed)
            if k == 97:      # sizes the library does not reach are passed over and listed
                got = ka.extendContigsWithContigExtender(make, cs, c["names"], rs, csr(c["pools"]), 127, 131, 2, **c["options"])
                assert got.skipped_k == [129, 131] and len(got[0]) == 0
    finally:
        for s in made.values():
            s.close()
        sp.close()


def test_refusals():
    c = ec.clean(21)[0]
    sp = spectrum_of(c)
    lib = sp.lib
    u64 = C.POINTER(C.c_uint64)
    try:
        with batch(sp, c["contigs"]) as cs, batch(sp, [s for s, _ in c["reads"]], [q for _, q in c["reads"]]) as rs:
            cfg = _lib.KmrExtendConfig()
            lib.kmr_extend_config_init(C.byref(cfg))

            def call(off, idx, cfg=cfg, h=sp.h, contigs=cs.r):
                off, idx = np.array(off, dtype=np.uint64), np.array(idx, dtype=np.uint64)
                e = C.c_void_p()
                rc = lib.kmr_extend_contigs(h, contigs, rs.r, off.ctypes.data_as(u64), idx.ctypes.data_as(u64), None, C.byref(cfg), C.byref(e))
                if e.value:
                    lib.kmr_extend_free(e)
                return rc
            assert call([0, 2], [0, 1]) == 0
            assert call([0, 2], [0, rs.n]) == -1          # a pool index out of range
            assert call([1, 2], [0, 1]) == -1             # the offsets do not start at 0
            with batch(sp, c["contigs"] * 2) as cs2:
                assert call([0, 2, 1], [0, 1], contigs=cs2.r) == -1      # the offsets descend
            big = _lib.KmrExtendConfig()
            lib.kmr_extend_config_init(C.byref(big))
            big.max_extend = _lib.KMR_EXTEND_MAX_EXTEND + 1
            assert call([0, 2], [0, 1], cfg=big) == -7    # KMR_ERR_UNSUPPORTED
            assert b"max_extend" in lib.kmr_last_error(sp.h)
            bad = _lib.KmrExtendConfig()
            lib.kmr_extend_config_init(C.byref(bad))
            bad.struct_size -= 4
            assert call([0, 2], [0, 1], cfg=bad) == -1
            assert call([0, 2], [0, 1], h=None) == -1
            # device arrays: the same refusals come from the device's own check
            import torch
            d = torch.device("cuda:0")
            for off, idx in (([0, 2], [0, rs.n]), ([1, 2], [0, 1])):
                t_off, t_idx = torch.tensor(off, dtype=torch.int64, device=d), torch.tensor(idx, dtype=torch.int64, device=d)
                torch.cuda.synchronize()
                e = C.c_void_p()
                assert lib.kmr_extend_contigs_dev(sp.h, cs.r, rs.r, t_off.data_ptr(), t_idx.data_ptr(), None, C.byref(cfg), C.byref(e)) == -1 and not e.value
            if torch.cuda.device_count() > 1:      # batches of another device
                sp1 = ka.KmerSpectrum(ka.default_config(21, device=1, estimated_raw_kmers=4096))
                try:
                    with batch(sp1, c["contigs"]) as other:
                        assert call([0, 2], [0, 1], contigs=other.r) == -1
                finally:
                    sp1.close()
    finally:
        sp.close()
