"""The device text dump at a size where byte offsets pass 2^32, run behind every other test file (see test_zz_gpu_at_scale.py).

One build with extension values of C2's reads (10 M x 150 bp, SURVEY.md 8(d)'s generator, noisy qualities, k = 31,
MeraculousCounter's settings) holds some 5 x 10^7 weak entries: its mergraph text is several GB.  The oracle is too slow to rerun
at this size, so the check is internal, but not circular:
  - the whole text made by one call equals, compared on the device, the concatenation of pieces of less than 1 GiB each -- the
    regime tests/test_mer_dump.py pins to the oracle byte for byte;
  - the first and the last 1 000 entries of the text are parsed again on the host and compared with the keys, counts and
    tallies of image()."""
import numpy as np
import pytest

import kmernator_amd as ka
from helpers import KMR_MAP_WEAK, KMR_VALUE_EXT

pytestmark = pytest.mark.gpu

READS, READ_LEN, K, MIN_DEPTH, SEED = 10_000_000, 150, 31, 2, 1234
KB, VSIZE = (K + 3) // 4, 60
RC_ORDER = [9, 8, 7, 6, 10, 11, 3, 2, 1, 0, 4, 5]          # ExtensionTracking::getReverseComplement (src/KmerTrackingData.h:219-226)


def _entries_from(img, offs, buckets, limit):
    """(keys [m, KB], values u32 [m, 15]) of the entries of `buckets` (in that order of buckets, map order inside one) until `limit`"""
    keys, vals = [], []
    for b in buckets:
        o = int(offs[b])
        n = int(img[o:o + 4].view(np.uint32)[0])
        if n:
            keys.append(img[o + 4:o + 4 + n * KB].reshape(n, KB))
            vals.append(img[o + 4 + n * KB:o + 4 + n * (KB + VSIZE)].copy().view(np.uint32).reshape(n, 15))
            limit -= n
            if limit <= 0:
                break
    return keys, vals


def _lines_of(key, val):
    codes = np.stack([(key >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:K]
    fwd = bytes(b"ACGT"[c] for c in codes)
    rev = bytes(b"ACGT"[3 - c] for c in codes[::-1])
    t = [int(x) for x in val[3:15]]
    tail = lambda ts: b"\t" + b"".join(b"%d " % x for x in ts) + b"0"
    return [fwd + tail(t), rev + tail([t[i] for i in RC_ORDER])]


def test_mergraph_text_beyond_4_gib():
    import torch
    dev = torch.device("cuda", 0)
    b, q, o = ka.synth_reads_device(torch, SEED, 0, READS, READ_LEN, 5 * READS, True, dev)
    p = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=READS * (READ_LEN - K + 1), device=0, value_kind=KMR_VALUE_EXT, min_weight=0.0, min_quality_score=2))
    p.buildKmerSpectrumDevice(b.data_ptr(), q.data_ptr(), o.data_ptr(), READS, READS * READ_LEN, 0)
    p.finalize(MIN_DEPTH)
    del b, q, o
    torch.cuda.empty_cache()
    n = p.stats()["weak_entries"]
    kept, nbytes = p.dumpTextSize("mergraph", MIN_DEPTH)
    print("weak entries %d, kept %d, mergraph text %d bytes" % (n, kept, nbytes))
    assert kept == n                                  # the map was finalized at this min depth: every entry is kept
    assert nbytes > 1 << 32, "the build is too small for this test: %d bytes of text" % nbytes
    free, total = torch.cuda.mem_get_info(0)
    need = nbytes + (2 << 30) + 12 * n + (1 << 30)     # the whole text, one piece, the size pass's scratch, slack
    if free < need:
        pytest.skip("the device has %.1f GB free of %.1f GB; the whole text and one piece need %.1f GB" % (free / 1e9, total / 1e9, need / 1e9))
    whole = p.dumpGraphsText(MIN_DEPTH)
    assert (whole.kept, whole.bytes) == (kept, nbytes)
    wt = whole.device_tensor()
    assert wt.numel() == nbytes
    # pieces of under 1 GiB
    step = int(0.9 * (1 << 30) / (nbytes / n))
    at, total_kept, pieces = 0, 0, 0
    for lo in range(0, n, step):
        with p.dumpGraphsText(MIN_DEPTH, lo, min(n, lo + step)) as piece:
            assert 0 < piece.bytes < 1 << 30
            assert (piece.kept, piece.bytes) == p.dumpTextSize("mergraph", MIN_DEPTH, lo, min(n, lo + step))
            pt = piece.device_tensor()
            assert torch.equal(wt[at:at + piece.bytes], pt), "piece of entries [%d, %d) differs from the whole text at byte %d" % (lo, lo + step, at)
            del pt
            at += piece.bytes
            total_kept += piece.kept
            pieces += 1
    assert (at, total_kept) == (nbytes, kept) and pieces > 4
    # head and tail against image()
    span = 1000 * 2 * 300
    head = wt[:span].cpu().numpy().tobytes().split(b"\n")[:2000]
    tail = wt[nbytes - span:].cpu().numpy().tobytes()
    assert tail.endswith(b"\n")
    tail = tail[:-1].split(b"\n")[-2000:]
    del wt
    whole.close()
    img = p.image(KMR_MAP_WEAK)
    nb = int(img[:8].view(np.uint64)[0])
    offs = img[16:16 + 8 * nb].view(np.uint64)
    keys, vals = _entries_from(img, offs, range(nb), 1000)
    keys, vals = np.concatenate(keys)[:1000], np.concatenate(vals)[:1000]
    want = [line for key, val in zip(keys, vals) for line in _lines_of(key, val)]
    assert head == want
    keys, vals = _entries_from(img, offs, range(nb - 1, -1, -1), 1000)
    keys, vals = np.concatenate(keys[::-1])[-1000:], np.concatenate(vals[::-1])[-1000:]
    want = [line for key, val in zip(keys, vals) for line in _lines_of(key, val)]
    assert tail == want
    assert all((int(v[0]) & 0xffff) >= MIN_DEPTH for v in vals)
    p.close()
