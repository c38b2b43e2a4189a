#!/usr/bin/env python3
"""Writes tests/golden/ref_lookup3_hashes.npz: what the reference's own lookup3 (KmerHasher::getHash, src/Kmer.h:207-230)
gives for the random keys tests/test_oracle_kat.py::test_hash_against_reference_lookup3 hashes -- 50 keys of every length
1 ... 40 bytes from numpy's default_rng(11), each hashed from an 8-byte aligned buffer and from a misaligned one (the
reference's word-wise and byte-wise paths must agree).  The keys are stored with their hashes, so the test needs neither the
reference nor the generator's stream.

The hashes come from oracle/_ref/libref_lookup3.so, which oracle/Makefile compiles from the reference checkout.  Run after
build() where that checkout is present: python tests/golden/make_ref_lookup3_hashes.py [path/to/libref_lookup3.so]"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SO = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "oracle", "_ref", "libref_lookup3.so")

ref = C.CDLL(SO)
ref.ref_get_hash.restype = C.c_uint64
ref.ref_get_hash.argtypes = [C.c_char_p, C.c_uint64]
rng = np.random.default_rng(11)
keys, lengths, hashes = [], [], []
for n in range(1, 41):
    for _ in range(50):
        key = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        h = ref.ref_get_hash(C.create_string_buffer(key, n), n)
        buf2 = C.create_string_buffer(b"x" + key, n + 1)
        assert ref.ref_get_hash(C.cast(C.addressof(buf2) + 1, C.c_char_p), n) == h
        keys.append(key)
        lengths.append(n)
        hashes.append(h)
out = os.path.join(HERE, "ref_lookup3_hashes.npz")
np.savez_compressed(out, keys=np.frombuffer(b"".join(keys), dtype=np.uint8), lengths=np.array(lengths, dtype=np.uint32),
                    hashes=np.array(hashes, dtype=np.uint64))
print(out, len(hashes), "keys", os.path.getsize(out), "bytes")
