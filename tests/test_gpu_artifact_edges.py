"""The artifact filter on the device (artifact_screen, artifact_action, artifact_gather; kmr_artifact_filter_apply) held to
tests/refartifact.py -- the reference's applyFilterToRead / recordAffectedRead restated from its source in its own byte-pointer
form, with nothing of the kernel's or the oracle's in it -- on the directed families of tests/artifactcases.py (proven on the CPU,
in tests/test_artifact_cases.py, to reach every threshold, tie and wrap they are written for).

Everything compared is an integer or a byte: all six result arrays and the read set afterwards (bases, qualities, offsets,
names) must be equal.  The reads go in through ReadSet.from_arrays, which lets every byte through; the names case goes through
FASTQ text.  Every case is then filtered a second time: the device's output of its own output against the reference applied to
the reference's first output."""
import functools

import numpy as np
import pytest

import artifactcases as ac
import kmernator_amd as ka
import refartifact as ra
from helpers import OracleArtifactFilter, artifact_config

pytestmark = pytest.mark.gpu

KEYS = ("value", "min_pass", "max_pass", "action", "remnant_off", "remnant_len")


class Device:
    """one handle and one filter per configuration, for the module's lifetime"""

    def __init__(self):
        self.sp = ka.KmerSpectrum(ka.default_config(31, estimated_raw_kmers=1000, device=0))
        self.filters = {}

    def filter(self, kw, fasta):
        key = (fasta, tuple(sorted(kw.items())))
        if key not in self.filters:
            self.filters[key] = ka.FilterKnownOddities(self.sp, fasta, **kw)
        return self.filters[key]

    def close(self):
        for f in self.filters.values():
            f.close()
        self.filters.clear()
        self.sp.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def second_pass(case_id):
    """the reference applied to the reference's own first output (remnants and emptied reads included; no pairs)"""
    seqs, quals, names = ac.reference(case_id)[1]
    return ac.reference_filter(case_id).apply(seqs, quals, None, names)


def offsets_of(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return off


def assert_equal(what, got, frs, want, after, names):
    for key in KEYS:
        bad = np.nonzero(got[key] != want[key])[0]
        assert bad.size == 0, (what, key, bad[:5], got[key][bad[:5]], want[key][bad[:5]])
    b, q, off, got_names = frs.arrays()
    assert frs.n == len(after[0]) and np.array_equal(off, offsets_of(after[0])), what
    assert b.tobytes() == b"".join(after[0]) and q.tobytes() == b"".join(after[1]), what
    assert got_names == (after[2] if names else [b""] * frs.n), what


@pytest.mark.parametrize("case_id", ac.ids())
def test_family_equals_the_reference(dev, case_id):
    c = ac.CASES[case_id]
    batch = c.batch()
    f = dev.filter(c.kw, c.fasta)
    flt = ac.reference_filter(case_id)
    assert (f.n_sequences, f.n_filter_kmers, f.remaining_edits) == (flt.n_seq, len(flt.table), flt.num_errors)
    if batch.names:
        rs = ka.ReadSet(dev.sp, batch.fastq(), input_quality_base=33)
        names = True
    else:
        rs = ka.ReadSet.from_arrays(dev.sp, *batch.arrays())
        names = False
    assert rs.n == batch.n
    want, after = ac.reference(case_id)
    want2, after2 = second_pass(case_id)
    if names:          # what the device shows of a name (it keeps the comment apart): carried means the input read's, unchanged
        shown = dict(zip(batch.names, rs.arrays()[3]))
        assert all(shown[nm] and nm.startswith(shown[nm]) for nm in batch.names) and len(set(shown.values())) == batch.n
        after = (after[0], after[1], [shown[nm] for nm in after[2]])
        after2 = (after2[0], after2[1], [shown[nm] for nm in after2[2]])
    got, frs = f.applyFilter(rs, batch.mate)
    assert_equal((case_id, "first pass"), got, frs, want, after, names)
    got2, frs2 = f.applyFilter(frs)
    assert_equal((case_id, "second pass"), got2, frs2, want2, after2, names)
    for r in (frs2, frs, rs):
        r.close()


@pytest.mark.parametrize("kw", [dict(ac.CLASSES), dict(match_length=12), dict(match_length=20), dict(match_length=28, **ac.CLASSES)])
def test_exact_filter_set_equals_the_references_own(dev, kw):
    """nothing built in: the canonical windows of the circularised sequences as refartifact computes them itself"""
    kw = dict(kw, build_edits=0)
    f = dev.filter(kw, ac.FASTA)
    flt = ra.Filter(ra.Config(**kw), ac.FASTA)
    kr, vr = flt.entries()
    kd, vd = f.entries()
    assert (f.n_sequences, f.n_filter_kmers, f.remaining_edits) == (flt.n_seq, kr.size, flt.num_errors)
    assert np.array_equal(kd, kr) and np.array_equal(vd, vr)


@pytest.mark.parametrize("kw", [dict(edit_distance=1), dict(edit_distance=2), dict(edit_distance=1, match_length=12),
                                dict(edit_distance=1, match_length=20), dict(edit_distance=1, match_length=28), dict(edit_distance=2, match_length=12, **ac.CLASSES)])
def test_built_in_filter_set_equals_the_oracles(dev, kw):
    """substitutions built in: the first writer in the reference map's iteration order keeps a key -- held to the oracle (lookup3)"""
    o = OracleArtifactFilter(artifact_config(**kw), ac.FASTA)
    f = dev.filter(kw, ac.FASTA)
    assert (f.n_sequences, f.n_filter_kmers, f.remaining_edits) == o.info() and f.remaining_edits == 0
    ko, vo = o.entries()
    kd, vd = f.entries()
    assert np.array_equal(kd, ko) and np.array_equal(vd, vo)
