"""Every directed case of tests/dedupcases.py through DuplicateFragmentFilter on the device against the restatement of
tests/refdedup.py, with the `check` of tests/test_gpu_dedup.py: discard flags, the four skip counters, affected, the group list and
the consensus batch's bases, qualities, lengths and names, byte for byte.  tests/test_dedup_cases.py proves on the CPU that the
cases reach the edges they are named for.  Each case runs from host text (or, where it has no names, from arrays); one case per
family runs from device text as well.  A handle's tables are made by its first dedup call, so every handle configuration gets a
handle of its own."""
import functools

import numpy as np
import pytest

import kmernator_amd as ka
import dedupcases as dc
import refdedup
from test_gpu_dedup import check, device_text_of

pytestmark = pytest.mark.gpu
K = 31


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def cases(family):
    return dc.family(family, cu_count()) if family == "M" else dc.family(family)


@functools.lru_cache(maxsize=None)
def wanted(family, index):
    """the restatement's results and pair list of a case, computed once for the host-text and the device-text run"""
    case = cases(family)[index]
    return dc.run(case), dc.pair_list(case)


class Handles:
    """one KmerSpectrum per handle configuration"""

    def __init__(self):
        self.by_cfg = {}

    def get(self, handle_cfg):
        key = tuple(sorted(handle_cfg.items()))
        if key not in self.by_cfg:
            self.by_cfg[key] = ka.KmerSpectrum(ka.default_config(K, estimated_raw_kmers=1 << 16, device=0, **handle_cfg))
        return self.by_cfg[key]


def read_set(sp, case):
    _, reads, _, cfg, _, _ = case
    if cfg["named"]:
        return ka.ReadSet(sp, refdedup.fastq_text(reads), store_comment=bool(cfg["store_comment"]))
    bases = np.frombuffer("".join(r[1] for r in reads).encode("latin-1"), dtype=np.uint8)
    quals = np.frombuffer("".join(r[2] for r in reads).encode("latin-1"), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.uint64)
    assert bases.size == quals.size == int(offsets[-1])
    return ka.ReadSet.from_arrays(sp, bases, quals, offsets)


def run_case(handles, family, index, from_device_text=False):
    case = cases(family)[index]
    label, reads, discarded, cfg, handle_cfg, _ = case
    want, pair_list = wanted(family, index)
    sp = handles.get(handle_cfg)
    rs = read_set(sp, case)
    assert rs.n == len(reads), label
    b, q, _, _ = rs.arrays()
    assert q.tobytes() == "".join(r[2] for r in reads).encode("latin-1"), label          # the batch holds the bytes the restatement is given
    assert b.tobytes() == "".join(r[1] for r in reads).upper().encode("latin-1") if cfg["named"] else b.tobytes() == "".join(r[1] for r in reads).encode("latin-1"), label
    pairs = rs.identifyPairs()
    assert [tuple(p) for p in pairs.pairs.tolist()] == pair_list, label
    dt = ptr = None
    if from_device_text:
        dt = device_text_of(rs) if rs.text else None
        ptr = dt.data_ptr() if dt is not None else 0          # a batch without names has no text: a null pointer and no bytes
    f = ka.DuplicateFragmentFilter(sp, cfg["dedup_mode"], cfg["dedup_length"], cfg["start_offset"])
    if cfg["passes"] == "both":
        res = f.filterDuplicateFragments(rs, pairs, discarded, dedup_single=True, device_text=ptr)
        check(res, want[0], label + " paired")
        check(res.single, want[1], label + " single")
    else:
        res = f._pass(rs, pairs, discarded, cfg["passes"] == "paired", ptr)
        check(res, want[0], label)
    res.close()
    pairs.close()
    rs.close()


@pytest.mark.parametrize("dedup_length", dc.LENGTHS)
def test_geometry(dedup_length):
    """G: four start offsets x two modes, each as the paired pass followed by the single pass"""
    handles = Handles()
    at = [i for i, c in enumerate(cases("G")) if c[3]["dedup_length"] == dedup_length]
    assert len(at) == 8
    for i in at:
        run_case(handles, "G", i)


@pytest.mark.parametrize("dedup_length", dc.K_LENGTHS)
def test_multi_word_keys(dedup_length):
    handles = Handles()
    at = [i for i, c in enumerate(cases("K")) if c[3]["dedup_length"] == dedup_length]
    assert len(at) == 2
    for i in at:
        run_case(handles, "K", i)


def _ids(family):
    return [c[0] for c in dc.family(family)]


@pytest.mark.parametrize("index", range(len(dc.family("Q"))), ids=_ids("Q"))
def test_quality_ladder(index):
    run_case(Handles(), "Q", index)


@pytest.mark.parametrize("index", range(len(dc.family("D"))), ids=_ids("D"))
def test_disagreement(index):
    run_case(Handles(), "D", index)


@pytest.mark.parametrize("index", range(len(dc.family("S"))), ids=_ids("S"))
def test_stops_and_lengths(index):
    run_case(Handles(), "S", index)


@pytest.mark.parametrize("index", range(len(dc.family("W"))), ids=_ids("W"))
def test_wrapped_count(index):
    run_case(Handles(), "W", index)


@pytest.mark.parametrize("index", range(len(dc.family("F"))), ids=_ids("F"))
def test_flips_sides_and_names(index):
    run_case(Handles(), "F", index)


@pytest.mark.parametrize("index", range(len(dc.family("P"))), ids=_ids("P"))
def test_pair_list_shapes(index):
    run_case(Handles(), "P", index)


@pytest.mark.parametrize("index", (0, 1), ids=("paired", "single"))
def test_many_groups(index):
    """more (group, side) tasks than two grids of the consensus kernel on this device hold"""
    case = cases("M")[index]
    sides = 2 if case[3]["passes"] == "paired" else 1
    want, _ = wanted("M", index)
    assert len(want[0].groups) * sides > 2 * 8 * cu_count() * 4
    run_case(Handles(), "M", index)


# one case per family from device text: W's is the wrap itself, Q's has no text at all
DEVICE_TEXT = {"G": 45, "K": 5, "Q": 0, "D": 0, "S": 0, "W": 1, "F": 1, "P": 0, "M": 0}


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_from_device_text(family):
    run_case(Handles(), family, DEVICE_TEXT[family], from_device_text=True)
