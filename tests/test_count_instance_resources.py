"""What the compiler gives the two instances of the one-weight, one-word count pass over super-k-mer lists
(sk_count_kernel<1, COUNT_LOG2S, false, false, true, false, BLOCKS>): the four-block one (BLOCKS = 0) and the five-block one that
kmr_tune "count_blocks" selects.  Five wavefronts per SIMD leave a wavefront 96 vector registers, and five blocks share the CU's
160 KB of LDS: the instance is only worth launching as five blocks per CU while it stays inside both, without scratch memory.

No GPU: kmr_inst.hip is compiled for the device alone, with the flags the Makefile gives the count pass's translation units, and the
kernels' metadata (.amdhsa notes of the assembly) is read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmernator_amd", "csrc")

LDS_PER_CU = 163840          # gfx950: 160 KB per compute unit
VGPRS_FIVE_WAVES = 96        # 512 registers per SIMD lane over five wavefronts, in allocation granules of eight
# vector registers the five-block instance may spill: none.  (As first compiled, with the four-block instance's code, it spilled 14:
# wave-uniform values -- slab cursors, kept counters, the prefetch's list -- that the compiler kept per lane; the instance now takes
# them as scalars)
SPILL_CEILING = 0


def _make_var(text, name):
    m = re.search(r"^%s \?= (.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: {metadata field: int}} of every sk_count_kernel instance of the one-word translation unit"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    out = str(tmp_path_factory.mktemp("skc") / "skc1.s")
    cmd = [hipcc] + _make_var(mk, "HIPFLAGS") + _make_var(mk, "SKC_FLAGS") + ["-DKMR_INST_SKC", "-DKMR_INST_W=1", "--cuda-device-only", "-S", "-o", out,
                                                                             os.path.join(CSRC, "kmr_inst.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC, timeout=600)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = {}
    for block in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "sk_count_kernel" not in name.group(1):
            continue
        res[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", block)}
    return res


def _instance(kernels, blocks):
    """the list instance <W = 1, LOG2S = 10, TRACK = false, EXT = false, UNI = true, ITEM = false, BLOCKS>"""
    tag = "sk_count_kernelILi1ELi10ELb0ELb0ELb1ELb0ELi%dEEE" % blocks
    hits = [v for n, v in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, sorted(kernels))
    return hits[0]


def _dynamic_lds():
    """sk_count_smem_bytes<1, 10, false, false, true>(): 1024 slots of 24 bytes (key, count | forward, first sighting; no weight sum),
    256 staged granules of 16 bytes, 256 bytes of wrecOf[], 64 spare"""
    return 1024 * 24 + 256 * 16 + 256 + 64


def test_five_block_instance_fits_five_to_a_cu(kernels):
    five = _instance(kernels, 5)
    print("five-block instance:", five, "dynamic LDS", _dynamic_lds())
    assert five["vgpr_count"] <= VGPRS_FIVE_WAVES
    assert (five["group_segment_fixed_size"] + _dynamic_lds()) * 5 <= LDS_PER_CU
    assert five["vgpr_spill_count"] <= SPILL_CEILING and five["private_segment_fixed_size"] == 0      # no scratch at all


def test_four_block_instance_still_spills_no_vector_register(kernels):
    four = _instance(kernels, 0)
    print("four-block instance:", four)
    assert four["vgpr_spill_count"] == 0 and four["private_segment_fixed_size"] == 0
    assert four["vgpr_count"] <= 128
    assert (four["group_segment_fixed_size"] + _dynamic_lds()) * 4 <= LDS_PER_CU
