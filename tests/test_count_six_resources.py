"""What the compiler gives the six-block instance of the one-weight, one-word count pass over super-k-mer lists
(sk_count_kernel<1, COUNT_LOG2S, false, false, true, false, 6>, kmr_tune "count_six").  Six wavefronts per SIMD leave a wavefront 80
vector registers (512 over six, in allocation granules of eight), and six blocks share the CU's 160 KB of LDS -- which they only fit
with table slots of 20 bytes: the instance is worth launching as six blocks per CU only while it stays inside both, without a
spilled vector register and without scratch memory.  The instances beside it must still be there, once each.

No GPU: as in test_count_instance_resources.py, kmr_inst.hip is compiled for the device alone with the flags the Makefile gives the
count pass's translation units, and the kernels' metadata (.amdhsa notes of the assembly) is read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmernator_amd", "csrc")

LDS_PER_CU = 163840          # gfx950: 160 KB per compute unit
VGPRS_SIX_WAVES = 80         # 512 registers per SIMD lane over six wavefronts, in allocation granules of eight
FIELDS = "vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size"


def _make_var(text, name):
    m = re.search(r"^%s \?= (.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """[(mangled name, {metadata field: int})] of every sk_count_kernel instance of the one-word translation unit"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    out = str(tmp_path_factory.mktemp("skc6") / "skc1.s")
    cmd = [hipcc] + _make_var(mk, "HIPFLAGS") + _make_var(mk, "SKC_FLAGS") + ["-DKMR_INST_SKC", "-DKMR_INST_W=1", "--cuda-device-only", "-S", "-o", out,
                                                                             os.path.join(CSRC, "kmr_inst.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC, timeout=600)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = []
    for block in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "sk_count_kernel" not in name.group(1):
            continue
        res.append((name.group(1), {f: int(v) for f, v in re.findall(r"\.(%s):\s+(\d+)" % FIELDS, block)}))
    return res


def _instances(kernels, blocks):
    """the list instances <W = 1, LOG2S = 10, TRACK = false, EXT = false, UNI = true, ITEM = false, BLOCKS>"""
    tag = "sk_count_kernelILi1ELi10ELb0ELb0ELb1ELb0ELi%dEEE" % blocks
    return [v for n, v in kernels if tag in n]


def _dynamic_lds_six():
    """sk_count_smem_bytes<1, 10, false, false, true, true>(): 1024 slots of 20 bytes (key, count | forward, a first-sighting word of 32
    bits), 256 staged granules of 16 bytes, 256 bytes of wrecOf[], 64 spare"""
    return 1024 * 20 + 256 * 16 + 256 + 64


def test_six_block_instance_fits_six_to_a_cu(kernels):
    hits = _instances(kernels, 6)
    assert len(hits) == 1, [n for n, _ in kernels]
    six = hits[0]
    print("six-block instance:", six, "dynamic LDS", _dynamic_lds_six())
    assert six["vgpr_count"] <= VGPRS_SIX_WAVES
    assert six["vgpr_spill_count"] == 0
    assert six["private_segment_fixed_size"] == 0      # no scratch at all
    assert (six["group_segment_fixed_size"] + _dynamic_lds_six()) * 6 <= LDS_PER_CU


def test_five_and_four_block_instances_exist_once(kernels):
    assert len(_instances(kernels, 5)) == 1
    assert len(_instances(kernels, 0)) == 1
