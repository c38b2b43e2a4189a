"""bench.py end to end at a small size.  A plain run prints the headline and what its timed steps measured; --full adds what
takes runs or checks of its own: the CPU baseline, the PCIe-inclusive legs and the oracle check."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "h2d", "value_incl_h2d", "oracle_check")


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--warmup", "1"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full is True


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_line(full):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--reads", "200000"]
    if full:
        cmd += ["--full", "--cpu-reads", "20000"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE)
    assert d["value"] > 0 and d["unit"] == "kmers/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    assert d["config"]["total_kmers"] == 200000 * 120 and d["steps"] == 2 and d["warmup"] == 1
    assert d["roofline"]["kernels"] and d["roofline"]["frac"] > 0
    if full:
        assert all(k in d for k in FULL_ONLY)
        assert d["cpu_baseline"]["value"] > 0 and d["value_incl_h2d"] > 0 and d["h2d"]["as_text"]["value_incl_h2d"] > 0
        assert d["oracle_check"] is None           # no committed digest at this size
    else:
        assert not any(k in d for k in FULL_ONLY)
