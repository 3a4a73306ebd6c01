"""bench.py without --full: one JSON line with the headline over the timed steps and the stage durations those
steps recorded, and none of the entries that run anything after them (replay, rooflines, CPU legs, verification,
streaming, sweep)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_alone():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--frames", "2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "blocks/s" and d["higher_is_better"] is True and d["dtype"].startswith("int32")
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["frames_per_gpu_per_step"] == 2
    assert abs(d["value"] - 2 * 3 * d["config"]["blocks_per_frame"] / (d["ms_per_step"] * 3e-3)) < 1e-3 * d["value"]
    assert d["price_margin_reruns"] is not None and d["theta_margin_reruns"] >= 0
    k = d["kernels"]
    assert "forward_pyramid_luma" in k and "pvq_ref_bands" in k
    assert all(e["launches"] > 0 and "exclusive_avg_ms" not in e for e in k.values())
    for key in ("roofline", "roofline_filter_dct", "pipelined_equals_serial", "step_counters", "single_frame_step",
                "streaming_input", "streaming_io", "cpu_baseline", "verified", "verification", "quality_sweep",
                "sharded_encode_check"):
        assert key not in d, key
