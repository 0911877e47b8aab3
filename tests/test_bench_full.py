"""bench.py: a plain run prints the headline and nothing it did not need to measure it; --full adds every other figure and check
(the compacted clouds leg, the side figures, the CPU baseline with its check of one view of the GPU result, the host buffer paths)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config", "roofline"}
FULL_KEYS = {"to_compacted_clouds", "side", "cpu_baseline", "host_buffers_one_view", "host_buffers_pipelined", "set_mask_us"}


def _bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=timeout)


def _line(p):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_shim_timing_needs_full():
    p = _bench("--shim-timing")
    assert p.returncode == 2 and "--full" in p.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_full_adds_the_rest():
    plain = _line(_bench("--gpus", "1", "--steps", "20", "--warmup", "5"))
    assert set(plain) == HEADLINE_KEYS, sorted(set(plain) ^ HEADLINE_KEYS)
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and "device_copy" not in plain["roofline"]

    full = _line(_bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--idle-samples", "3", "--idle-sleep", "0.05"))
    assert set(full) == HEADLINE_KEYS | FULL_KEYS, sorted(set(full) ^ (HEADLINE_KEYS | FULL_KEYS))
    assert full["metric"] == plain["metric"] and full["roofline"]["kernel"] == plain["roofline"]["kernel"]
    assert full["to_compacted_clouds"]["value"] > 0 and "error" not in full["to_compacted_clouds"]
    s = full["side"]
    assert "error" not in s and s["cold_20_steps"]["value"] > 0 and s["config2_12mp"]["value"] > 0
    assert {"resident", "with_upload"} <= set(s["one_scan_from_idle"])
    assert full["roofline"]["device_copy"]["GBps"] > 0
    c = full["cpu_baseline"]
    assert c["value"] > 0 and c["gpu_matches_oracle"]["valid_map_bit_exact"] is True and c["gpu_matches_oracle"]["max_rel_point_error"] <= 1e-5
    assert full["host_buffers_pipelined"]["equals_resident_result"] is True
