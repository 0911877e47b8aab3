"""bench.py --dump-outputs: the results of the last timed launch land in DIR as float32 / float64 .npy files (at most 64 MB; a
fixed seeded sample of the pixels when the batch is larger), and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

COMMON = ["--warmup", "1", "--precondition-ms", "0", "--no-cpu-baseline", "--no-side", "--no-clouds"]


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)


def _line(p):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("pixel_index", "xyz", "valid")}


def test_dump_outputs_arguments_are_checked_before_the_gpu(tmp_path):
    for argv in (["--gpus", "2"], ["--idle-only"], ["--families-only"], ["--one-view-cold-only"]):
        p = _bench(*argv, "--dump-outputs", str(tmp_path / "d"))
        assert p.returncode == 2 and "--dump-outputs" in p.stderr, argv
    p = _bench("--steps", "0")
    assert p.returncode == 2 and "--steps" in p.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,views,sampled", [(320, 240, 2, False), (640, 480, 8, True)])
def test_dump_outputs_repeat_exactly(tmp_path, width, height, views, sampled):
    size = ["--width", str(width), "--height", str(height), "--views", str(views)]
    runs = []
    for k, steps in enumerate((3, 5)):
        d = str(tmp_path / f"run{k}")
        line = _line(_bench("--gpus", "1", "--steps", str(steps), *size, *COMMON, "--dump-outputs", d))
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["dump_outputs"]["dir"] == d and line["dump_outputs"]["of_pixels"] == views * width * height
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        runs.append(_load(d))
    a, b = runs
    assert a["pixel_index"].dtype == np.float64 and a["xyz"].dtype == np.float32 and a["valid"].dtype == np.float32
    idx = a["pixel_index"].astype(np.int64)
    n = len(idx)
    assert a["xyz"].shape == (n, 3) and a["valid"].shape == (n,)
    if sampled:
        assert n < views * width * height and (np.diff(idx) > 0).all() and idx[-1] < views * width * height
    else:
        assert np.array_equal(idx, np.arange(views * width * height))
    # finite everywhere: 0 where a pixel is invalid (the library's NaN), a point where it is valid; every view has valid pixels
    v = a["valid"] == 1
    assert np.isin(a["valid"], (0.0, 1.0)).all() and all(np.isfinite(x).all() for x in a.values())
    assert (a["xyz"][~v] == 0).all() and (~v).any() and (np.abs(a["xyz"][v]).sum(axis=1) > 0).all()
    assert len(np.unique(idx[v] // (width * height))) == views
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
