"""The recovery of the turntable's step and axis by the rule of include/sl3d_align.h, on the restatement alone (tests/align_reference.py; the
GPU twin, tests/test_gpu_align_refine.py, holds the library to this very loop).

The scene is ray-cast in NumPy float64 through the test's camera (the package's synthetic rig at 160 x 120, radially distorted): an
ellipsoid of three different semi-axes whose centre is off the turntable axis and a smaller sphere beside it, 4 views, step 20 degrees.
The refinement starts from a step 1.5 degrees too large and an axis 1.8 mm off.  What is asserted is the bar the feature was given:
the first pass accepts at least half of its sources; after at most 20 iterations the step error and the axis distance are both below
their starting values; rms_xz of the last pass is below that of the first.  The figures the restatement reaches are printed and written
down in DESIGN 4w; nothing else is claimed -- point-to-point ICP over projective correspondences settles on a biased estimate, about half
a degree and 0.7 mm on this scene (0.527 degrees, 0.656 mm), and started from the truth it drifts to one like it (0.60 degrees, 0.75 mm)."""
import numpy as np
import pytest

import align_reference as AR

S = AR.SCENE


@pytest.fixture(scope="module")
def scene():
    cal = AR.scene_calibration()
    cam = AR.camera_of(cal[0], cal[1], cal[2], cal[3])
    points, valid, truth = AR.raycast_scene(cam)
    return cam, points, valid, truth


def test_the_scene_is_what_it_says(scene):
    cam, points, valid, truth = scene
    assert points.shape == (4, 120, 160, 3) and valid.shape == (4, 120, 160)
    assert (valid.reshape(4, -1).sum(axis=1) > 2500).all() and np.isfinite(points[valid == 1]).all() and np.isnan(points[valid == 0]).all()
    # every point projects to its own pixel, and a view turned by the true step lies on the view before it
    for v in range(4):
        p = points[v][valid[v] == 1]
        cc, rr, ok = AR.centre(p.astype(np.float64), cam, 0, 0)
        r, c = np.nonzero(valid[v] == 1)
        assert ok.all() and np.array_equal(cc, c) and np.array_equal(rr, r)
    words = AR.pass_sums(points, valid, cam, 0, 0, truth, truth[2], truth[3], S["rng"], 0.75, S["window"])
    assert (words[:, 0] > 0.8 * words[:, 11]).all()                        # (what is not matched has turned out of sight)
    body = points[0][valid[0] == 1].astype(np.float64)
    assert np.hypot(body[:, 0].mean() - truth[2], body[:, 2].mean() - truth[3]) > 5.0    # the body's centre is off the axis


def test_recovery_from_a_perturbed_start(scene):
    cam, points, valid, truth = scene
    tx, ty, tz, rot = AR.scene_start(truth)
    out = AR.refine(points, valid, cam, 0, 0, tx, ty, tz, rot, S["rng"], S["max_dist"], S["window"], S["iterations"])
    log = out["log"]
    first, last = AR.errors(log[0]["est"], truth), AR.errors(out["est"], truth)
    print(f"start: step error {first[0]:.4f} deg, axis {first[1]:.4f} mm, rms_xz {log[0]['rms_xz']:.4f} mm, accepted {log[0]['n']} of {log[0]['sources']}")
    print(f"after {out['n_done']} iterations: step error {last[0]:.4f} deg, axis {last[1]:.4f} mm, rms_xz {log[-1]['rms_xz']:.4f} mm, "
          f"rms_y {log[-1]['rms_y']:.4f} mm, accepted {log[-1]['n']} of {log[-1]['sources']}")
    assert abs(first[0] - 1.5) < 1e-3 and abs(first[1] - np.hypot(1.5, 1.0)) < 1e-3      # the start is the perturbation
    assert 2 * log[0]["n"] >= log[0]["sources"] > 0                        # the first pass accepts at least half of its sources
    assert out["n_done"] <= 20 and not out["degenerate"]
    assert last[0] < first[0] and last[1] < first[1]
    assert log[-1]["rms_xz"] < log[0]["rms_xz"]
    assert out["ty"] == ty and out["n"] == log[-1]["n"] and out["rms_xz"] == log[-1]["rms_xz"]
    # the result in the registration's units: back through the registration's own conversion it is the estimate
    a = float(out["rot_step"]) * 22.0 / 7.0 / 180.0
    assert abs(np.cos(a) - out["est"][0]) < 1e-6 and abs(np.sin(a) - out["est"][1]) < 1e-6
    assert out["tx"] == np.float32(out["est"][2]) and out["tz"] == np.float32(out["est"][3])
