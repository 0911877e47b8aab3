"""The recovery of the turntable's step and axis by the point-to-plane rule of include/sl3d_align_plane.h, on the restatement alone
(tests/align_plane_reference.py; the GPU twin, tests/test_gpu_align_plane_refine.py, holds the library to this very loop entry by entry).

The scene, the perturbed start, max_dist, window and the iteration budget are those of tests/test_align_recovery_reference.py
(align_reference.SCENE: ellipsoid off the axis and a sphere, 160 x 120, 4 views at 20 degrees, a start 1.5 degrees and 1.8 mm off);
normal_edge is 2 mm.  The bar is taken from the parent, not from the code under test: align_reference.refine, the point-to-point loop, runs
in the same test on the same scene and start, and the point-to-plane loop must end at most ONE TENTH as far from the truth in the step and
in the axis point -- from the perturbed start and from the truth itself.  It must stop by the repeated-words rule within the budget, and
its first pass must accept at least half of its sources.  The figures are printed; DESIGN 4x holds a copy."""
import numpy as np
import pytest

import align_plane_reference as PR
import align_reference as AR

S = AR.SCENE
NORMAL_EDGE = 2.0


@pytest.fixture(scope="module")
def scene():
    cal = AR.scene_calibration()
    cam = AR.camera_of(cal[0], cal[1], cal[2], cal[3])
    points, valid, truth = AR.raycast_scene(cam)
    return cam, points, valid, truth


def _starts(truth):
    return {"perturbed": AR.scene_start(truth),
            "truth": (np.float32(truth[2]), np.float32(0.0), np.float32(truth[3]), AR.degrees_22_7(S["step_deg"]))}


@pytest.mark.parametrize("start", ["perturbed", "truth"])
def test_recovery_to_a_tenth_of_the_point_to_point_error(scene, start):
    cam, points, valid, truth = scene
    tx, ty, tz, rot = _starts(truth)[start]
    args = (points, valid, cam, 0, 0, tx, ty, tz, rot, S["rng"], S["max_dist"])
    parent = AR.refine(*args, S["window"], S["iterations"])
    out = PR.refine(*args, NORMAL_EDGE, S["window"], S["iterations"])
    log = out["log"]
    bar, first, last = AR.errors(parent["est"], truth), AR.errors(log[0]["est"], truth), AR.errors(out["est"], truth)
    print(f"{start} start: step error {first[0]:.4f} deg, axis {first[1]:.4f} mm; point-to-point after {parent['n_done']} iterations: "
          f"{bar[0]:.4f} deg, {bar[1]:.4f} mm")
    print(f"point-to-plane after {out['n_done']} iterations: step error {last[0]:.4f} deg (1/{bar[0] / last[0]:.0f}), axis {last[1]:.4f} mm "
          f"(1/{bar[1] / last[1]:.0f}), rms_plane {log[0]['rms_xz']:.4f} -> {log[-1]['rms_xz']:.4f} mm, accepted {log[-1]['n']} of "
          f"{log[-1]['sources']}, {log[-1]['lost']} lost to a missing normal")
    if start == "perturbed":
        assert abs(first[0] - 1.5) < 1e-3 and abs(first[1] - np.hypot(1.5, 1.0)) < 1e-3      # the start is the perturbation
    else:
        assert first[0] < 1e-4 and first[1] < 1e-4                                          # ... or the truth, as float32 holds it
    assert not out["degenerate"] and 2 <= out["n_done"] < S["iterations"]                   # stopped by the repeated-words rule, not the budget
    assert (log[-1]["n"], log[-1]["sources"], log[-1]["lost"]) == (log[-2]["n"], log[-2]["sources"], log[-2]["lost"])
    assert 2 * log[0]["n"] >= log[0]["sources"] > 0                                         # the first pass accepts at least half of its sources
    assert 10.0 * last[0] <= bar[0] and 10.0 * last[1] <= bar[1]                            # THE BAR: a tenth of the parent's errors
    assert out["ty"] == ty and out["n"] == log[-1]["n"] and out["rms_xz"] == log[-1]["rms_xz"] and np.isnan(out["rms_y"])
    a = float(out["rot_step"]) * 22.0 / 7.0 / 180.0                                         # back through the registration's own conversion
    assert abs(np.cos(a) - out["est"][0]) < 1e-6 and abs(np.sin(a) - out["est"][1]) < 1e-6
    assert out["tx"] == np.float32(out["est"][2]) and out["tz"] == np.float32(out["est"][3])


def test_the_loop_stops_on_repeated_words_exactly(scene):
    """by the restatement alone: the last two passes of the loop return the same 18 words per pair, and the one before does not"""
    cam, points, valid, truth = scene
    tx, ty, tz, rot = AR.scene_start(truth)
    out = PR.refine(points, valid, cam, 0, 0, tx, ty, tz, rot, S["rng"], S["max_dist"], NORMAL_EDGE, S["window"], S["iterations"])
    ox, oz = float(tx), float(tz)
    words = [PR.pass_sums(points, valid, cam, 0, 0, e["est"], ox, oz, S["rng"], S["max_dist"], NORMAL_EDGE, S["window"]) for e in out["log"]]
    assert np.array_equal(words[-1], words[-2]) and not any(np.array_equal(a, b) for a, b in zip(words[:-2], words[1:-1]))
    assert words[0].shape == (S["V"] - 1, 18) and (words[-1][:, 17] > 0).all() and (words[-1][:, 0] + words[-1][:, 17] <= words[-1][:, 16]).all()
