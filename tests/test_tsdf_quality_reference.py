"""What volumetric fusion by the rule of include/sl3d_tsdf.h gives, on the restatement alone (tests/tsdf_reference.py; the GPU twin,
tests/test_gpu_tsdf_scene.py, holds the library to these very planes and this very surface, bit for bit).

The scene is the ray-cast turntable scene of tests/align_reference.py -- an ellipsoid and a sphere, 160 x 120 pixels, 4 views 20 degrees
apart -- fused with the true estimate: voxel 1.0 mm, trunc 3.0 mm, min_weight 1, the volume around the registered cloud plus 2 voxels.
The distance of a point to the true surfaces is taken to first order, |F| / |grad F|.

Noise-free, the restatement's crossings lie 0.0279 mm rms from the surfaces (4,934 crossings in a volume of 69 x 64 x 28); the
bar is twice that figure, NOISE_FREE_BAR = 0.0558 mm -- the margin covers the first-order distance measure and another choice of bounds.
With 0.3 mm of Gaussian depth noise along the ray (a fixed seed) the crossings must lie at most half as far from the surfaces, rms, as
the registered noisy cloud itself, computed here: the restatement gives 0.0769 mm against 0.2273 mm, a ratio of 0.34.  In both cases at
least 95 % of the noise-free registered points must have a crossing within 2 voxels -- a condition against an empty result, not a
measurement; the restatement reaches 99.4 %."""
import numpy as np
import pytest

import tsdf_cases as TC

RESTATEMENT_RMS = 0.0279                                                    # mm, the noise-free figure of the restatement itself
NOISE_FREE_BAR = 2.0 * RESTATEMENT_RMS
NOISE_RATIO_BAR = 0.5
COVERAGE_BAR = 0.95


def _rms(d):
    return float(np.sqrt((d * d).mean()))


@pytest.fixture(scope="module")
def clean_cloud():
    return TC.fused_scene(0.0)["cloud"]


def test_noise_free_crossings_lie_on_the_surfaces(clean_cloud):
    f = TC.fused_scene(0.0)
    assert _rms(TC.surface_distance(f["cam"], f["cloud"])) < 1e-5           # the registered cloud itself lies on them: the estimate is the truth
    rms = _rms(TC.surface_distance(f["cam"], f["xyz"]))
    cover = TC.coverage(clean_cloud, f["xyz"], 2.0 * float(TC.SCENE["voxel"]))
    print(f"noise-free: volume {f['vol']['dims']}, samples {f['counts'][0]}, stats {f['stats']}, rms of the crossings {rms:.4f} mm, coverage {cover:.4f}")
    assert f["stats"][2] == len(f["xyz"]) > 1000
    assert rms <= NOISE_FREE_BAR
    assert cover >= COVERAGE_BAR


def test_fusion_averages_depth_noise(clean_cloud):
    f = TC.fused_scene(TC.SCENE["sigma"])
    cloud_rms = _rms(TC.surface_distance(f["cam"], f["cloud"]))
    rms = _rms(TC.surface_distance(f["cam"], f["xyz"]))
    cover = TC.coverage(clean_cloud, f["xyz"], 2.0 * float(TC.SCENE["voxel"]))
    print(f"sigma {TC.SCENE['sigma']} mm: registered cloud {cloud_rms:.4f} mm rms, crossings {rms:.4f} mm rms (ratio {rms / cloud_rms:.3f}), "
          f"{len(f['xyz'])} crossings, coverage {cover:.4f}")
    assert 0.15 < cloud_rms < 0.3                                           # (the noise is there: sigma along the ray, seen along the normal)
    assert rms <= NOISE_RATIO_BAR * cloud_rms
    assert cover >= COVERAGE_BAR


def test_the_normals_point_out_of_the_object():
    f = TC.fused_scene(0.0)
    n, p = f["normals"].astype(np.float64), f["xyz"].astype(np.float64)
    assert np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    # against the true outward normal of the nearer surface: grad F
    best, true = np.full(len(p), np.inf), np.zeros_like(p)
    for c, s in TC.scene_shapes(f["cam"]):
        e = (p - c) / s
        d = np.abs((e * e).sum(axis=1) - 1.0) / np.linalg.norm(2.0 * e / s, axis=1)
        g = e / s
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        true[d < best], best = g[d < best], np.minimum(d, best)
    cos = (n * true).sum(axis=1)
    print(f"normals: median angle to the truth {np.degrees(np.arccos(np.clip(np.median(cos), -1, 1))):.2f} deg, share within 30 deg {(cos > np.cos(np.radians(30))).mean():.4f}")
    assert (cos > 0.0).mean() > 0.99 and np.median(cos) > np.cos(np.radians(10.0))
