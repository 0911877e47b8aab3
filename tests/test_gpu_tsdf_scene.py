"""GPU test (-m gpu) of volumetric fusion on the ray-cast turntable scene: the four 160 x 120 views of
tests/align_reference.raycast_scene, written into a context's dense planes, are integrated on the device with the true estimate into the
volume of tests/test_tsdf_quality_reference.py -- voxel 1.0 mm, trunc 3.0 mm, the bounds of the registered cloud plus 2 voxels -- and
extracted at min_weight 1.  Both planes, both counts and the surface equal the restatement's bit for bit, so the bars the quality test
holds the restatement to -- the distance of the crossings to the true surfaces and their coverage of the scan -- hold for the device by
equality (the restatement runs through the device's own camera, whose rotation may differ from NumPy's in a last bit, and is held to
the noise-free bars here as well).  The views are integrated once in one call and once in two batches through two slots."""
import numpy as np
import pytest

import align_reference as AR
import tsdf_cases as TC
from conftest import pkg
from test_tsdf_quality_reference import COVERAGE_BAR, NOISE_FREE_BAR
from tsdf_gpu import check_planes, check_surface, put, reset

pytestmark = pytest.mark.gpu


def test_the_scene_fused_on_the_device():
    S = pkg("scanner")
    W, H, V = AR.SCENE["W"], AR.SCENE["H"], AR.SCENE["V"]
    with S.Scanner(W, H, 256, 256, 7, 7, 2, 2, max_views=V) as sc:
        sc.set_calibration(*AR.scene_calibration())
        sc.set_masks(np.ones((H, W), np.uint8))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
        sc.run(0, V)
        sc.synchronize()
        f = TC.fused_scene(0.0, cam=sc.align_camera())                    # the restatement through the device's own camera, fused once
        d = TC.surface_distance(f["cam"], f["xyz"])
        assert float(np.sqrt((d * d).mean())) <= NOISE_FREE_BAR and TC.coverage(f["cloud"], f["xyz"], 2.0 * float(TC.SCENE["voxel"])) >= COVERAGE_BAR
        for v in range(V):
            put(sc, v, np.array(f["points"][v]), np.array(f["valid"][v]))
        origin, dims = S.tsdf_bounds(f["cloud"], TC.SCENE["voxel"], TC.SCENE["margin"])
        assert np.array_equal(origin, f["vol"]["origin"]) and dims == f["vol"]["dims"]
        sc.tsdf_reset(origin, TC.SCENE["voxel"], TC.SCENE["trunc"], dims)
        assert sc.tsdf_integrate(0, V, f["truth"]) == list(f["counts"])
        check_planes(sc, f["vol"], f["sum"], f["weight"])
        xyz, nrm, edge, stats = check_surface(sc, f["sum"], f["weight"], f["vol"], TC.SCENE["min_weight"])
        assert stats == f["stats"] and len(edge) > 1000
        # in two batches through the slots 0 and 1: views 2 and 3 take the places of views 0 and 1
        reset(sc, f["vol"])
        first = sc.tsdf_integrate(0, 2, f["truth"])
        for v in (2, 3):
            put(sc, v - 2, np.array(f["points"][v]), np.array(f["valid"][v]))
        second = sc.tsdf_integrate(0, 2, f["truth"], first_step=2)
        assert first[0] + second[0] == f["counts"][0] and second[1] == f["counts"][1]
        check_planes(sc, f["vol"], f["sum"], f["weight"])
