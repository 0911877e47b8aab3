"""GPU tests (-m gpu) of the row clip of the newest vertical-neighbourhood readers against the rows of the neighbouring views:
ALIGN_SEARCH under k_align_pass<WINDOW> and k_align_plane_pass<WINDOW>, the stencil of k_align_normals, and tsdf_cell / tsdf_sample_plane
under k_tsdf_integrate, each against its NumPy restatement (tests/align_reference.py, tests/align_plane_reference.py,
tests/tsdf_reference.py) word for word, with the camera taken from sl3d_get_align_camera.

A context stacks its views without a gap, so row -1 of view v is the last row of view v - 1 and row H the first row of view v + 1.  The
inputs (tests/view_seams.py) put there what a reader without the clip would take; tests/test_view_seam_cases.py shows on the CPU that
every such reading changes the result, and the cheap part of that is repeated here under the device's camera before the device is
called.  Every context has four views, a window origin of (37, 5) in a 320 x 240 frame, and poisoned padding columns.

1. sl3d_align_sums and sl3d_align_plane_sums at 3 x 2, 9 x 5, 67 x 19 and 130 x 37 and windows 0 .. 4, over the views (0, 4), (1, 2) -- the one
   pair with both neighbours --, (1, 3) and (2, 2); the planes of all four views are unchanged afterwards.
2. sl3d_align_normals over (1, 1), (1, 2) and (0, 4) on the smooth views: every plane bit for bit, rows 0 and H - 1 NaN throughout.
3. sl3d_tsdf_integrate at 20 x 6 and 67 x 19 with a volume that reaches past the frame's top and bottom rows: all views, the views
   1 .. V - 2 at first_step 1, two calls that must equal one; sum, weight, the counts; the surface at min_weight 1 and 2."""
import numpy as np
import pytest

import align_plane_reference as PR
import align_reference as AR
import tsdf_cases as TC
import view_seams as VS
from dense_planes import dense_layout
from test_view_seam_cases import (EDGE, MAX_DIST, ORIGIN, RANGE, SHAPES, TSDF_SHAPES, V, WINDOWS, align_purpose, fused, normals_purpose,
                                  quantisation_centre, tsdf_purpose)
from tsdf_gpu import check_planes, check_surface, context, put, reset, same_bits

pytestmark = pytest.mark.gpu

SPANS = ((0, 4), (1, 2), (1, 3), (2, 2))                                    # (first view, views): the pairs first .. first + views - 2


def _put_all(sc, points, valid, pads):
    assert (TC.FULL, TC.ORIGIN) == ((320, 240), ORIGIN) and dense_layout(sc, 0)[4] > sc.W       # there are padding columns to poison
    for v in range(V):
        put(sc, v, points[v], valid[v], pads[v])


def _planes_are(sc, points, valid):
    for v in range(V):
        xyz, val = sc.points(v)
        assert same_bits(xyz, points[v]) and np.array_equal(val, valid[v]), v


def _same_plane(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_pass_seams(W, H):
    with context(W, H, V) as sc:
        cam = sc.align_camera()
        points, valid, pads, est, made = align_purpose(cam, W, H, windows=(0, 1))      # extended != clipped, under this camera
        assert made == 2 * 2 * (1 + 2 * (V - 2))
        _put_all(sc, points, valid, pads)
        ox, oz = quantisation_centre(est)
        nrm = [PR.normals(points[v], valid[v], EDGE) for v in range(V - 1)]
        for window in WINDOWS:
            want = AR.pass_sums(points, valid, cam, *ORIGIN, est, ox, oz, RANGE, MAX_DIST, window)
            plane = PR.pass_sums(points, valid, cam, *ORIGIN, est, ox, oz, RANGE, MAX_DIST, EDGE, window, nrm)
            assert want.shape == (V - 1, 12) and plane.shape == (V - 1, 18)
            for first, n in SPANS:
                got = sc.align_sums(first, n, est, ox, oz, RANGE, MAX_DIST, window)
                assert got.dtype == np.int64 and np.array_equal(got, want[first:first + n - 1]), (window, first, n)
                got = sc.align_plane_sums(first, n, est, ox, oz, RANGE, MAX_DIST, EDGE, window)
                assert got.dtype == np.int64 and np.array_equal(got, plane[first:first + n - 1]), (window, first, n)
        assert np.array_equal(sc.align_plane_sums(0, V, est, ox, oz, RANGE, MAX_DIST, EDGE, window), plane)
        for v in range(V - 1):                                              # that pass's own normals: rows 0 and H - 1 hold none
            assert _same_plane(sc.align_normal_plane(v), nrm[v]), v
        _planes_are(sc, points, valid)


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_normal_seams(W, H):
    with context(W, H, V) as sc:
        cam = sc.align_camera()
        points, valid, pads = normals_purpose(cam, W, H)                    # with the neighbours' rows, rows 0 and H - 1 have normals
        for k, (first, n) in enumerate(((1, 1), (1, 2), (0, 4))):
            holed = valid.copy()
            if H >= 3:                                                       # another pixel without a point before every call: no plane
                holed[:, H // 2, 1 + k % (W - 2)] = 0                        # of an earlier call passes for this one's
            _put_all(sc, points, holed, pads)
            sc.align_normals(first, n, VS.NORMAL_EDGE)
            for v in range(first, first + n):
                want = PR.normals(points[v], holed[v], VS.NORMAL_EDGE)
                got = sc.align_normal_plane(v)
                assert _same_plane(got, want), (first, n, v)
                assert np.isnan(got[0]).all() and np.isnan(got[H - 1]).all(), (first, n, v)
                if H >= 3:                                                   # the hole and its neighbours have none, the others have
                    assert 0 < int((~np.isnan(want[..., 0])).sum()) < (W - 2) * (H - 2)
            _planes_are(sc, points, holed)


@pytest.mark.parametrize("W,H", TSDF_SHAPES, ids=[f"{w}x{h}" for w, h in TSDF_SHAPES])
def test_tsdf_seams(W, H):
    with context(W, H, V) as sc:
        cam = sc.align_camera()
        points, valid, pads, est, vol = tsdf_purpose(cam, W, H, spans=((1, V - 2, 1),))      # extended != clipped, under this camera
        _put_all(sc, points, valid, pads)

        def want(first, n, first_step):
            return fused(vol, points[first:first + n], valid[first:first + n], cam, est, first_step)
        sV, wV, cV = want(0, V, 0)
        for first, n, first_step, (s, w, counts) in ((0, V, 0, (sV, wV, cV)), (1, V - 2, 1, want(1, V - 2, 1))):
            reset(sc, vol)
            assert sc.tsdf_integrate(first, n, est, first_step) == counts, (first, n, first_step)
            check_planes(sc, vol, s, w)
        c1 = want(0, 1, 0)[2]                                                # two calls equal one call over the same views
        reset(sc, vol)
        assert sc.tsdf_integrate(0, 1, est, 0) == c1
        assert sc.tsdf_integrate(1, V - 1, est, 1) == [cV[0] - c1[0], cV[1]]
        check_planes(sc, vol, sV, wV)
        for mw in (1, 2):
            edge, stats = check_surface(sc, sV, wV, vol, mw)[2:]
            assert stats[2] >= 1 and np.all(np.diff(edge) > 0)
        _planes_are(sc, points, valid)
