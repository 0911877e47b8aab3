"""GPU tests (-m gpu) of the TSDF volume on the frames and volumes where a kernel's indexing goes wrong and that
tests/test_gpu_tsdf_cases.py and tests/test_gpu_tsdf_extract.py leave out: k_tsdf_depth, k_tsdf_integrate, k_tsdf_count and k_tsdf_scatter
against the NumPy restatement of the rule (tests/tsdf_reference.py), every word of sum, weight, the counts, xyz, normals and edge, with
the camera taken from sl3d_get_align_camera.  tests/test_tsdf_layout_cases.py says on the CPU what each case is for; the cheap part of
that is repeated here under the device's camera before the device is called.

1. Windows whose pitch (W + 15) & ~15 is above W, several views: 67 x 19 (pitch 80), 300 x 20 (pitch 304: k_tsdf_depth takes 256
   columns a block, so two column blocks) and 530 x 6 (pitch 544: three).  The padding columns of every view hold perfect points under
   valid bytes.  One view, all views, views from slot 1 on with first_step 1, two calls that must equal one; the surface at min_weight
   1 and 2; the planes of a view afterwards bit for bit what was put.
2. A 2 x 2 window (one cell), and 1 x 7 and 9 x 1 (no cell: no sample, an empty surface).
3. The int32 bound of sum: 65,535 equal views of two voxels whose votes are +32767 and -32767 (13,107 asynchronous calls of five views,
   as many launches as test_the_view_limit makes), the crossing between them at weight 65,535, the refusal of one more view.
4. The turntable indices 65530 .. 65534 in one call: the last rows of the recurrence's table."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reference as TR
from dense_planes import dense_layout
from test_tsdf_layout_cases import fused, late_purpose, padded_layout_purpose, saturation_purpose, small_layout_purpose
from tsdf_gpu import UNSUPPORTED, check_planes, check_surface, context, put, reset, same_bits

pytestmark = pytest.mark.gpu


def _runs(sc, cam, points, valid, est, vol):
    """every way of calling over the views, planes and counts after each, the surface at two weights; returns the planes of all views"""
    V = len(points)

    def want(first_view, n_views, first_step):
        return fused(vol, points[first_view:first_view + n_views], valid[first_view:first_view + n_views], cam, est, first_step)
    for first_view, n_views, first_step in ((0, 1, 0), (0, V, 0), (1, V - 1, 1)):
        s, w, counts = want(first_view, n_views, first_step)
        reset(sc, vol)
        assert sc.tsdf_integrate(first_view, n_views, est, first_step) == counts, (first_view, n_views, first_step)
        check_planes(sc, vol, s, w)
    # two calls equal one call over the same views
    sV, wV, cV = want(0, V, 0)
    s1, w1, c1 = want(0, 1, 0)
    reset(sc, vol)
    assert sc.tsdf_integrate(0, 1, est, 0) == c1
    assert sc.tsdf_integrate(1, V - 1, est, 1) == [cV[0] - c1[0], cV[1]]
    check_planes(sc, vol, sV, wV)
    for mw in (1, 2):
        edge = check_surface(sc, sV, wV, vol, mw)[2]
        assert np.all(np.diff(edge) > 0)
    return sV, wV, cV


@pytest.mark.parametrize("name", list(TC.LAYOUTS))
def test_layouts(name):
    lay = TC.LAYOUTS[name]
    W, H = lay["frame"]
    with context(W, H, lay["V"], full=lay["full"]) as sc:
        cam = sc.align_camera()
        points, valid, est, pads, vol = TC.layout_case(cam, name)
        assert dense_layout(sc, 0)[4] == TC.pitch_of(W) > W
        if name in TC.PADDED:
            padded_layout_purpose(name, cam, points, valid, est, pads, vol)
        else:
            small_layout_purpose(name, cam, points, valid, est, vol)
        for v in range(lay["V"]):
            put(sc, v, points[v], valid[v], pads[v])
        s, w, counts = _runs(sc, cam, points, valid, est, vol)
        if min(W, H) == 1:
            xyz, nrm, edge, stats = sc.tsdf_extract(1, stats=True)
            assert stats == [int(np.prod(vol["dims"])), 0, 0] and len(xyz) == len(nrm) == len(edge) == 0 and counts == [0, 0]
        for v in range(lay["V"]):                                           # the calls wrote no plane
            xyz, val = sc.points(v)
            assert same_bits(xyz, points[v]) and np.array_equal(val, valid[v])


@pytest.fixture(scope="module")
def exact():
    with context(TC.EXACT["W"], TC.EXACT["H"], 5, cal=TC.exact_calibration()) as sc:
        cam = sc.align_camera()
        assert np.array_equal(cam, TC.camera(TC.exact_calibration()))
        yield sc, cam


def test_saturation(exact):
    sc, cam = exact
    xyz, valid, vol, s, w = saturation_purpose(cam)
    pad = np.zeros((TC.EXACT["H"], 3), np.float32)
    pad[:, 2] = 64.0
    for v in range(5):
        put(sc, v, xyz, valid, pad)
    reset(sc, vol)
    e = np.ascontiguousarray(TC.IDENTITY, np.float64)
    for _ in range(TC.SATURATION_VIEWS // 5):
        assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 5, 0, e.ctypes.data, None) == 0
    sc.synchronize()
    assert 5 * (TC.SATURATION_VIEWS // 5) == TC.SATURATION_VIEWS and list(s) == [TC.SATURATED, -TC.SATURATED]
    check_planes(sc, vol, s, w)
    pos = check_surface(sc, s, w, vol, TC.SATURATION_VIEWS)[0]
    assert len(pos) == 1
    assert check_surface(sc, s, w, vol, TC.SATURATION_VIEWS + 1)[3] == [2, 0, 0]
    # one more view is refused and changes nothing
    counts = (C.c_int64 * 2)(-7, -7)
    assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 1, 0, e.ctypes.data, counts) == UNSUPPORTED and list(counts) == [-7, -7]
    check_planes(sc, vol, s, w)
    reset(sc, vol)                                                          # a reset clears the planes and starts the count again
    check_planes(sc, vol, *TR.new_volume(vol))
    assert sc.tsdf_integrate(0, 1, TC.IDENTITY) == [2, 2]
    check_planes(sc, vol, np.array([32767, -32767], np.int32), np.ones(2, np.uint32))


def test_late_steps():
    W, H = TC.FRAME
    with context(W, H, TC.LATE["V"]) as sc:
        cam = sc.align_camera()
        points, valid, est, pads, vol = TC.late_case(cam)
        s, w, counts = late_purpose(cam, points, valid, est, vol)
        for v in range(TC.LATE["V"]):
            put(sc, v, points[v], valid[v], pads[v])
        reset(sc, vol)
        assert sc.tsdf_integrate(0, TC.LATE["V"], est, TC.LATE["first_step"]) == counts
        check_planes(sc, vol, s, w)
        check_surface(sc, s, w, vol, 1)
