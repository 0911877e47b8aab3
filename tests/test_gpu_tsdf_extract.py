"""GPU tests (-m gpu) of the extraction of a TSDF volume's zero level: sl3d_tsdf_extract / k_tsdf_count, k_compact_scan,
k_tsdf_scatter against the NumPy restatement of the rule (tests/tsdf_reference.py): xyz, normals, edge and the three counts, bit for bit.
The planes of a volume are set by integrating crafted views; the restatement extracts from the planes the device hands back, which the
tests hold to the restatement's own as well.

1. The shapes of tests/test_gpu_tsdf_cases.py -- (5, 3, 2), (64, 1, 1), (65, 3, 2), (33, 9, 7), (70, 33, 5): k_tsdf_count and k_tsdf_scatter
   take 1024 voxels a block, 4 a lane -- over five crafted turntable views, at min_weight 1 and 2; for the two larger ones crossings
   past the first block of the scatter pass.
2. Volumes crafted voxel by voxel through an exact camera (tests/tsdf_cases.slab_case / column_case): a crossing on each axis, crossings
   whose neighbours lie outside the volume (one-sided gradients), a zero gradient (NaN normal), f0 == 0 and f1 == 0 exactly, unknown
   voxels between known ones, and empty results (tests/test_tsdf_arith.py says by the restatement alone what each is for).
3. The protocol: device pointers, a capacity below m, a surface that survives an integration and not a reset."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reference as TR
from test_tsdf_arith import _extraction_cases
from tsdf_gpu import STATE, check_planes, check_surface, context, put, reset, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def views():
    W, H = TC.FRAME
    with context(W, H, 5) as sc:
        cam = sc.align_camera()
        points, valid, est, pads, _ = TC.shape_case(cam, (1, 1, 1), 5, 11)
        for v in range(5):
            put(sc, v, points[v], valid[v], pads[v])
        yield sc, cam, points, valid, est + np.array([0.0, 0.0, 0.05, -0.03])


@pytest.mark.parametrize("dims", TC.SHAPES, ids=["x".join(map(str, d)) for d in TC.SHAPES])
def test_shapes(views, dims):
    sc, cam, points, valid, est = views
    vol = TC.shape_case(cam, dims, 1, 11)[4]
    s, w = TR.new_volume(vol)
    counts = TR.integrate(s, w, vol, points, valid, cam, *TC.ORIGIN, est)
    reset(sc, vol)
    assert sc.tsdf_integrate(0, 5, est) == list(counts)
    check_planes(sc, vol, s, w)
    for mw in (1, 2):
        xyz, nrm, edge, stats = check_surface(sc, s, w, vol, mw)
        assert np.all(np.diff(edge) > 0)                                    # ascending (v0, axis)
        if np.prod(dims) >= 900:                                            # by the restatement alone
            assert stats[2] > 0 and 0 < stats[1] < stats[0] and edge.max() >= 3 * 1024 and {int(a) for a in edge % 3} == {0, 1, 2}
            assert np.isfinite(nrm).all(axis=1).any()
    # a volume of which nothing is known: an empty result
    xyz, nrm, edge, stats = check_surface(sc, s, w, vol, 6)
    assert stats == [int(np.prod(dims)), 0, 0] and len(xyz) == len(nrm) == len(edge) == 0


@pytest.fixture(scope="module")
def exact():
    with context(TC.EXACT["W"], TC.EXACT["H"], 2, cal=TC.exact_calibration()) as sc:
        yield sc, sc.align_camera()


@pytest.mark.parametrize("case", range(len(_extraction_cases())), ids=[c[0] for c in _extraction_cases()])
def test_crafted_volumes(exact, case):
    sc, cam = exact
    name, (xyz, valid, vol), mw = _extraction_cases()[case]
    put(sc, 0, xyz, valid)
    s, w = TR.new_volume(vol)
    counts = TR.integrate(s, w, vol, xyz[None], valid[None], cam, *TC.ORIGIN, TC.IDENTITY)
    reset(sc, vol)
    assert sc.tsdf_integrate(0, 1, TC.IDENTITY) == list(counts)
    check_planes(sc, vol, s, w)
    check_surface(sc, s, w, vol, mw)
    check_surface(sc, s, w, vol, 3 - mw)                                    # ... and at the other min_weight


def test_protocol(views):
    sc, cam, points, valid, est = views
    vol = TC.shape_case(cam, (33, 9, 7), 1, 11)[4]
    s, w = TR.new_volume(vol)
    TR.integrate(s, w, vol, points[:3], valid[:3], cam, *TC.ORIGIN, est)
    reset(sc, vol)
    sc.tsdf_integrate(0, 3, est)
    rxyz, rnrm, redge, rstats = TR.extract(s, w, vol, 1)
    m = rstats[2]
    assert m > 8
    out, stats = sc.tsdf_extract_device(1)
    assert stats == rstats and out.xyz and out.normals and out.edge and len({out.xyz, out.normals, out.edge}) == 3
    # a capacity below m: the first rows only, *n is still m
    n = C.c_int64(-7)
    xyz, nrm, edge = np.full((m, 3), -7, np.float32), np.full((m, 3), -7, np.float32), np.full(m, -7, np.int32)
    assert sc.L.sl3d_get_tsdf_surface(sc._h, xyz.ctypes.data, nrm.ctypes.data, edge.ctypes.data, 5, C.byref(n)) == 0 and n.value == m
    assert same_bits(xyz[:5], rxyz[:5]) and same_bits(nrm[:5], rnrm[:5]) and np.array_equal(edge[:5], redge[:5])
    assert (xyz[5:] == -7).all() and (nrm[5:] == -7).all() and (edge[5:] == -7).all()
    # any output may be left out
    assert sc.L.sl3d_get_tsdf_surface(sc._h, None, None, edge.ctypes.data, m, C.byref(n)) == 0 and np.array_equal(edge, redge)
    assert sc.L.sl3d_get_tsdf_surface(sc._h, None, None, None, -1, C.byref(n)) == -1
    # the asynchronous form of the counts: none asked for, the surface is the same
    assert sc.L.sl3d_tsdf_extract(sc._h, 1, None, None) == 0
    got = sc._fill("sl3d_get_tsdf_surface", (), (np.float32, 3), (np.float32, 3), (np.int32,))
    assert same_bits(got[0], rxyz) and same_bits(got[1], rnrm) and np.array_equal(got[2], redge)
    # an integration leaves the last surface alone; the next extraction sees the new planes
    TR.integrate(s, w, vol, points[3:5], valid[3:5], cam, *TC.ORIGIN, est, 3)
    sc.tsdf_integrate(3, 2, est, 3)
    got = sc._fill("sl3d_get_tsdf_surface", (), (np.float32, 3), (np.float32, 3), (np.int32,))
    assert same_bits(got[0], rxyz) and np.array_equal(got[2], redge)
    check_planes(sc, vol, s, w)
    check_surface(sc, s, w, vol, 2)
    # a reset discards the surface
    reset(sc, vol)
    assert sc.L.sl3d_get_tsdf_surface(sc._h, None, None, None, 0, C.byref(n)) == STATE
    xyz, nrm, edge, stats = sc.tsdf_extract(1, stats=True)
    assert stats == [33 * 9 * 7, 0, 0] and len(edge) == 0
