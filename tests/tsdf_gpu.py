"""What the GPU tests of the TSDF volume share (tests/test_gpu_tsdf_cases.py, tests/test_gpu_tsdf_extract.py, tests/test_gpu_tsdf_layouts.py,
tests/test_gpu_tsdf_scene.py):
a context whose dense planes a test writes itself (tests/dense_planes.py), and the comparison of a fused volume and its surface with
the restatement (tests/tsdf_reference.py), word for word."""
import numpy as np

import tsdf_cases as TC
import tsdf_reference as TR
from conftest import pkg
from dense_planes import _copy_rows, dense_layout, put_dense

INVALID_ARG, STATE, UNSUPPORTED = -1, -4, -5


def context(W, H, V, cal=None, full=TC.FULL, origin=TC.ORIGIN, run=True):
    """a context of the shape behind one run over small synthetic views (every buffer exists, nothing is pending), then under the
    calibration `cal` if one is given"""
    S, syn = pkg("scanner"), pkg("synth")
    sc = S.Scanner(W, H, 2048, 2048, 10, 10, 2, 2, max_views=V, full_size=full, origin=origin)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(full[0], full[1], 2048, 2048)))
    if run:
        sc.set_masks(np.ones((full[1], full[0]), np.uint8))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
        sc.run(0, V)
        sc.synchronize()
    if cal is not None:
        sc.set_calibration(*cal)
    return sc


def put(sc, view, xyz, valid, pad=None):
    """the planes of a view; pad: (H, 3) float32, the point of every padding column of a row, under valid bytes of 1"""
    put_dense(sc, view, xyz, valid, pad_xyz=np.float32(0.0), pad_valid=0 if pad is None else 1)
    if pad is not None:
        p_addr, p_pitch, _, _, pitch = dense_layout(sc, view)
        if pitch > sc.W:
            rows = np.ascontiguousarray(np.repeat(pad[:, None, :], pitch - sc.W, axis=1))
            _copy_rows(p_addr, p_pitch, sc.H, 12 * sc.W, rows.view(np.uint8).reshape(sc.H, 12 * (pitch - sc.W)))


def same_bits(got, want):
    """bit for bit, NaNs included"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint32),
                                                                                 np.ascontiguousarray(want).view(np.uint32))


def reset(sc, vol):
    sc.tsdf_reset(vol["origin"], vol["voxel"], vol["trunc"], vol["dims"])


def check_planes(sc, vol, want_sum, want_weight):
    nx, ny, nz = vol["dims"]
    s, w = sc.tsdf_volume()
    assert s.dtype == np.int32 and w.dtype == np.uint32 and s.shape == w.shape == (nz, ny, nx)
    assert np.array_equal(s.ravel(), want_sum) and np.array_equal(w.ravel(), want_weight)


def check_surface(sc, want_sum, want_weight, vol, min_weight):
    """the device's extraction of its own volume against the restatement's of the same planes; returns the restatement's"""
    xyz, nrm, edge, stats = sc.tsdf_extract(min_weight, stats=True)
    rxyz, rnrm, redge, rstats = TR.extract(want_sum, want_weight, vol, min_weight)
    assert stats == rstats, (stats, rstats)
    assert edge.dtype == np.int32 and np.array_equal(edge, redge)
    assert same_bits(xyz, rxyz) and same_bits(nrm, rnrm)
    return rxyz, rnrm, redge, rstats
