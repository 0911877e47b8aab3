"""CPU tests of the inputs of tests/test_gpu_tsdf_layouts.py (tests/tsdf_cases.py: layout_case, saturation_case, late_case): what each
case is for, by the NumPy restatement of the rule alone (tests/tsdf_reference.py), and every case through the library's own arithmetic
on the CPU (tests/native/tsdf_check.cpp, plain and with -fsanitize=address,undefined, as in tests/test_tsdf_arith.py: a stand-alone
program, nothing is loaded into python; the program has no pitch).

1. Windows whose rows are padded (67 x 19, pitch 80) and wider than one and two blocks of the depth pre-pass (300 x 20, 530 x 6), three
   views each: every view is sampled past the block boundaries and at the last usable column, the weights disagree, the surface has
   crossings past the scatter pass's first block -- and a kernel that took the padding for pixels, W for the row stride or one view's
   planes for another's would leave another volume.
2. A 2 x 2 window (one cell) takes samples; 1 x 7 and 9 x 1 (no cell) take none, whatever the volume.
3. Two voxels whose votes are +32767 and -32767: 65,535 equal views bring sum to +-2,147,385,345, the largest magnitude the view limit
   lets an int32 reach, and the crossing between them is found at weight 65,535 and not at 65,536.
4. Five views at the turntable indices 65530 .. 65534 of a step of a 65,532nd of a turn: samples are taken, and other ones than at
   the indices 0 .. 4."""
import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reference as TR
from test_tsdf_arith import _check, checker  # noqa: F401  (the fixture: the native program, plain and sanitized)


def fused(vol, points, valid, cam, est, first_step=0):
    s, w = TR.new_volume(vol)
    counts = TR.integrate(s, w, vol, points, valid, cam, *TC.ORIGIN, est, first_step)
    return s, w, list(counts)


def padded_layout_purpose(name, cam, points, valid, est, pads, vol):
    """what a padded layout is for, by the restatement alone (tests/test_gpu_tsdf_layouts.py repeats it under the device's camera);
    returns the fused planes and counts of all views"""
    W, H = TC.LAYOUTS[name]["frame"]
    V = len(points)
    assert TC.pitch_of(W) > W and valid.shape == (V, H, W)
    s, w, counts = fused(vol, points, valid, cam, est)
    cols = TC.sample_columns(vol, points, valid, cam, est)
    for block in range(1, (W + 255) // 256):                                # every column block of the depth pre-pass, in every view
        assert all((c >= 256 * block).any() for c in cols), (name, block)
    assert max(int(c.max()) for c in cols) == W - 2                         # the last usable column
    assert (w == 0).any() and (w == V).any() and ((w > 0) & (w < V)).any()
    assert len({len(c) for c in cols}) == V and sum(len(c) for c in cols) == counts[0]          # the views' sample counts differ
    for mw in (1, 2):
        edge, stats = TR.extract(s, w, vol, mw)[2:]
        assert stats[2] >= 1 and edge.max() >= 3 * 1024
    # a wrong stride would show: the padding taken for pixels, W taken for the row stride, the planes of views 0 and 1 exchanged
    for other in (TC.padded_image(points, valid, pads), TC.misread_rows(points, valid, pads), (points[[1, 0, 2]], valid[[1, 0, 2]])):
        s2, w2, _ = fused(vol, *other, cam, est)
        assert not np.array_equal(s2, s) and not np.array_equal(w2, w), name
    return s, w, counts


def small_layout_purpose(name, cam, points, valid, est, vol):
    W, H = TC.LAYOUTS[name]["frame"]
    s, w, counts = fused(vol, points, valid, cam, est)
    if min(W, H) == 1:                                                      # no cell: fu + 1 < W or fv + 1 < H never holds
        assert counts == [0, 0] and not s.any() and not w.any()
        xyz, nrm, edge, stats = TR.extract(s, w, vol, 1)
        assert stats == [len(s), 0, 0] and len(xyz) == len(nrm) == len(edge) == 0
    else:
        assert counts[0] >= 1 and set(np.concatenate(TC.sample_columns(vol, points, valid, cam, est))) == {0}
    return s, w, counts


def saturation_purpose(cam):
    """returns xyz, valid, vol, and the planes 65,535 equal views leave"""
    xyz, valid, vol = TC.saturation_case()
    s, w, counts = fused(vol, xyz[None], valid[None], cam, TC.IDENTITY)
    assert list(s) == [32767, -32767] and list(w) == [1, 1] and counts == [2, 2]
    assert np.array_equal(TR.turns(TC.IDENTITY, 8), [[1.0, 0.0]] * 8)       # every view of every call votes the same: by multiplication
    n = TC.SATURATION_VIEWS
    big = s.astype(np.int64) * n
    assert list(big) == [2147385345, -2147385345] and TC.SATURATED == 2147385345 and np.abs(big).max() < 2**31
    s, w = big.astype(np.int32), np.full(2, n, np.uint32)
    pos, nrm, edge, stats = TR.extract(s, w, vol, n)
    X, _ = TR.centres(vol)
    assert stats == [2, 2, 1] and list(edge) == [0] and np.array_equal(pos[0], (0.5 * (X[0] + X[1])).astype(np.float32))
    assert TR.extract(s, w, vol, n + 1)[3] == [2, 0, 0]
    return xyz, valid, vol, s, w


def late_purpose(cam, points, valid, est, vol):
    s, w, counts = fused(vol, points, valid, cam, est, TC.LATE["first_step"])
    assert TC.LATE["first_step"] + TC.LATE["V"] == TR.MAX_STEPS and counts[0] > 0
    assert not np.array_equal(fused(vol, points, valid, cam, est, 0)[0], s)
    return s, w, counts


@pytest.fixture(scope="module")
def cams():
    return {full: TC.camera(TC.rig_calibration(full)) for full in (TC.FULL, TC.WIDE)}


@pytest.fixture(scope="module")
def exact_cam():
    return TC.camera(TC.exact_calibration())


@pytest.mark.parametrize("name", list(TC.LAYOUTS))
def test_layouts(cams, name):
    cam = cams[TC.LAYOUTS[name]["full"]]
    points, valid, est, pads, vol = TC.layout_case(cam, name)
    assert np.prod(vol["dims"]) <= 30000 and valid[0].size <= 6000
    if name in TC.PADDED:
        padded_layout_purpose(name, cam, points, valid, est, pads, vol)
    else:
        small_layout_purpose(name, cam, points, valid, est, vol)


def test_saturation(exact_cam):
    saturation_purpose(exact_cam)


def test_late_steps(cams):
    cam = cams[TC.FULL]
    points, valid, est, _, vol = TC.late_case(cam)
    late_purpose(cam, points, valid, est, vol)


# ---- the same cases through the library's arithmetic on the CPU ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.LAYOUTS))
def test_layouts_native(checker, tmp_path, cams, name):
    cam = cams[TC.LAYOUTS[name]["full"]]
    points, valid, est, _, vol = TC.layout_case(cam, name)
    V = len(points)
    for first, n, mw in ((0, 1, 1), (0, V, 1), (0, V, 2), (1, V - 1, 1)):
        _check(checker, tmp_path, cam, est, vol, points[first:first + n], valid[first:first + n], first, mw)


def test_saturation_native(checker, tmp_path, exact_cam):
    xyz, valid, vol = TC.saturation_case()
    _check(checker, tmp_path, exact_cam, TC.IDENTITY, vol, xyz[None], valid[None])


def test_late_steps_native(checker, tmp_path, cams):
    cam = cams[TC.FULL]
    points, valid, est, _, vol = TC.late_case(cam)
    _check(checker, tmp_path, cam, est, vol, points, valid, TC.LATE["first_step"])
