"""CPU tests of the inputs of tests/test_gpu_view_seams.py (tests/view_seams.py): what each input is for, by the NumPy restatements alone
(tests/align_reference.py, tests/align_plane_reference.py, tests/tsdf_reference.py).

A context stacks its views without a gap: for a kernel that walks a vertical neighbourhood of view v, row -1 is the last row of view
v - 1 and row H the first row of view v + 1.  A row clip that is off by one reads valid data there and nothing faults; these tests show
that with the inputs of view_seams every such reading changes the result, so that the word-for-word comparisons on the device can fail:

1. Both correspondence passes, four crafted views at 3 x 2 (H below the window), 9 x 5, 67 x 19 and 130 x 37, a window origin of (37, 5), under
   two cameras: for every pair that has the neighbour, either side and every window 0 .. 4 the words over the target extended by the
   neighbour's row differ from the clipped words -- at window 0 through the sources whose centre is row -1 or row H, which a clipped
   pass cannot match at any window.  The clipped words have 0 < n < sources; the point-to-plane form loses the sources it finds behind
   the seam to the missing normal (word 17 grows), since rows 0 and H - 1 of a normal plane never hold one.  (Where H < 3 no pixel has a
   normal: n is 0 by the rule, and 0 < word 17 < sources stands in for it.)
2. The normals of the smooth views: rows 0 and H - 1 of a middle view are NaN throughout, and the same view with its neighbours' rows
   has normals in both.
3. The TSDF volume at 20 x 6 and 67 x 19: integrating the frames extended below, and above, changes sum, weight and the sample count, over
   all views and over the views 1 .. V - 2 at first_step 1; the rows fv = -1 and fv = H - 1 have voxels."""
import numpy as np
import pytest

import align_plane_reference as PR
import align_reference as AR
import tsdf_cases as TC
import tsdf_reference as TR
import view_seams as VS
from test_align_arith import CAMERAS

ORIGIN = (37, 5)
SHAPES = [(3, 2), (9, 5), (67, 19), (130, 37)]                              # (W, H)
TSDF_SHAPES = [(20, 6), (67, 19)]
V = 4
WINDOWS = (0, 1, 2, 3, 4)
RANGE, MAX_DIST, EDGE = 64.0, 0.5, 1.0


def seed_of(W, H):
    """100 W + H as in the other pass tests; 9 x 5 has 21 interior pixels, and under most seeds some pair keeps no normal under an
    accepted pair at window 0: one of the seeds under which every pair of either camera does"""
    return 4 if (W, H) == (9, 5) else 100 * W + H


def quantisation_centre(est):
    return float(est[2]) - 0.25, float(est[3]) + 0.5


def align_purpose(cam, W, H, windows=WINDOWS):
    """what seam_views is for, by the restatements alone (tests/test_gpu_view_seams.py repeats a part under the device's camera);
    returns points, valid, pads, est and the number of comparisons made"""
    est = VS.pass_estimate(cam)
    points, valid, pads, marks = VS.seam_views(cam, W, H, *ORIGIN, V, seed_of(W, H), est)
    ox, oz = quantisation_centre(est)
    tail = (est, ox, oz, RANGE, MAX_DIST)
    nrm = np.stack([PR.normals(points[v], valid[v], EDGE) for v in range(V)])
    assert np.isnan(nrm[:, 0]).all() and np.isnan(nrm[:, H - 1]).all()
    made = 0
    for j in range(V - 1):
        assert len(marks[j]["below"]) >= 1 and (j == 0 or len(marks[j]["above"]) >= 1), (j, marks[j])
        for window in windows:
            clipped = AR.pair_words(points[j + 1], valid[j + 1], points[j], valid[j], cam, *ORIGIN, *tail, window)
            plane = PR.pair_words(points[j + 1], valid[j + 1], points[j], valid[j], nrm[j], cam, *ORIGIN, *tail, window)
            assert 0 < clipped[0] < clipped[11], (j, window, clipped)
            assert plane[16] == clipped[11]
            if H >= 3:
                assert 0 < plane[0] < plane[16] and plane[17] > 0, (j, window, plane)
            else:                                                            # no pixel has a normal: every near source is lost
                assert plane[0] == 0 and 0 < plane[17] < plane[16], (j, window, plane)
            for side in VS.SIDES[0 if j >= 1 else 1:]:
                tp, tv, shift = VS.extended_target(points, valid, j, side)
                wrong = AR.pair_words(points[j + 1], valid[j + 1], tp, tv, cam, ORIGIN[0], ORIGIN[1] + shift, *tail, window)
                assert wrong != clipped and wrong[0] >= clipped[0] + len(marks[j][side]), (j, side, window)
                wrong = PR.pair_words(points[j + 1], valid[j + 1], tp, tv, VS.extended_plane(nrm, j, side), cam, ORIGIN[0], ORIGIN[1] + shift,
                                      *tail, window)
                assert wrong != plane and wrong[17] >= plane[17] + len(marks[j][side]), (j, side, window)
                made += 2
    return points, valid, pads, est, made


def normals_purpose(cam, W, H):
    """what seam_surfaces is for the normals; returns points, valid, pads"""
    points, valid, _, pads = VS.seam_surfaces(cam, W, H, *ORIGIN, V)
    for v in (1, 2):
        n = PR.normals(points[v], valid[v], VS.NORMAL_EDGE)
        assert np.isnan(n[0]).all() and np.isnan(n[H - 1]).all()
        if H >= 3:
            assert not np.isnan(n[1:H - 1, 1:W - 1]).any()                  # (smooth and within the edge: every interior pixel has one)
        wide = PR.normals(*VS.extended_both(points, valid, v), VS.NORMAL_EDGE)
        assert not np.isnan(wide[1, 1:W - 1]).any() and not np.isnan(wide[H, 1:W - 1]).any()       # the view's rows 0 and H - 1
    return points, valid, pads


def fused(vol, points, valid, cam, est, first_step=0, shift=0):
    s, w = TR.new_volume(vol)
    counts = TR.integrate(s, w, vol, points, valid, cam, ORIGIN[0], ORIGIN[1] + shift, est, first_step)
    return s, w, list(counts)


def seam_rows(vol, cam, est, H, view):
    """the window rows fv of the voxels of `vol` in the frame of the view with turntable index `view`"""
    X, _ = TR.centres(vol)
    v = TR.project(TR.step(X, TR.turns(est, view + 1)[view], est[2], est[3]), cam)[1]
    return np.floor(v) - ORIGIN[1]


def tsdf_purpose(cam, W, H, spans=((0, V, 0), (1, V - 2, 1))):
    """what seam_surfaces and seam_volume are for the TSDF volume; returns points, valid, pads, est, vol"""
    points, valid, est, pads = VS.seam_surfaces(cam, W, H, *ORIGIN, V)
    est = est + VS.EST_OFFSET
    vol = VS.seam_volume(points)
    assert np.prod(vol["dims"]) <= 200000
    for view in range(V):
        rows = seam_rows(vol, cam, est, H, view)
        assert (rows == -1).any() and (rows == H - 1).any() and (rows <= -2).any() and (rows >= H).any()
    for first, n, first_step in spans:
        s, w, counts = fused(vol, points[first:first + n], valid[first:first + n], cam, est, first_step)
        assert counts[0] > 0 and (w == n).any() and (w == 0).any()
        for side in VS.SIDES:
            xp, xv, shift = VS.extended_views(points, valid, side)
            s2, w2, c2 = fused(vol, xp[first:first + n], xv[first:first + n], cam, est, first_step, shift)
            assert c2[0] > counts[0] and not np.array_equal(w2, w) and not np.array_equal(s2, s), (first, n, side)
    return points, valid, pads, est, vol


@pytest.fixture(scope="module", params=["distorted", "rig"])
def cam(request):
    return CAMERAS["distorted"] if request.param == "distorted" else TC.camera(TC.rig_calibration())


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_align_seams(cam, W, H):
    made = align_purpose(cam, W, H)[4]
    assert made == 2 * len(WINDOWS) * (1 + 2 * (V - 2))                     # pair 0 has one side, the others two; both forms


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_normal_seams(cam, W, H):
    normals_purpose(cam, W, H)


@pytest.mark.parametrize("W,H", TSDF_SHAPES, ids=[f"{w}x{h}" for w, h in TSDF_SHAPES])
def test_tsdf_seams(cam, W, H):
    tsdf_purpose(cam, W, H)


def test_the_halves_and_the_extensions():
    """the builders' own bookkeeping: disjoint halves, and an extended view is the stacked memory"""
    for W in (2, 3, 9, 67, 130):
        lo, hi = VS.halves(W)
        assert len(lo) and len(hi) and not set(lo) & set(hi) and sorted([*lo, *hi]) == list(range(W))
    c = CAMERAS["distorted"]
    points, valid, pads, marks = VS.seam_views(c, 9, 5, *ORIGIN, V, 1, VS.pass_estimate(c))
    flat = points.reshape(V * 5, 9, 3)                                       # the views as a context stacks them (no padding here)
    for j in (1, 2):
        tp, tv, shift = VS.extended_target(points, valid, j, "above")
        assert shift == -1 and np.array_equal(tp.view(np.uint32), flat[5 * j - 1:5 * j + 5].view(np.uint32))
        tp, tv, shift = VS.extended_target(points, valid, j, "below")
        assert shift == 0 and np.array_equal(tp.view(np.uint32), flat[5 * j:5 * j + 6].view(np.uint32))
    assert all(len(p) == 5 and p.dtype == np.float32 for p in pads) and len(pads) == V
