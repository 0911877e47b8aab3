"""GPU tests (-m gpu) of the dense normals and of one point-to-plane pass of the turntable refinement: sl3d_align_normals /
k_align_normals and sl3d_align_plane_sums / k_align_plane_pass<WINDOW> against the NumPy restatement of the rule
(tests/align_plane_reference.py) -- every normal plane bit for bit, every pass word for word -- with the camera taken from
sl3d_get_align_camera.

The inputs go into a context's dense planes through tests/dense_planes.put_dense behind sc.run(); sc.synchronize().  Every context is a
window with col0, row0 != 0 inside a larger full frame.  The tile of both kernels is 64 x 32, a wave a row of 64.

1. Shapes 1 x 1, 3 x 2 (no interior pixel: every normal NaN, n == 0, word 17 the sources with a candidate within max_dist), 9 x 9, 67 x 19,
   130 x 37, 257 x 9 (across the 64-column tile edge and, at 130 x 37, the 32-row one), each at windows 0, 1, 2, 4: three crafted turntable
   views (align_reference.crafted_views) whose two pairs differ, as three views, as two, and as the two from view 1 on.  normal_edge is
   1 mm -- three pixel spacings of the builder's surface, a third of its outliers' reach -- and for every shape from 9 x 9 up the
   restatement alone first shows that each pair of views accepts pairs, loses sources to missing normals and rejects others.  The padding
   columns of every target are poisoned with valid bytes over the spot a source of the last interior column lands on: a stencil or a window
   clipped to the pitch would use them, and the restatement alone shows that both change the result.
2. Crafted planes (align_plane_reference.special_planes) at windows 0, 1, 2, 4 and two ranges, all sources at once and each alone: a
   neighbour with valid == 0, one with a NaN under a valid byte, one exactly at normal_edge (kept) and one ulp beyond (dropped), collinear
   and coincident neighbours, the frame's borders and a corner, a best candidate without a normal beside a farther one with (lost, not
   re-matched), a feature exactly at the range limit and just below; empty views.
3. The calls' protocol: normals alone and their download, SL3D_E_STATE before they exist, the asynchronous form, every refusal -- and that a
   refused call changes nothing: the words of the next good call are those of a fresh context."""
import ctypes as C

import numpy as np
import pytest

import align_plane_reference as PR
import align_reference as AR
from conftest import pkg
from dense_planes import _copy_rows, dense_layout, put_dense

pytestmark = pytest.mark.gpu

FULL, ORIGIN = (320, 240), (37, 5)
SHAPES = [(1, 1), (3, 2), (9, 9), (67, 19), (130, 37), (257, 9)]       # (W, H)
WINDOWS = (0, 1, 2, 3, 4)
RANGE, MAX_DIST, EDGE = 64.0, 0.5, 1.0
INVALID_ARG, STATE = -1, -4


def _context(W, H, V, run=True):
    """a context of the shape behind one run over small synthetic views: every buffer exists, nothing is pending"""
    S, syn = pkg("scanner"), pkg("synth")
    sc = S.Scanner(W, H, 2048, 2048, 10, 10, 2, 2, max_views=V, full_size=FULL, origin=ORIGIN)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(FULL[0], FULL[1], 2048, 2048)))
    if run:
        sc.set_masks(np.ones((FULL[1], FULL[0]), np.uint8))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
        sc.run(0, V)
        sc.synchronize()
    return sc


def _put(sc, view, xyz, valid, pad=None):
    """the planes of a view; pad: (H, 3) float32, the point of every padding column of a row, under valid bytes of 1"""
    put_dense(sc, view, xyz, valid, pad_xyz=np.float32(0.0), pad_valid=0 if pad is None else 1)
    if pad is not None:
        p_addr, p_pitch, _, _, pitch = dense_layout(sc, view)
        if pitch > sc.W:
            rows = np.ascontiguousarray(np.repeat(pad[:, None, :], pitch - sc.W, axis=1))
            _copy_rows(p_addr, p_pitch, sc.H, 12 * sc.W, rows.view(np.uint8).reshape(sc.H, 12 * (pitch - sc.W)))


def _same_plane(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])


def _near(points, valid, cam, est, window):
    """by the restatement alone: per pair the sources with a best candidate within max_dist"""
    out = []
    for j in range(len(points) - 1):
        p = points[j + 1].reshape(-1, 3)
        p = p[(valid[j + 1].reshape(-1) == 1) & np.isfinite(p).all(axis=1)]
        best = PR.best_candidates(p, AR.step(p, est), points[j], valid[j], cam, *ORIGIN, window)[0]
        out.append(int((best <= np.float64(np.float32(MAX_DIST)) ** 2).sum()))
    return out


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes_and_windows(W, H):
    with _context(W, H, 3) as sc:
        cam = sc.align_camera()
        points, valid, est, pads = AR.crafted_views(cam, W, H, ORIGIN[0], ORIGIN[1], 3, 100 * W + H)
        if W >= 3:                                                           # the poison of a target's padding: the very spot the source of the
            for v in range(2):                                               # row's last INTERIOR column lands on, nearer than any real candidate
                pads[v] = AR.turn(points[v + 1][:, W - 2].astype(np.float64), est).astype(np.float32)
        for v in range(3):
            _put(sc, v, points[v], valid[v], pads[v])
        assert dense_layout(sc, 0)[4] > W                                   # there are padding columns to poison
        est = est + np.array([0.0, 0.0, 0.05, -0.03])                       # (not the estimate that made the views)
        ox, oz = float(est[2]) - 0.25, float(est[3]) + 0.5
        args = (cam, ORIGIN[0], ORIGIN[1], est, ox, oz, RANGE, MAX_DIST, EDGE)
        nrm = [PR.normals(points[v], valid[v], EDGE) for v in range(3)]
        sc.align_normals(0, 3, EDGE)
        for v in range(3):
            assert _same_plane(sc.align_normal_plane(v), nrm[v]), v
        if W * H < 81:
            assert all(np.isnan(n).all() for n in nrm)                      # no interior pixel: no normal at all
        else:
            assert all(0 < (~np.isnan(n[..., 0])).sum() < (W - 2) * (H - 2) for n in nrm[1:])     # noise and invalid pixels take some
            # ... and a stencil that read the padding would have given the last column normals
            wide = PR.normals(np.concatenate([points[1], pads[1][:, None, :]], axis=1), np.concatenate([valid[1], np.ones((H, 1), np.uint8)], axis=1), 1e3)
            assert (~np.isnan(wide[:, W - 1, 0])).any() and np.isnan(nrm[1][:, W - 1]).all()
        for window in WINDOWS:
            want = PR.pass_sums(points, valid, *args, window)
            if W * H >= 81:                                                  # by the restatement alone, first: the case can fail
                assert (want[:, 0] > 0).all() and (want[:, 17] > 0).all() and (want[:, 0] + want[:, 17] < want[:, 16]).all()
                assert not np.array_equal(want[0], want[1])                 # the two pairs differ: a wrong pair stride shows
            else:
                assert (want[:, 0] == 0).all() and not want[:, 1:16].any() and list(want[:, 17]) == _near(points, valid, cam, est, window)
                assert (want[:, 17] > 0).all()
            got = sc.align_plane_sums(0, 3, est, ox, oz, RANGE, MAX_DIST, EDGE, window)
            assert got.dtype == np.int64 and got.shape == (2, 18) and np.array_equal(got, want), window
            assert np.array_equal(sc.align_plane_sums(0, 2, est, ox, oz, RANGE, MAX_DIST, EDGE, window), want[:1]), window
            assert np.array_equal(sc.align_plane_sums(1, 2, est, ox, oz, RANGE, MAX_DIST, EDGE, window), want[1:]), window
            if window >= 2 and W * H >= 81:
                # a pass that clipped the window to the pitch would have taken the poisoned column, two pixels from the source's centre,
                # and lost the pair (no normal is ever written there)
                tp = np.concatenate([points[0], pads[0][:, None, :]], axis=1)
                tv = np.concatenate([valid[0], np.ones((H, 1), np.uint8)], axis=1)
                tn = np.concatenate([nrm[0], np.full((H, 1, 3), np.nan, np.float32)], axis=1)
                wrong = PR.pair_words(points[1], valid[1], tp, tv, tn, *args[:8], window)
                assert wrong != list(want[0]), window
        got_xyz, got_valid = sc.points(1)                                    # the calls wrote no plane of a view
        assert np.array_equal(got_valid, valid[1]) and np.array_equal(got_xyz.view(np.uint32), points[1].view(np.uint32))
        assert _same_plane(sc.align_normal_plane(1), nrm[1])                 # the pass's own normals are the same normals


@pytest.fixture(scope="module")
def special():
    W, H = PR.SPECIAL["W"], PR.SPECIAL["H"]
    with _context(W, H, 2) as sc:
        cam = sc.align_camera()
        points, valid, names, at = PR.special_planes(cam, *ORIGIN)
        yield sc, cam, points, valid, names, at


def _centre(points, names, rng):
    i = names.index("feature exactly at the range limit")
    return float(points[1].reshape(-1, 3)[i][0]) - 4.0 * rng, float(points[0][12, 20][2])


NO_NORMAL = ["a neighbour invalid", "a neighbour NaN under a valid byte", "a neighbour one ulp beyond normal_edge",
             "a lower neighbour one ulp beyond normal_edge", "collinear neighbours", "coincident neighbours", "top border", "bottom border",
             "left border", "right border", "corner", "best without a normal, a farther one with"]


@pytest.mark.parametrize("rng", [64.0, 2.0])
def test_special_cases(special, rng):
    sc, cam, points, valid, names, at = special
    est, md, edge = np.array(PR.SPECIAL["est"]), PR.SPECIAL["max_dist"], PR.SPECIAL["normal_edge"]
    ox, oz = _centre(points, names, rng)
    for v in range(2):
        _put(sc, v, points[v], valid[v])
    nrm = PR.normals(points[0], valid[0], edge)
    sc.align_normals(0, 1, edge)
    assert _same_plane(sc.align_normal_plane(0), nrm)
    # what the cases are for, by the restatement alone: each cell of the normal plane
    for name, (r, c) in at.items():
        assert np.isnan(nrm[r, c]).all() == (name in NO_NORMAL), name
    assert np.array_equal(nrm[at["a flat plus: the normal (0, 0, 1)"]], np.float32([0, 0, 1]))
    assert not np.isnan(nrm[9, 17]).any()                                   # the farther candidate of the lost source has a normal
    assert int((~np.isnan(nrm[..., 0])).sum()) == len(names) - len(NO_NORMAL) + 1
    want = {w: PR.pass_sums(points, valid, cam, *ORIGIN, est, ox, oz, rng, md, edge, w) for w in WINDOWS}
    for w in WINDOWS:
        assert np.array_equal(sc.align_plane_sums(0, 2, est, ox, oz, rng, md, edge, w), want[w]), w
        assert int(want[w][0, 16]) == len(names) and int(want[w][0, 17]) == len(NO_NORMAL) and int(want[w][0, 0]) == len(names) - len(NO_NORMAL) - 1
    # every case alone, as the only source: the library gives the restatement's words
    for i, name in enumerate(names):
        only = valid.copy()
        only[1] = 0
        only[1].reshape(-1)[i] = 1
        _put(sc, 1, points[1], only[1])
        for w in (0, 1, 2):
            ref = PR.pass_sums(points, only, cam, *ORIGIN, est, ox, oz, rng, md, edge, w)
            assert np.array_equal(sc.align_plane_sums(0, 2, est, ox, oz, rng, md, edge, w), ref), (name, w)
            lost = int(name in NO_NORMAL)
            accepted = int(not lost and name != "feature exactly at the range limit")
            assert (int(ref[0, 0]), int(ref[0, 16]), int(ref[0, 17])) == (accepted, 1, lost), (name, w)
        if name == "best without a normal, a farther one with":             # the farther candidate was in reach: the pair is lost all the same
            p = points[1].reshape(-1, 3)[i:i + 1]
            assert AR.dist2(points[0][9, 17][None], p.astype(np.float64))[0] <= md * md


def test_empty_views(special):
    sc, cam, points, valid, names, at = special
    est, md, edge = np.array(PR.SPECIAL["est"]), PR.SPECIAL["max_dist"], PR.SPECIAL["normal_edge"]
    ox, oz = _centre(points, names, 64.0)
    none = np.zeros_like(valid[0])
    for tv, sv in ((valid[0], none), (none, valid[1]), (none, none)):
        _put(sc, 0, points[0], tv)
        _put(sc, 1, points[1], sv)
        want = PR.pass_sums(points, np.stack([tv, sv]), cam, *ORIGIN, est, ox, oz, 64.0, md, edge, 2)
        assert np.array_equal(sc.align_plane_sums(0, 2, est, ox, oz, 64.0, md, edge, 2), want)
        assert not want[0, :16].any() and int(want[0, 17]) == 0
        if not tv.any():
            assert np.isnan(sc.align_normal_plane(0)).all()


def test_state_and_refusals():
    S = pkg("scanner")
    est = np.array([1.0, 0.0, 0.0, 0.0])
    sums = np.full((2, 18), -7, np.int64)
    call = lambda sc, **kw: sc.L.sl3d_align_plane_sums(sc._h, kw.get("first", 0), kw.get("n", 3), kw.get("est", est).ctypes.data, kw.get("ox", 0.0),
                                                       kw.get("oz", 0.0), kw.get("rng", 64.0), kw.get("md", 0.5), kw.get("edge", 1.0), kw.get("window", 2),
                                                       sums.ctypes.data)
    with S.Scanner(9, 9, 2048, 2048, 10, 10, 2, 2, max_views=3, full_size=FULL, origin=ORIGIN) as fresh:
        assert call(fresh) == STATE and (sums == -7).all()                  # no calibration yet
    with _context(9, 9, 3, run=False) as sc:
        assert call(sc) == STATE and (sums == -7).all()                     # a calibration, but no dense result yet
        assert sc.L.sl3d_align_normals(sc._h, 0, 1, 1.0) == STATE
    nan, inf = float("nan"), float("inf")
    bad = [dict(n=1), dict(n=0), dict(n=4), dict(first=-1), dict(first=2, n=2), dict(rng=0.0), dict(rng=-1.0), dict(rng=nan), dict(rng=inf),
           dict(md=0.0), dict(md=-0.5), dict(md=nan), dict(md=inf), dict(md=65.0), dict(edge=0.0), dict(edge=-1.0), dict(edge=nan), dict(edge=inf),
           dict(window=-1), dict(window=5), dict(est=np.array([nan, 0.0, 0.0, 0.0])), dict(est=np.array([1.0, 0.0, inf, 0.0])), dict(ox=nan),
           dict(oz=-inf)]
    with _context(9, 9, 3) as sc:
        cam = sc.align_camera()
        points, valid, e, pads = AR.crafted_views(cam, 9, 9, *ORIGIN, 3, 5)
        for v in range(3):
            _put(sc, v, points[v], valid[v])
        nrm = np.empty((9, 9, 3), np.float32)
        assert sc.L.sl3d_get_align_normals(sc._h, 0, nrm.ctypes.data, nrm.strides[0]) == STATE      # never computed
        # every refusal on a context that has allocated nothing for the calls yet ...
        for kw in bad:
            assert call(sc, **kw) == INVALID_ARG and (sums == -7).all(), kw
        assert sc.L.sl3d_align_plane_sums(sc._h, 0, 3, None, 0.0, 0.0, 64.0, 0.5, 1.0, 2, sums.ctypes.data) == INVALID_ARG
        for a in ((0, 0, 1.0), (0, 4, 1.0), (-1, 1, 1.0), (3, 1, 1.0), (0, 1, 0.0), (0, 1, nan), (0, 1, inf), (0, 1, -2.0)):
            assert sc.L.sl3d_align_normals(sc._h, *a) == INVALID_ARG, a
        assert sc.L.sl3d_get_align_normals(sc._h, 0, nrm.ctypes.data, nrm.strides[0]) == STATE      # ... which changed nothing
        # ... then the first good call gives the words of a fresh context: the restatement's
        want = PR.pass_sums(points, valid, cam, *ORIGIN, e, e[2], e[3], RANGE, MAX_DIST, EDGE, 2)
        assert (want[:, 0] > 0).all()
        assert np.array_equal(sc.align_plane_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, EDGE, 2), want)
        # the pass computed the normals of its targets, views 0 and 1, not of view 2
        assert _same_plane(sc.align_normal_plane(1), PR.normals(points[1], valid[1], EDGE))
        assert sc.L.sl3d_get_align_normals(sc._h, 2, nrm.ctypes.data, nrm.strides[0]) == STATE
        for view, stride in ((-1, nrm.strides[0]), (3, nrm.strides[0]), (0, 12 * 9 - 4), (0, 12 * 9 + 2)):
            assert sc.L.sl3d_get_align_normals(sc._h, view, nrm.ctypes.data, stride) == INVALID_ARG
        assert sc.L.sl3d_get_align_normals(sc._h, 0, None, nrm.strides[0]) == INVALID_ARG
        # refusals between good calls change nothing either
        for kw in bad:
            assert call(sc, **kw) == INVALID_ARG and (sums == -7).all(), kw
        assert np.array_equal(sc.align_plane_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, EDGE, 2), want)
        # the asynchronous form: no words, the call returns at once; the next synchronising pass is unaffected
        assert sc.L.sl3d_align_plane_sums(sc._h, 0, 3, e.ctypes.data, float(e[2]), float(e[3]), RANGE, MAX_DIST, EDGE, 2, None) == 0
        sc.synchronize()
        assert np.array_equal(sc.align_plane_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, EDGE, 2), want)
        # another normal_edge is another plane: the pass always recomputes
        wide = PR.pass_sums(points, valid, cam, *ORIGIN, e, e[2], e[3], RANGE, MAX_DIST, 8.0, 2)
        assert not np.array_equal(wide, want)
        assert np.array_equal(sc.align_plane_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, 8.0, 2), wide)
        # normals of a view outside the span so far: the span widens, the plane of view 2 appears
        sc.align_normals(2, 1, EDGE)
        assert _same_plane(sc.align_normal_plane(2), PR.normals(points[2], valid[2], EDGE))
        assert np.array_equal(sc.align_plane_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, EDGE, 2), want)
