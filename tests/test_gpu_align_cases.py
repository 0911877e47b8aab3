"""GPU tests (-m gpu) of one correspondence pass of the turntable refinement: sl3d_align_sums / k_align_pass<WINDOW> against the
NumPy restatement of the rule (tests/align_reference.py), word for word, with the camera taken from sl3d_get_align_camera.

The inputs go into a context's dense planes through tests/dense_planes.put_dense behind sc.run(); sc.synchronize().  Every context is a
window with col0, row0 != 0 inside a larger full frame.  The tile of k_align_pass is 64 x 32, a wave a row of 64.

1. Shapes 1 x 1, 3 x 2, 9 x 9, 67 x 19 (past one wave, ragged rows), 130 x 37 (several blocks in both directions), 257 x 9, each at windows 0, 1, 2,
   4: three crafted turntable views (align_reference.crafted_views) whose two pairs differ in content -- a wrong pair stride shows -- as
   two views, as three, and as the two views from view 1 on.  The padding columns of every target are poisoned: valid = 1 over the very
   spot the row's last source lands on, closer than any real candidate -- a kernel that clips the window to the pitch takes it, and the
   restatement alone shows that this changes the words.  For the larger shapes the restatement alone shows that word 0 is neither 0 nor
   word 11: the case cannot pass on an identity.
2. Crafted planes (align_reference.special_planes), at windows 0, 1, 2, 4 and two ranges: a projected centre outside the frame on each side
   with the window reaching back in, candidates at equal d2, a nearer candidate later in row-major order, NaN, +-inf and +-3e38 under valid
   bytes on both sides, finite points under invalid bytes, points behind the camera, d2 exactly at max_dist^2 and just above,
   out-of-range coordinates of the source and of the target; an empty source view and an empty target view.
3. The call's protocol: the asynchronous form, the camera's 26 doubles against the calibration, the state a pass needs, every refusal."""
import ctypes as C

import numpy as np
import pytest

import align_reference as AR
from conftest import pkg
from dense_planes import _copy_rows, dense_layout, put_dense

pytestmark = pytest.mark.gpu

FULL, ORIGIN = (320, 240), (37, 5)
SHAPES = [(1, 1), (3, 2), (9, 9), (67, 19), (130, 37), (257, 9)]       # (W, H)
WINDOWS = (0, 1, 2, 3, 4)
RANGE, MAX_DIST = 64.0, 0.5
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


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes_and_windows(W, H):
    with _context(W, H, 3) as sc:
        cam = sc.align_camera()
        points, valid, est, pads = AR.crafted_views(cam, W, H, ORIGIN[0], ORIGIN[1], 3, 100 * W + H)
        for v in range(3):
            _put(sc, v, points[v], valid[v], pads[v])
        assert dense_layout(sc, 0)[4] > W                                   # there are padding columns to poison
        got_xyz, got_valid = sc.points(1)
        assert np.array_equal(got_valid, valid[1]) and np.array_equal(got_xyz.view(np.uint32), points[1].view(np.uint32))
        est = est + np.array([0.0, 0.0, 0.05, -0.03])                       # (not the estimate that made the views)
        ox, oz = float(est[2]) - 0.25, float(est[3]) + 0.5
        args = (cam, ORIGIN[0], ORIGIN[1], est, ox, oz, RANGE, MAX_DIST)
        for window in WINDOWS:
            want = AR.pass_sums(points, valid, *args, window)
            got = sc.align_sums(0, 3, est, ox, oz, RANGE, MAX_DIST, window)
            assert got.dtype == np.int64 and got.shape == (2, 12) and np.array_equal(got, want), window
            assert np.array_equal(sc.align_sums(0, 2, est, ox, oz, RANGE, MAX_DIST, window), want[:1]), window
            assert np.array_equal(sc.align_sums(1, 2, est, ox, oz, RANGE, MAX_DIST, window), want[1:]), window
            assert not np.array_equal(want[0], want[1])                     # the two pairs differ: a wrong pair stride shows
            if W * H >= 81:                                                  # by the restatement alone: no identity passes
                assert (want[:, 0] > 0).all() and (want[:, 0] < want[:, 11]).all() and (want[:, 11] < W * H).any()
            if window >= 1 and W * H >= 6:
                # ... and a pass that clipped the window to the pitch would have taken the poisoned column
                tp = np.concatenate([points[0], pads[0][:, None, :]], axis=1)
                tv = np.concatenate([valid[0], np.ones((H, 1), np.uint8)], axis=1)
                wrong = AR.pair_words(points[1], valid[1], tp, tv, *args, window)
                assert wrong != list(want[0]), window
        assert np.array_equal(sc.points(1)[0].view(np.uint32), points[1].view(np.uint32))      # the passes wrote no plane


@pytest.fixture(scope="module")
def special():
    W, H = AR.SPECIAL["W"], AR.SPECIAL["H"]
    with _context(W, H, 2) as sc:
        cam = sc.align_camera()
        points, valid, names = AR.special_planes(cam, *ORIGIN)
        yield sc, cam, points, valid, names


@pytest.mark.parametrize("rng", [64.0, 2.0])
def test_special_cases(special, rng):
    sc, cam, points, valid, names = special
    est, md = np.array(AR.SPECIAL["est"]), AR.SPECIAL["max_dist"]
    ox, oz = float(points[0][12, 20][0]), float(points[0][12, 20][2])
    for v in range(2):
        _put(sc, v, points[v], valid[v])
    want = {w: AR.pass_sums(points, valid, cam, *ORIGIN, est, ox, oz, rng, md, w) for w in WINDOWS}
    for w in WINDOWS:
        assert np.array_equal(sc.align_sums(0, 2, est, ox, oz, rng, md, w), want[w]), w
    # what the cases are for, by the restatement alone
    n_src = int(np.isfinite(points[1].reshape(-1, 3)[:len(names)]).all(axis=1).sum())
    assert all(int(want[w][0, 11]) == n_src == len(names) - 3 for w in WINDOWS)        # NaN and the infinities are no sources
    if rng == 64.0:
        assert want[0][0, 0] < want[1][0, 0] < want[2][0, 0] == want[4][0, 0] < n_src    # the centres outside need the window
    else:
        assert 0 < want[2][0, 0] < AR.pass_sums(points, valid, cam, *ORIGIN, est, ox, oz, 64.0, md, 2)[0, 0]        # the range takes pairs away
    # every case alone, as the only source: the library gives the restatement's words
    for i, name in enumerate(names):
        only = valid.copy()
        only[1] = 0
        only[1].reshape(-1)[i] = 1
        _put(sc, 1, points[1], only[1])
        for w in (0, 1, 2):
            ref = AR.pass_sums(points, only, cam, *ORIGIN, est, ox, oz, rng, md, w)
            assert np.array_equal(sc.align_sums(0, 2, est, ox, oz, rng, md, w), ref), (name, w)
            if rng == 64.0 and w == 1:
                accepted = {"outside far corner": 0, "only odd candidates": 0, "source NaN": 0, "source +inf": 0, "source -inf": 0, "source 3e38": 0,
                            "source -3e38": 0, "behind the camera": 0, "far behind the camera": 0, "distance 0.75": 0,
                            "distance 0.5000152587890625": 0}.get(name, 1)
                assert int(ref[0, 0]) == accepted, name
            if rng == 2.0 and name.endswith("out of range"):
                assert int(ref[0, 0]) == 0 and int(ref[0, 11]) == 1, name


def test_empty_views(special):
    sc, cam, points, valid, names = special
    est, md = np.array(AR.SPECIAL["est"]), AR.SPECIAL["max_dist"]
    ox, oz = float(points[0][12, 20][0]), float(points[0][12, 20][2])
    none = np.zeros_like(valid[0])
    for tv, sv in ((valid[0], none), (none, valid[1]), (none, none)):
        _put(sc, 0, points[0], tv)
        _put(sc, 1, points[1], sv)
        want = AR.pass_sums(points, np.stack([tv, sv]), cam, *ORIGIN, est, ox, oz, 64.0, md, 2)
        assert np.array_equal(sc.align_sums(0, 2, est, ox, oz, 64.0, md, 2), want)
        assert int(want[0, 0]) == 0 and not want[0, 1:11].any()


def test_the_camera_is_the_calibrations():
    syn = pkg("synth")
    with _context(9, 9, 2, run=False) as sc:
        cal = syn.cal_tuple(syn.synth_rig(FULL[0], FULL[1], 2048, 2048))
        cam = sc.align_camera()
        assert cam.shape == (26,) and np.array_equal(cam[9:12], cal[3]) and np.array_equal(cam[12:21], cal[0]) and np.array_equal(cam[21:26], cal[1])
        assert np.allclose(cam[0:9].reshape(3, 3), AR.rodrigues(cal[2]), rtol=0, atol=1e-14)


def test_state_and_refusals():
    S = pkg("scanner")
    est = np.array([1.0, 0.0, 0.0, 0.0])
    with S.Scanner(9, 9, 2048, 2048, 10, 10, 2, 2, max_views=3, full_size=FULL, origin=ORIGIN) as fresh:
        cam = (C.c_double * 26)(*([-7.0] * 26))
        assert fresh.L.sl3d_get_align_camera(fresh._h, cam) == STATE and list(cam) == [-7.0] * 26          # no calibration yet
        sums = np.full((2, 12), -7, np.int64)
        call = lambda sc, **kw: sc.L.sl3d_align_sums(sc._h, kw.get("first", 0), kw.get("n", 3), kw.get("est", est).ctypes.data, kw.get("ox", 0.0),
                                                     kw.get("oz", 0.0), kw.get("rng", 64.0), kw.get("md", 0.5), kw.get("window", 2), sums.ctypes.data)
        assert call(fresh) == STATE and (sums == -7).all()
    with _context(9, 9, 3, run=False) as sc:
        assert call(sc) == STATE and (sums == -7).all()                     # a calibration, but no dense result yet
    with _context(9, 9, 3) as sc:
        cam = sc.align_camera()
        points, valid, e, pads = AR.crafted_views(cam, 9, 9, *ORIGIN, 3, 5)
        for v in range(3):
            _put(sc, v, points[v], valid[v])
        want = AR.pass_sums(points, valid, cam, *ORIGIN, e, e[2], e[3], RANGE, MAX_DIST, 2)
        assert np.array_equal(sc.align_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, 2), want)
        nan, inf = float("nan"), float("inf")
        bad = [dict(n=1), dict(n=0), dict(n=4), dict(first=-1), dict(first=2, n=2), dict(rng=0.0), dict(rng=-1.0), dict(rng=nan), dict(rng=inf),
               dict(md=0.0), dict(md=-0.5), dict(md=nan), dict(md=inf), dict(md=65.0), dict(window=-1), dict(window=5),
               dict(est=np.array([nan, 0.0, 0.0, 0.0])), dict(est=np.array([1.0, 0.0, inf, 0.0])), dict(ox=nan), dict(oz=-inf)]
        for kw in bad:
            assert call(sc, **kw) == INVALID_ARG and (sums == -7).all(), kw
        assert sc.L.sl3d_align_sums(sc._h, 0, 3, None, 0.0, 0.0, 64.0, 0.5, 2, sums.ctypes.data) == INVALID_ARG
        # the asynchronous form: no words, the call returns at once; the next synchronising pass is unaffected
        assert sc.L.sl3d_align_sums(sc._h, 0, 3, e.ctypes.data, float(e[2]), float(e[3]), RANGE, MAX_DIST, 2, None) == 0
        sc.synchronize()
        assert np.array_equal(sc.align_sums(0, 3, e, e[2], e[3], RANGE, MAX_DIST, 2), want)
        assert sc.L.sl3d_get_align_camera(sc._h, None) == INVALID_ARG
