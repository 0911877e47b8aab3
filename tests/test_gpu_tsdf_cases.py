"""GPU tests (-m gpu) of the integration of views into a TSDF volume: sl3d_tsdf_reset / sl3d_tsdf_integrate / k_tsdf_integrate
against the NumPy restatement of the rule (tests/tsdf_reference.py), sum, weight and both counts word for word, with the camera taken from
sl3d_get_align_camera.

The inputs go into a context's dense planes through tests/dense_planes.put_dense behind sc.run(); sc.synchronize().  Every context is a
window with col0, row0 != 0 inside a larger full frame, at most 48 x 36.  k_tsdf_integrate takes a voxel a lane, 256 a block, i along the wave.

1. Volumes (5, 3, 2) below a wave, (64, 1, 1), (65, 3, 2) across lane 64 in i, (33, 9, 7) with a last partial block and (70, 33, 5), over five
   crafted turntable views (tests/tsdf_cases.shape_case: noise, outliers that trip the depth guard, invalid pixels): 1, 2 and 5 views,
   first_step 0 and 3, views from slot 1 on, two calls that must equal one call over the same views, and a reset that clears.  At 48
   columns the pitch is 48: these views have no padding columns (tests/test_gpu_tsdf_layouts.py runs several views on windows that
   have them, with perfect points under valid bytes there).
2. One voxel each (tests/tsdf_cases.special_cases, an exact camera): a centre behind the camera, a projection on the last usable column
   and row and one past it, one of the four pixels invalid, a NaN or an infinity under a valid byte, a depth spread exactly T and just
   above, sdf exactly -T and just below, d clamped at 1, d * 32767 on a tie.
3. The call's protocol: the asynchronous form, the state the calls need, every refusal, each checked to have changed nothing.
Padded and wide windows, windows without a cell, the int32 bound of sum and the last turntable indices: tests/test_gpu_tsdf_layouts.py."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reference as TR
from conftest import pkg
from tsdf_gpu import INVALID_ARG, STATE, UNSUPPORTED, check_planes, context, put, reset

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
def test_shapes_views_and_steps(views, dims):
    sc, cam, points, valid, est = views
    vol = TC.shape_case(cam, dims, 1, 11)[4]

    def fused(first_view, n_views, first_step):
        s, w = TR.new_volume(vol)
        counts = TR.integrate(s, w, vol, points[first_view:first_view + n_views], valid[first_view:first_view + n_views], cam, *TC.ORIGIN, est, first_step)
        return s, w, list(counts)
    for first_view, n_views, first_step in ((0, 1, 0), (0, 2, 0), (0, 5, 0), (0, 2, 3), (1, 3, 1)):
        s, w, counts = fused(first_view, n_views, first_step)
        reset(sc, vol)
        assert sc.tsdf_integrate(first_view, n_views, est, first_step) == counts, (first_view, n_views, first_step)
        check_planes(sc, vol, s, w)
    # two calls equal one call over the same views: the second call's counts are its own samples and the volume's occupancy
    s5, w5, c5 = fused(0, 5, 0)
    s2, w2, c2 = fused(0, 2, 0)
    reset(sc, vol)
    assert sc.tsdf_integrate(0, 2, est, 0) == c2
    assert sc.tsdf_integrate(2, 3, est, 2) == [c5[0] - c2[0], c5[1]]
    check_planes(sc, vol, s5, w5)
    if np.prod(dims) >= 900:                                                # by the restatement alone: both outcomes, and views that disagree
        assert (w5 == 0).any() and (w5 == 5).any() and ((w5 > 0) & (w5 < 5)).any() and 0 < c2[0] < c5[0]
        assert not np.array_equal(fused(0, 2, 3)[0], s2)                    # first_step matters
    reset(sc, vol)                                                          # a reset clears
    check_planes(sc, vol, *TR.new_volume(vol))
    assert np.array_equal(sc.points(1)[0].view(np.uint32), points[1].view(np.uint32))          # the calls wrote no plane


@pytest.fixture(scope="module")
def exact():
    with context(TC.EXACT["W"], TC.EXACT["H"], 2, cal=TC.exact_calibration()) as sc:
        cam = sc.align_camera()
        assert np.array_equal(cam, TC.camera(TC.exact_calibration()))       # Rc = I, tc = 0, the Kc and dc of tests/tsdf_cases.py, to the bit
        yield sc, cam


def test_special_cases(exact):
    sc, cam = exact
    xyz, valid, pad, cases = TC.special_cases()
    put(sc, 0, xyz, valid, pad)
    for name, vol, weight, q in cases:
        s, w = TR.new_volume(vol)
        counts = list(TR.integrate(s, w, vol, xyz[None], valid[None], cam, *TC.ORIGIN, TC.IDENTITY))
        assert int(w[0]) == weight and (q is None or int(s[0]) == q), name  # what the case is for, by the restatement alone
        reset(sc, vol)
        assert sc.tsdf_integrate(0, 1, TC.IDENTITY) == counts == [weight, weight], name
        check_planes(sc, vol, s, w)


def test_state_and_refusals(views):
    S = pkg("scanner")
    sc0, cam, points, valid, est = views
    vol = TC.shape_case(cam, (5, 3, 2), 1, 11)[4]
    counts = (C.c_int64 * 3)(-7, -7, -7)
    n = C.c_int64(-7)

    def volume(**kw):
        o = kw.get("origin", vol["origin"])
        return S.TsdfVolume((C.c_float * 3)(*[float(x) for x in o]), kw.get("voxel", 1.0), kw.get("trunc", 3.0), (C.c_int32 * 3)(*kw.get("dims", (5, 3, 2))))

    def integrate(sc, **kw):
        e = np.ascontiguousarray(kw.get("est", est), np.float64)
        return sc.L.sl3d_tsdf_integrate(sc._h, kw.get("first", 0), kw.get("n", 2), kw.get("step", 0), e.ctypes.data, counts)
    W, H = TC.FRAME
    with S.Scanner(W, H, 2048, 2048, 10, 10, 2, 2, max_views=2, full_size=TC.FULL, origin=TC.ORIGIN) as fresh:
        v = volume()
        assert fresh.L.sl3d_tsdf_reset(fresh._h, C.byref(v)) == 0           # a volume needs neither a calibration nor a dense result
        assert integrate(fresh) == STATE and list(counts) == [-7] * 3       # ... an integration does: no calibration
    with context(W, H, 2, run=False) as sc:
        v = volume()
        assert sc.L.sl3d_tsdf_reset(sc._h, C.byref(v)) == 0
        assert integrate(sc) == STATE and list(counts) == [-7] * 3          # a calibration, but no dense result yet
    with context(W, H, 2) as sc:
        # before a reset
        assert integrate(sc) == STATE and list(counts) == [-7] * 3
        assert sc.L.sl3d_tsdf_extract(sc._h, 1, None, counts) == STATE and list(counts) == [-7] * 3
        assert sc.L.sl3d_get_tsdf(sc._h, None, None, 0, C.byref(n)) == STATE and n.value == -7
        assert sc.L.sl3d_get_tsdf_surface(sc._h, None, None, None, 0, C.byref(n)) == STATE and n.value == -7
        nan, inf = float("nan"), float("inf")
        bad = [dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(trunc=0.0), dict(trunc=-3.0), dict(trunc=nan), dict(trunc=inf),
               dict(origin=(nan, 0.0, 0.0)), dict(origin=(0.0, -inf, 0.0)), dict(origin=(0.0, 0.0, inf)), dict(dims=(0, 3, 2)), dict(dims=(5, -1, 2)),
               dict(dims=(5, 3, 0)), dict(dims=(1 << 14, 1 << 14, 2)), dict(dims=(1 << 16, 1 << 16, 1 << 16)), dict(dims=((1 << 28) + 1, 1, 1))]
        for kw in bad:
            v = volume(**kw)
            assert sc.L.sl3d_tsdf_reset(sc._h, C.byref(v)) == INVALID_ARG, kw
            assert integrate(sc) == STATE, kw                               # the refused reset defined nothing
        assert sc.L.sl3d_tsdf_reset(sc._h, None) == INVALID_ARG
        for v in range(2):
            put(sc, v, points[v], valid[v])
        reset(sc, vol)
        assert sc.L.sl3d_get_tsdf_surface(sc._h, None, None, None, 0, C.byref(n)) == STATE and n.value == -7          # no extraction yet
        s, w = TR.new_volume(vol)
        want = list(TR.integrate(s, w, vol, points[:2], valid[:2], cam, *TC.ORIGIN, est))
        assert sc.tsdf_integrate(0, 2, est) == want
        bad = [dict(n=0), dict(n=-1), dict(n=3), dict(first=-1), dict(first=1, n=2), dict(first=2, n=1), dict(step=-1), dict(step=65534), dict(step=65535),
               dict(est=np.array([nan, 0.0, 0.0, 0.0])), dict(est=np.array([1.0, 0.0, inf, 0.0])), dict(est=np.array([1.0, -inf, 0.0, 0.0]))]
        for kw in bad:
            assert integrate(sc, **kw) == INVALID_ARG and list(counts) == [-7] * 3, kw
            check_planes(sc, vol, s, w)
        assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 2, 0, None, counts) == INVALID_ARG and list(counts) == [-7] * 3
        assert integrate(sc, step=65533) == 0 and list(counts) != [-7] * 3  # the last admissible index
        reset(sc, vol)
        assert sc.tsdf_integrate(0, 2, est) == want
        counts[:] = [-7] * 3
        for mw in (0, -1):
            assert sc.L.sl3d_tsdf_extract(sc._h, mw, None, counts) == INVALID_ARG and list(counts) == [-7] * 3
        words = np.full(4, -7, np.int32)
        assert sc.L.sl3d_get_tsdf(sc._h, words.ctypes.data, None, -1, C.byref(n)) == INVALID_ARG and (words == -7).all()
        assert sc.L.sl3d_get_tsdf(sc._h, words.ctypes.data, None, 4, None) == INVALID_ARG and (words == -7).all()
        check_planes(sc, vol, s, w)
        # size then fill with a capacity below the total: the first words only
        assert sc.L.sl3d_get_tsdf(sc._h, words.ctypes.data, None, 3, C.byref(n)) == 0 and n.value == 30
        assert np.array_equal(words[:3], s[:3]) and words[3] == -7
        # the asynchronous form: no counts, the call returns at once; what follows is unaffected
        e = np.ascontiguousarray(est, np.float64)
        reset(sc, vol)
        assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 1, 0, e.ctypes.data, None) == 0
        assert sc.L.sl3d_tsdf_integrate(sc._h, 1, 1, 1, e.ctypes.data, None) == 0
        sc.synchronize()
        check_planes(sc, vol, s, w)


def test_the_view_limit(views):
    """65,535 views since the last reset: the call that would pass the limit is refused with SL3D_E_UNSUPPORTED and changes nothing.  One
    voxel far outside every frame, so that the 13,107 calls of five views cost a launch each and nothing else."""
    sc, cam, points, valid, est = views
    vol = dict(origin=np.array([1e6, 1e6, 1e6], np.float32), voxel=np.float32(1.0), trunc=np.float32(3.0), dims=(1, 1, 1))
    reset(sc, vol)
    e = np.ascontiguousarray(est, np.float64)
    for _ in range(65535 // 5):
        assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 5, 0, e.ctypes.data, None) == 0
    counts = (C.c_int64 * 2)(-7, -7)
    assert sc.L.sl3d_tsdf_integrate(sc._h, 0, 1, 0, e.ctypes.data, counts) == UNSUPPORTED and list(counts) == [-7, -7]
    check_planes(sc, vol, *TR.new_volume(vol))
    reset(sc, vol)                                                          # a reset starts the count again
    assert sc.tsdf_integrate(0, 1, est) == [0, 0]
