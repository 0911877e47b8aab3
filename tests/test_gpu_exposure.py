"""GPU tests (-m gpu) of the exposure fusion: sl3d_fuse_exposures / k_fuse_exposures against the NumPy restatement of the rule
(tests/exposure_reference.py), bit for bit -- frames, map and counts.

1. Crafted bytes from the alphabet {0, 10, 200, 254, 255} (clip-count ties and score ties are frequent; half the pixels draw whole plane
   vectors from a pool of six, and two pairs of exposures are identical: the smallest-e rule decides), over the shapes 64x7, 67x9, 322x13,
   1920x3, E = 1, 2, 3, 8, saturation 255, 200, 256, 1, F = 3 and 4, (N_v, N_h) = (7, 7), (6, 5), (0, 4), (16, 16), dst_view below and above
   the sources, sources that do not start at view 0.
2. Flags: an integer context, SUBPIXEL | DIRECT_GRAY, SUBPIXEL | ONLY_VERTICAL, SUBPIXEL | ONLY_HORIZONTAL | DIRECT_GRAY, KEEP_STAGES.  The
   planes not in use hold 255 in the sources and a marker in dst_view: the result is the restatement's, the marker is still there.
3. The decode property on the three-band scene: sl3d_run of the fused view gives, pixel by pixel, what it gives of the exposure the map
   names; on the lit pixels what it gives of the gain-0.8 capture; every single exposure equals that capture on strictly fewer pixels.
4. Ordering behind the launch lanes, a second fusion into the same dst_view, a fused view used as a source.
5. Every refusal, each leaving frames and map as they were; map and counts agree."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import pkg

import exposure_reference as XR
from exposure_cases import _crafted

pytestmark = pytest.mark.gpu

MARKER = 0x5C
SHAPES = [(64, 7), (67, 9), (322, 13), (1920, 3)]
GRAYS = [(7, 7), (6, 5), (0, 4), (16, 16)]
EXPOSURES = (1, 2, 3, 8)
SATURATIONS = (255, 200, 256, 1)
INVALID_ARG, STATE, UNSUPPORTED = -1, -4, -5


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _ppv(F, N):
    return 2 * F + 2 * N[0] + 2 * N[1]


def _scanner(W, H, N, F=3, max_views=1, **kw):
    return pkg("scanner").Scanner(W, H, 512, 384, N[0], N[1], 4, 4, n_fringe=F, max_views=max_views, **kw)


def _upload(sc, view, planes, F, N):
    b = F + 2 * N[0]
    sc.set_frames(0, list(planes[:b]), view=view)
    sc.set_frames(1, list(planes[b:]), view=view)


def _download(sc, view):
    return np.stack(sc.frames(0, view) + sc.frames(1, view))


def _check_fusion(sc, stack, first, E, dst, sat, F, N, flags, what):
    """fuse views [first, first + E) (which hold stack[0 .. E)) into dst and compare with the restatement; returns (fused planes, map)"""
    counts = sc.fuse_exposures(first, E, dst, saturation=sat)
    want_f, want_m, want_c = XR.fuse(stack[:E], F, N[0], N[1], flags, sat)
    use = XR.planes_in_use(F, N[0], N[1], flags)
    got_f, got_m = _download(sc, dst), sc.exposure_map(dst)
    assert counts.dtype == np.uint32 and np.array_equal(counts, want_c), (what, counts, want_c)
    assert np.array_equal(got_m, want_m), (what, int((got_m != want_m).sum()), "map bytes differ")
    assert np.array_equal(got_f[use], want_f[use]), (what, int((got_f[use] != want_f[use]).sum()), "frame bytes differ")
    assert np.array_equal(counts[:E], np.bincount((got_m & 7).ravel(), minlength=E)) and counts[E] == int((got_m & 0x80).astype(bool).sum()), what
    return got_f, got_m


# ---- 1. crafted bytes: device == restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4])
@pytest.mark.parametrize("N", GRAYS, ids=lambda n: "N%d_%d" % n)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_crafted_bytes_equal_the_restatement(shape, N, F):
    (W, H), ppv = shape, _ppv(F, N)
    stack = _crafted(W, H, ppv, 1000 * W + 10 * ppv + F)
    ties = 0
    with _scanner(W, H, N, F, max_views=12) as sc:                      # exposures in views 1 .. 8, dst_view 0 (below) or 9 .. 11 (above)
        for e in range(8):
            _upload(sc, 1 + e, stack[e], F, N)
        k = 0
        for E in EXPOSURES:
            for sat in SATURATIONS:
                first = 1 if k % 2 == 0 else 9 - E                      # the first E exposures, or the last E
                dst = (0, 9, 11, 1 + 8)[k % 4] if first + E <= 9 else 0
                src = stack[first - 1:first - 1 + E]
                _, m = _check_fusion(sc, src, first, E, dst, sat, F, N, 0, (shape, N, F, E, sat, first, dst))
                if E == 8 and first == 1:                               # exposure 2 is exposure 0, exposure 6 is exposure 3: never chosen
                    assert not np.isin(m & 7, (2, 6)).any()
                    ties += 1
                k += 1
        assert ties
        for e in range(8):                                              # the sources are as they were
            assert np.array_equal(_download(sc, 1 + e), stack[e]), ("source view", 1 + e)


def test_crafted_bytes_hold_the_ties_the_rule_is_about():
    """The yardstick's inputs do what the docstring says: with all eight exposures, many pixels have several exposures at the smallest clip
    count, and many have several of those at the largest score (only the smallest e separates them)."""
    F, N = 3, (6, 5)
    stack = _crafted(67, 9, _ppv(F, N), 1)
    use = XR.planes_in_use(F, *N, 0)
    n = (stack[:, use] >= 255).sum(axis=1)
    q = np.minimum(XR.score(F, stack[:, 0:F].transpose(1, 0, 2, 3)), XR.score(F, stack[:, F + 2 * N[0]:][:, :F].transpose(1, 0, 2, 3)))
    fewest = n == n.min(axis=0)
    best = fewest & (q == np.where(fewest, q, -1).max(axis=0))
    assert (fewest.sum(axis=0) > 1).mean() > 0.3 and (best.sum(axis=0) > 1).mean() > 0.2


# ---- 2. flags ----------------------------------------------------------------------------------------------------------------------------------
FLAGGED = {
    "integer": (0, {}),
    "subpixel_direct": (XR.DIRECT_GRAY, dict(subpixel=True, direct_gray=True)),
    "subpixel_vertical": (XR.ONLY_VERTICAL, dict(subpixel=True, only_axis=0)),
    "subpixel_horizontal_direct": (XR.ONLY_HORIZONTAL | XR.DIRECT_GRAY, dict(subpixel=True, only_axis=1, direct_gray=True)),
    "keep_stages": (0, dict(keep_stages=True)),
}


@pytest.mark.parametrize("F", [3, 4])
@pytest.mark.parametrize("name", FLAGGED)
def test_flags_decide_the_planes_in_use(name, F):
    flags, kw = FLAGGED[name]
    (W, H), N = (67, 9), (6, 5)
    ppv = _ppv(F, N)
    use = XR.planes_in_use(F, N[0], N[1], flags)
    unused = [p for p in range(ppv) if p not in use]
    assert bool(unused) == (flags != 0)
    stack = _crafted(W, H, ppv, 77 + F)[:3].copy()
    stack[:, unused] = 255                                              # clipped wherever nothing may look
    with _scanner(W, H, N, F, max_views=5, **kw) as sc:
        for e in range(3):
            _upload(sc, 1 + e, stack[e], F, N)
        for dst, sat in ((0, 255), (4, 200)):
            _upload(sc, dst, np.full((ppv, H, W), MARKER, np.uint8), F, N)
            got, _ = _check_fusion(sc, stack, 1, 3, dst, sat, F, N, flags, (name, F, dst, sat))
            assert (got[unused] == MARKER).all(), (name, "the planes not in use keep what they held")
        for e in range(3):
            assert np.array_equal(_download(sc, 1 + e), stack[e])


# ---- 3. the decode property --------------------------------------------------------------------------------------------------------------------
SCENE = dict(W=96, H=40, PW=512, PH=384, N=7, fw=4)


@functools.lru_cache(maxsize=None)
def _scene(F):
    s = SCENE
    return XR.three_band_scene(pkg("synth"), s["W"], s["H"], s["PW"], s["PH"], s["N"], s["fw"], F)


def _scene_scanner(F, max_views, **kw):
    s = SCENE
    sc = pkg("scanner").Scanner(s["W"], s["H"], s["PW"], s["PH"], s["N"], s["N"], s["fw"], s["fw"], n_fringe=F, max_views=max_views, **kw)
    sc.set_calibration(*pkg("synth").cal_tuple(_scene(F)["cal"]))
    return sc


def _result(sc, view, residual):
    """the dense result of a view as bit patterns: [H][W][4 or 5] -- valid, x, y, z(, residual)"""
    xyz, valid = sc.points(view)
    parts = [valid.astype(np.uint32)[..., None], _bits(xyz)] + ([_bits(sc.residuals(view))[..., None]] if residual else [])
    return np.concatenate(parts, axis=-1)


@pytest.mark.parametrize("name,F,kw", [("plain", 3, {}), ("plain_four_step", 4, {}), ("subpixel_anchored", 3, dict(subpixel=True, anchored=True))],
                         ids=["plain", "plain_four_step", "subpixel_anchored"])
def test_decode_of_the_fused_view(name, F, kw):
    sn, N = _scene(F), (SCENE["N"], SCENE["N"])
    lit = sn["lit"]
    with _scene_scanner(F, 5, **kw) as sc:
        for e in range(3):
            _upload(sc, e, sn["stack"][e], F, N)
        _upload(sc, 4, sn["base"], F, N)                                # the gain-0.8 capture in a further view
        sc.set_masks(sn["mask"])                                        # one mask for all views
        counts = sc.fuse_exposures(0, 3, 3)
        emap = sc.exposure_map(3)
        sc.run(0, 5)
        res = [_result(sc, v, bool(kw)) for v in range(5)]
    assert counts[3] == 0 and np.array_equal(emap[lit], sn["band"][lit])
    fused, base = res[3], res[4]
    assert (base[..., 0] == 1)[lit].mean() > 0.5, "the capture decodes on most lit pixels"
    picked = np.take_along_axis(np.stack(res[:3]), (emap & 7).astype(np.int64)[None, ..., None], axis=0)[0]
    assert np.array_equal(fused, picked), "every pixel: the result of the exposure the map names"
    assert np.array_equal(fused[lit], base[lit]), "the lit pixels: the result of the gain-0.8 capture"
    same_fused = int((fused == base).all(axis=-1).sum())
    for e in range(3):
        same = int((res[e] == base).all(axis=-1).sum())
        print(f"{name}: exposure {e} equals the capture's result on {same} pixels, the fused view on {same_fused} of {lit.size}")
        assert same < same_fused


# ---- 4. ordering -------------------------------------------------------------------------------------------------------------------------------
def _ordering_sequence(sc, sn, F, N, series):
    """exposures in views 0 .. 2, other sources (exposures 2, 0) in views 4, 5, dst_view 3; returns everything a caller can observe"""
    for v, e in ((0, 0), (1, 1), (2, 2), (3, 1), (4, 2), (5, 0)):
        _upload(sc, v, sn["stack"][e], F, N)
    sc.set_masks(sn["mask"])
    sc.synchronize()
    if series:
        for i in range(10):                                             # dst_view and a source in turn: the last two launches go to the lanes
            sc.run(3 if i % 2 == 0 else 0, 1)
        assert sc.launch_counts()[1] > 0, "the series put the launch lanes to use"
    out = []
    out.append(_check_fusion(sc, sn["stack"], 0, 3, 3, 255, F, N, 0, "behind the series"))
    sc.run(3, 1)
    out.append(_result(sc, 3, False))
    src = np.stack([sn["stack"][2], sn["stack"][0]])
    out.append(_check_fusion(sc, src, 4, 2, 3, 255, F, N, 0, "a second fusion into the same dst_view, other sources"))
    sc.run(3, 1)
    out.append(_result(sc, 3, False))
    src = np.stack([out[-2][0], sn["stack"][2]])
    out.append(_check_fusion(sc, src, 3, 2, 5, 255, F, N, 0, "a fused view as a source"))
    sc.run(5, 1)
    out.append(_result(sc, 5, False))
    return out


def test_fusion_comes_behind_the_launch_lanes():
    F, N = 3, (SCENE["N"], SCENE["N"])
    sn = _scene(F)
    with _scene_scanner(F, 6) as lanes, _scene_scanner(F, 6, serial_launches=True) as serial:
        got, want = _ordering_sequence(lanes, sn, F, N, True), _ordering_sequence(serial, sn, F, N, False)
        assert serial.launch_counts()[1] == 0
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g if isinstance(g, tuple) else (g,), w if isinstance(w, tuple) else (w,)):
            assert np.array_equal(a, b), ("step", k)
    assert not np.array_equal(got[0][1], got[2][1]), "the second fusion chose differently"
    assert (got[1][..., 0] == 1).any()


# ---- 5. contracts ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_frames_and_map_as_they_were():
    S = pkg("scanner")
    (W, H), N, F = (67, 9), (6, 5), 3
    stack = _crafted(W, H, _ppv(F, N), 5)
    with _scanner(W, H, N, F, max_views=6) as sc:
        L, h = sc.L, sc._h
        for e in range(4):
            _upload(sc, 1 + e, stack[e], F, N)
        out = np.zeros((H, W), np.uint8)
        assert L.sl3d_get_exposure_map(h, 5, out.ctypes.data, W) == STATE          # no fusion yet on this context
        assert "no sl3d_fuse_exposures" in L.sl3d_last_error(h).decode()
        _, m0 = _check_fusion(sc, stack, 1, 4, 5, 255, F, N, 0, "the fusion the refusals follow")
        before = [_download(sc, v) for v in range(6)]
        counts = (C.c_uint32 * 9)(*[0xDEADBEEF] * 9)
        refused = [(-1, 2, 5, 255), (5, 2, 0, 255), (4, 3, 0, 255), (0, 2, 6, 255), (0, 2, -1, 255),      # a view out of range
                   (1, 0, 5, 255), (1, 9, 5, 255), (0, -1, 5, 255),                                         # n_exposures outside 1 .. 8
                   (1, 3, 1, 255), (1, 3, 2, 255), (1, 3, 3, 255), (5, 1, 5, 255),                           # dst_view is an exposure
                   (1, 3, 5, 0), (1, 3, 5, 257), (1, 3, 5, -1)]                                              # saturation outside 1 .. 256
        for first, E, dst, sat in refused:
            for c in (counts, None):
                assert L.sl3d_fuse_exposures(h, first, E, dst, sat, c) == INVALID_ARG, (first, E, dst, sat)
        assert all(c == 0xDEADBEEF for c in counts)
        for view, ptr, stride in ((5, None, W), (5, out.ctypes.data, W - 1), (6, out.ctypes.data, W), (-1, out.ctypes.data, W)):
            assert L.sl3d_get_exposure_map(h, view, ptr, stride) == INVALID_ARG, (view, stride)
        assert L.sl3d_get_exposure_map(h, 0, out.ctypes.data, W) == STATE           # a view no fusion has written
        with pytest.raises(S.Sl3dError):
            sc.exposure_map(0)
        assert not out.any()
        for v in range(6):
            assert np.array_equal(_download(sc, v), before[v]), ("frames after the refusals", v)
        assert np.array_equal(sc.exposure_map(5), m0)
        # counts=False: enqueued, nothing returned, the same result
        assert sc.fuse_exposures(2, 2, 0, saturation=200, counts=False) is None
        want_f, want_m, _ = XR.fuse(stack[1:3], F, N[0], N[1], 0, 200)
        assert np.array_equal(sc.exposure_map(0), want_m) and np.array_equal(_download(sc, 0), want_f)
        assert np.array_equal(sc.exposure_map(5), m0)                               # a view's map stays until a fusion writes that view
    with _scanner(W, H, N, 5, max_views=3) as sc:                                   # five fringes: no score is defined
        ppv = _ppv(5, N)
        for v in range(3):
            _upload(sc, v, np.full((ppv, H, W), 10 * v + 1, np.uint8), 5, N)
        assert sc.L.sl3d_fuse_exposures(sc._h, 0, 2, 2, 255, None) == UNSUPPORTED
        assert "n_fringe" in sc.L.sl3d_last_error(sc._h).decode()
        assert sc.L.sl3d_get_exposure_map(sc._h, 2, out.ctypes.data, W) == STATE
        for v in range(3):
            assert (_download(sc, v) == 10 * v + 1).all()
