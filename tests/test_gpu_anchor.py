"""GPU tests (-m gpu) of SL3D_FLAG_ANCHOR_PERIODS on the captures of tests/subpixel_cases.py (320 x 240 full frame; the 70 x 9
window at (37, 5); plain, radial and tangential rigs).

1. The staged route (KEEP_STAGES | SUBPIXEL | ANCHOR_PERIODS): sl3d_get_correspondences_subpixel against the NumPy restatement of the
   definition (tests/anchor_reference.py) applied to the very planes downloaded before the call, bit for bit, NaN pattern included;
   sl3d_triangulate_subpixel(+inf) against tests/subpixel_reference.py at those coordinates within the bars of tests/test_gpu_subpixel.py
   (1e-5 relative on points, 1e-6 * ref + 1e-7 px on residuals); the merged valid map, c_p_map and the unwrapped planes byte for byte those
   of an unflagged context.
2. A finite max_residual: rejections and counts equal the restatement's, at thresholds asserted on the restatement to take both branches
   clear of ties.
3. The timed context (SUBPIXEL | ANCHOR_PERIODS): sl3d_run equals the staged route bit for bit on points, valid and residual.
4. A group of three stripes equals the single context.  5. The refusals.  6. The accuracy the flag is for.  7. The kernel names."""
import functools

import numpy as np
import pytest

from conftest import assert_points_close, pkg

import anchor_reference as AR
import subpixel_cases as SC
import subpixel_reference as SR
from test_anchor_arith import accuracy

pytestmark = pytest.mark.gpu

INF = float("inf")
NAME = "sl3d::k_subpixel_fused<true>"
# max_residual of test 2, per scene: inputs of the call (the window of the plain rig holds no pixel that is off by a period: its residuals
# end at 0.005 px; the capture does not model the projector's distortion, which is what the other two rigs' residuals show)
THRESHOLDS = {("plain", "full"): 1.0, ("radial", "full"): 1.0, ("tangential", "full"): 1.0,
              ("plain", "window"): 0.003, ("radial", "window"): 0.61, ("tangential", "window"): 0.345}


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _open(rig, win, *, keep=False, anchored=True, max_views=1, eager_mask=False):
    s = SC.scene(rig, win)
    sc = pkg("scanner").Scanner(s["W"], s["H"], SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW, keep_stages=keep, full_size=SC.FULL, origin=s["origin"],
                                max_views=max_views, subpixel=True, anchored=anchored, eager_mask=eager_mask)
    sc.set_calibration(*s["cal"])
    return sc


def _frames(sc, cap, view=0):
    sc.set_frames(0, cap["planes_v"], view=view)
    sc.set_frames(1, cap["planes_h"], view=view)


def _load(sc, cap, view=0, mask=None):
    _frames(sc, cap, view)
    sc.set_mask(pkg("synth").default_mask(*SC.FULL) if mask is None else mask, view=view)


def _stages345(sc, view=0):
    for a in (0, 1):
        sc.compute_wrapped_phase(a, view)
    for a in (0, 1):
        sc.unwrap_phase(a, view)
    sc.compute_c_p_map(view)


def _inputs(sc, view=0):
    """What the anchored calls read, downloaded before them."""
    return dict(w=(sc.wrapped_phase(0, view), sc.wrapped_phase(1, view)), code=(sc.code(0, view), sc.code(1, view)),
                unw=(sc.unwrapped_phase(0, view), sc.unwrapped_phase(1, view)), valid_axis=(sc.valid_map(0, view), sc.valid_map(1, view)),
                valid=sc.valid_map(view=view), c_p_map=sc.c_p_map(view), A=sc.projection_matrices())


def _restate_xy(inp, origin, fw=(SC.FW, SC.FW), n_fringe=3, n_gray=(SC.N, SC.N), full=SC.FULL):
    return AR.correspondences(inp["w"], inp["code"], inp["unw"], inp["valid_axis"], fw, n_fringe, n_gray, origin, full)


def _restate(inp, cal, origin, max_residual=INF):
    return SR.triangulate(_restate_xy(inp, origin), inp["valid"], cal, *inp["A"], origin, max_residual)


def _out(sc, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid, residual=sc.residuals(view))


def _same(got, want, what):
    for k in ("valid", "points", "residual"):
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _sane(want, what, some_valid=True):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1}
    assert v.any() == some_valid, what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["residual"]), ~v), what


def _check(got, want, what):
    """The device's planes of one view against the restatement's, at the bars of tests/test_gpu_subpixel.py."""
    assert np.array_equal(got["valid"], want["valid"]), (what, "valid map", int((got["valid"] != want["valid"]).sum()))
    v = want["valid"] == 1
    assert v.sum() > 0
    assert np.array_equal(np.isnan(got["points"]).any(-1), ~v) and np.array_equal(np.isnan(got["points"]).all(-1), ~v), (what, "NaN pattern of points")
    e_f = assert_points_close(got["points"], want["ipoints"], v)
    t = ~np.isnan(want["residual"])
    assert np.array_equal(~np.isnan(got["residual"]), t), (what, "NaN pattern of the residuals")
    ref = want["residual"][t].astype(np.float64)
    err = np.abs(got["residual"][t].astype(np.float64) - ref)
    k = int(np.argmax(err - 1e-6 * ref))
    print(f"{what}: points {e_f:.2e} rel, residuals max |diff| {err.max():.2e} px (at {ref[k]:.3g} px: {err[k]:.2e})")
    assert (err <= 1e-6 * ref + 1e-7).all(), (what, float(err[k]), float(ref[k]))


@functools.lru_cache(maxsize=None)
def _staged(rig, win):
    """Per scene, computed once and left unchanged, on a KEEP_STAGES | SUBPIXEL | ANCHOR_PERIODS context: the inputs stage 4 and 5 leave,
    the coordinates, and the planes sl3d_triangulate_subpixel(+inf) leaves -- the yardstick of the timed context."""
    s = SC.scene(rig, win)
    with _open(rig, win, keep=True) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        inp = _inputs(sc)
        xy = sc.correspondences_subpixel()
        counts = sc.triangulate_subpixel()
        want = _out(sc)
        after = dict(valid=sc.valid_map(), c_p_map=sc.c_p_map(), unw=(sc.unwrapped_phase(0), sc.unwrapped_phase(1)))
    _sane(want, (rig, win))
    return dict(inp=inp, xy=xy, counts=counts, want=want, after=after)


# ---- 1. the staged route against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_staged_route_equals_the_restatement(rig, win):
    s, y = SC.scene(rig, win), _staged(rig, win)
    inp = y["inp"]
    want_xy = _restate_xy(inp, s["origin"])
    nan = np.isnan(want_xy)
    assert np.array_equal(np.isnan(y["xy"]), nan) and nan.sum() < nan.size, "NaN pattern of the coordinates"
    assert np.array_equal(_bits(y["xy"])[~nan], _bits(want_xy)[~nan]), int((_bits(y["xy"])[~nan] != _bits(want_xy)[~nan]).sum())
    plain = SR.correspondences(*inp["unw"], *inp["valid_axis"], SC.FW, SC.FW)
    v = inp["valid"] == 1
    assert (y["xy"][v] != plain[v]).mean() > 0.9, "the anchored coordinates are not the unanchored ones"
    want = _restate(inp, s["cal"], s["origin"])
    assert y["counts"] == [want["counts"]] and y["counts"][0][1] == 0
    _check(y["want"], want, (rig, win))
    # validity, c_p_map and the unwrapped planes: those of a context without the flag, before and after the call
    with _open(rig, win, keep=True, anchored=False) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        plain_inp = _inputs(sc)
        plain_xy = sc.correspondences_subpixel()
    assert np.array_equal(_bits(plain_xy)[~nan], _bits(plain)[~nan]), "a context without the flag behaves as before"
    for k in ("valid", "c_p_map"):
        assert np.array_equal(plain_inp[k], inp[k]) and np.array_equal(plain_inp[k], y["after"][k]), k
    for a in (0, 1):
        assert np.array_equal(_bits(plain_inp["unw"][a]), _bits(inp["unw"][a])) and np.array_equal(_bits(plain_inp["unw"][a]), _bits(y["after"]["unw"][a]))
        assert np.array_equal(_bits(plain_inp["w"][a]), _bits(inp["w"][a])) and np.array_equal(plain_inp["code"][a], inp["code"][a])


# ---- 2. a finite max_residual --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_rejection_equals_the_restatement(rig, win):
    s, y = SC.scene(rig, win), _staged(rig, win)
    thr = THRESHOLDS[(rig, win)]
    free = _restate(y["inp"], s["cal"], s["origin"])
    res = free["residual"][y["inp"]["valid"] == 1].astype(np.float64)
    rejected = ~(res <= thr)
    assert np.isfinite(res).all() and rejected.sum() >= 1 and (~rejected).mean() >= 0.8, (int(rejected.sum()), float((~rejected).mean()))
    assert (np.abs(res - thr) > 1e-4 * thr).all(), "the threshold must stay clear of every residual"
    want = _restate(y["inp"], s["cal"], s["origin"], max_residual=thr)
    with _open(rig, win, keep=True) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        counts = sc.triangulate_subpixel(max_residual=thr)
        got = _out(sc)
    assert counts == [want["counts"]] and counts[0] == (len(res), int(rejected.sum()))
    _check(got, want, (rig, win, "threshold", thr))
    gone = (y["inp"]["valid"] == 1) & (got["valid"] == 0)
    assert gone.sum() == rejected.sum() and np.isnan(got["points"][gone]).all() and np.isfinite(got["residual"][gone]).all()


# ---- 3. the timed context ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_run_equals_the_staged_route(rig, win):
    s, y = SC.scene(rig, win), _staged(rig, win)
    with _open(rig, win) as sc:
        assert sc.fused_kernel_name(1) == NAME and sc.camera_table_bytes_per_pixel(1) == 0
        _load(sc, s["cap"])
        sc.run()
        _same(_out(sc), y["want"], (rig, win))
        assert sc.last_fused_kernel_name() == NAME and sc.launch_counts() == (1, 0)
    with _open(rig, win, keep=True) as sc:                      # KEEP_STAGES: the parity launch + the anchored k_subpixel
        _load(sc, s["cap"])
        sc.run()
        _same(_out(sc), y["want"], (rig, win, "KEEP_STAGES"))
        assert sc.last_fused_kernel_name().startswith("sl3d::k_fused<true")
    with _open(rig, win, anchored=False) as sc:                 # no flag: the sub-pixel scan as it was
        _load(sc, s["cap"])
        sc.run()
        got = _out(sc)
        assert np.array_equal(got["valid"], y["want"]["valid"]), "validity does not change"
        assert not np.array_equal(_bits(got["points"]), _bits(y["want"]["points"]))


def test_three_views_behind_an_untouched_slot():
    rig, win = "radial", "full"
    caps = [SC.scene(rig, win, plane)["cap"] for plane in SC.VIEW_PLANES]
    with _open(rig, win, keep=True, max_views=4) as sc:
        for v, cap in enumerate(caps, start=1):
            _load(sc, cap, view=v)
            _stages345(sc, v)
        assert sc.triangulate_subpixel(1, 3, want_counts=False) is None
        want = {v: _out(sc, v) for v in (1, 2, 3)}
    for v in want:
        _sane(want[v], ("view", v))
    assert len({w["points"].tobytes() for w in want.values()}) == 3, "the views must differ"
    with _open(rig, win, max_views=4) as sc:
        for v, cap in enumerate(caps, start=1):
            _load(sc, cap, view=v)
        slot0 = sc.points(0)
        sc.run(1, 3)
        for v in want:
            _same(_out(sc, v), want[v], ("run(1, 3)", v))
        after = _out(sc, 0)
        assert np.array_equal(after["valid"], slot0[1]) and np.array_equal(_bits(after["points"]), _bits(slot0[0])) and np.isnan(after["residual"]).all()
        sc.run(2, 1)
        for v in want:
            _same(_out(sc, v), want[v], ("after run(2, 1)", v))
        assert sc.launch_counts() == (2, 0)
        # sl3d_run_timed agrees with sl3d_run
        assert sc.run_timed(1, 3) > 0
        for v in want:
            _same(_out(sc, v), want[v], ("run_timed(1, 3)", v))


# (W, H, PW, PH, n_fringe, n_gray (v, h), fringe widths (v, h), noise): 90 columns are a 96-column pitch, the last quad of a row half outside
CONFIGS = {
    "four_step": (4, (5, 5), (4, 4), 0),
    "five_step": (5, (5, 5), (4, 4), 0),
    "unequal_axes": (3, (7, 5), (4, 4), 0),
    "no_gray_vertical": (3, (0, 5), (128, 4), 0),
    "no_gray_horizontal": (3, (5, 0), (4, 96), 0),
    "noise": (3, (5, 5), (4, 4), 2),
}


@pytest.mark.parametrize("name", CONFIGS)
def test_configurations(name):
    F, (nv, nh), (fv, fh), noise = CONFIGS[name]
    W, H, PW, PH = 90, 60, 128, 96
    syn = pkg("synth")
    cap = syn.make_capture(W, H, PW, PH, nv, nh, fv, fh, n_fringe=F, noise=noise)
    cal = syn.cal_tuple(cap["cal"])
    outs, xy = {}, {}
    for kind in ("staged", "timed", "unanchored"):
        with pkg("scanner").Scanner(W, H, PW, PH, nv, nh, fv, fh, n_fringe=F, keep_stages=kind != "timed", subpixel=True, anchored=kind != "unanchored") as sc:
            sc.set_calibration(*cal)
            _frames(sc, cap)
            sc.set_mask(cap["mask"])
            if kind == "timed":
                sc.run()
                assert sc.last_fused_kernel_name() == NAME
            else:
                _stages345(sc)
                if kind == "staged":
                    inp = _inputs(sc)
                xy[kind] = sc.correspondences_subpixel()
                assert sc.triangulate_subpixel(want_counts=False) is None
            outs[kind] = _out(sc)
    _sane(outs["staged"], name, some_valid=F != 5)
    _same(outs["timed"], outs["staged"], name)
    assert np.array_equal(outs["unanchored"]["valid"], outs["staged"]["valid"])
    if F == 5:
        got = outs["timed"]
        assert (got["valid"] == 0).all() and np.isnan(got["points"]).all() and np.isnan(got["residual"]).all()
        return
    v = outs["staged"]["valid"] == 1
    assert v.sum() > 1000, name
    want_xy = _restate_xy(inp, (0, 0), fw=(fv, fh), n_fringe=F, n_gray=(nv, nh), full=(W, H))
    nan = np.isnan(want_xy)
    assert np.array_equal(np.isnan(xy["staged"]), nan) and np.array_equal(_bits(xy["staged"])[~nan], _bits(want_xy)[~nan])
    for axis, n in enumerate((nv, nh)):
        same = np.array_equal(_bits(xy["staged"][..., axis]), _bits(xy["unanchored"][..., axis]))
        assert same == (n == 0), (name, axis, "an axis without Gray planes keeps the unanchored coordinate, an axis with them does not")


@pytest.mark.parametrize("eager", [False, True])
def test_lasso_mask(eager):
    s = SC.scene("plain", "full")
    W, H = SC.FULL
    lasso = np.zeros((H, W), np.uint8)
    lasso[67:174, 91:230] = 1                                     # about a fifth of the frame, edges on no multiple of 4
    with _open("plain", "full", keep=True) as sc:
        _load(sc, s["cap"], mask=lasso)
        _stages345(sc)
        sc.triangulate_subpixel(want_counts=False)
        want = _out(sc)
    _sane(want, "lasso")
    assert 0 < (want["valid"] == 1).sum() <= lasso.sum() and not want["valid"][lasso == 0].any()
    with _open("plain", "full", eager_mask=eager) as sc:
        _frames(sc, s["cap"])
        sc.set_mask(lasso)                                         # set and run at once on one view
        sc.run()
        _same(_out(sc), want, ("lasso", eager))
        assert sc.last_fused_kernel_name() == NAME


def test_process_views_equals_run():
    rig, win = "radial", "window"
    caps = [SC.scene(rig, win, plane)["cap"] for plane in SC.VIEW_PLANES[:2]]
    with _open(rig, win, max_views=2) as sc:
        for v, cap in enumerate(caps):
            _load(sc, cap, view=v)
        sc.run(0, 2)
        want = [_out(sc, v) for v in range(2)]
        assert len({w["points"].tobytes() for w in want}) == 2
    _same(want[0], _staged(rig, win)["want"], "view 0 is the scene's")
    with _open(rig, win, max_views=2) as sc:
        for v in range(2):
            sc.set_mask(pkg("synth").default_mask(*SC.FULL), view=v)
        frames = np.stack([np.stack(cap["planes_v"] + cap["planes_h"]) for cap in caps])
        xyz, valid = sc.process_views(frames)
        for v in range(2):
            assert np.array_equal(valid[v], want[v]["valid"]) and np.array_equal(_bits(xyz[v]), _bits(want[v]["points"])), v
            _same(_out(sc, v), want[v], ("the slot's planes", v))
        assert sc.last_fused_kernel_name() == NAME


# ---- 4. a group ----------------------------------------------------------------------------------------------------------------------------
def test_group_of_three_stripes():
    S = pkg("scanner")
    s = SC.scene("plain", "full")
    single = _staged("plain", "full")["want"]
    W, H = SC.FULL
    with S.Group(W, H, SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW, devices=[0, 0, 0], flags=S.SL3D_FLAG_SUBPIXEL | S.SL3D_FLAG_ANCHOR_PERIODS) as g:
        assert len(g.stripes()) == 3
        g.set_calibration(*s["cal"])
        _load(g, s["cap"])
        g.run()
        xyz, valid = g.download_points()
        assert np.array_equal(valid[0], single["valid"]) and np.array_equal(_bits(xyz[0]), _bits(single["points"])), "download_points"
        g.gather()
        xyz, valid = g.points()
        assert np.array_equal(valid, single["valid"]) and np.array_equal(_bits(xyz), _bits(single["points"])), "gather + get_points"
        with pytest.raises(S.Sl3dError):
            g.run_clouds()
        g.synchronize()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    s = SC.scene("plain", "window")
    y = _staged("plain", "window")
    with _open("plain", "window", keep=True) as sc:             # sl3d_repair_periods on an anchored KEEP_STAGES context
        L, h = sc.L, sc._h
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate_subpixel(want_counts=False)
        before, planes = _out(sc), _inputs(sc)
        _same(before, y["want"], "the run before the refusals")
        for axis in (0, 1):
            assert L.sl3d_repair_periods(h, 0, axis, 4, None) == -5
            text = L.sl3d_last_error(h)
            assert b"SL3D_FLAG_ANCHOR_PERIODS" in text and b"repair_periods" in text and b"without SL3D_FLAG_ANCHOR_PERIODS" in text, text
        assert L.sl3d_repair_periods(h, 0, 2, 4, None) == -1, "the arguments are checked first"
        assert L.sl3d_run_clouds(h, 0, 1) == -4                 # (the timed mode's call, as on every KEEP_STAGES context)
        after = _inputs(sc)
        for k in ("w", "code", "unw", "valid_axis"):
            for a in (0, 1):
                assert np.array_equal(_bits(after[k][a]), _bits(planes[k][a])), (k, a)
        assert np.array_equal(after["valid"], planes["valid"]) and np.array_equal(after["c_p_map"], planes["c_p_map"])
        _same(_out(sc), before, "after the refusals")
    with _open("plain", "window") as sc:                        # the timed context
        L, h = sc.L, sc._h
        _load(sc, s["cap"])
        sc.run()
        before = _out(sc)
        _same(before, y["want"], "the run before the refusals")
        assert L.sl3d_run_clouds(h, 0, 1) == -5 and b"sl3d_compact_views" in L.sl3d_last_error(h) and b"SL3D_FLAG_SUBPIXEL" in L.sl3d_last_error(h)
        assert L.sl3d_repair_periods(h, 0, 0, 4, None) == -4 and b"KEEP_STAGES" in L.sl3d_last_error(h)
        xy = np.zeros((s["H"], s["W"], 2))
        assert L.sl3d_get_correspondences_subpixel(h, 0, xy.ctypes.data, s["W"]) == -4
        assert L.sl3d_triangulate_subpixel(h, 0, 1, INF, None) == -4
        with pytest.raises(pkg("scanner").Sl3dError):
            sc.fused_kernel_name(1, clouds=True)
        _same(_out(sc), before, "after the refusals")


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------------
def test_accuracy_of_the_device_output():
    """The bars of tests/test_anchor_arith.py (b) on the device's own planes."""
    s, y = SC.scene("plain", "full"), _staged("plain", "full")
    cap = s["cap"]
    with _open("plain", "full", keep=True) as sc:
        _load(sc, s["cap"])
        sc.run()
        xy, ip, res, valid = sc.correspondences_subpixel(), sc.intersection_points(), sc.residuals(), sc.valid_map()
    assert np.array_equal(_bits(xy), _bits(y["xy"])) and np.array_equal(valid, y["inp"]["valid"])
    with _open("plain", "full", keep=True, anchored=False) as sc:
        _load(sc, s["cap"])
        sc.run()
        plain_xy, plain_ip, plain_res = sc.correspondences_subpixel(), sc.intersection_points(), sc.residuals()
        good = SC.good_pixels(cap, sc.c_p_map(), sc.valid_map())
    bar = SC.plane_rms(plain_ip, good)
    share0, _, med0, _ = accuracy(cap, valid, plain_xy, plain_ip, plain_res)
    share, rms, med, n = accuracy(cap, valid, xy, ip, res)
    print(f"within 0.5 px on both axes: unflagged {share0:.4%}, anchored {share:.4%} ({n} pixels); RMS to the plane: sub-pixel over good_pixels {bar:.4f} mm, "
          f"anchored over S {rms:.4f} mm, ratio {rms / bar:.3f}; median residual: unflagged {med0:.4f} px, anchored {med:.4f} px")
    assert share >= 0.995
    assert rms <= 0.1 * bar
    assert med <= 0.01


# ---- 7. the kernel names -------------------------------------------------------------------------------------------------------------------
def test_kernel_names_tell_the_instantiations_apart():
    s = SC.scene("plain", "window")
    names = {}
    for anchored in (False, True):
        with _open("plain", "window", anchored=anchored) as sc:
            _load(sc, s["cap"])
            sc.run()
            names[anchored] = (sc.fused_kernel_name(1), sc.last_fused_kernel_name())
    assert names[True] == (NAME, NAME)
    assert names[False] == ("sl3d::k_subpixel_fused<false>",) * 2
