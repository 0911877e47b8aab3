"""GPU tests (-m gpu) of sl3d_triangulate_subpixel / sl3d_get_residuals / sl3d_get_correspondences_subpixel on the captures of
tests/subpixel_cases.py: what k_subpixel leaves in the dense planes and the residual plane against the NumPy restatement of the
definition (tests/subpixel_reference.py) applied to the very planes downloaded before the call -- points and intersection_points within
the project's 1e-5 bar, residuals within 1e-6 * ref + 1e-7 px (the evaluation orders differ by ~1e-12 px, the float cast is 6e-8
relative), NaN and valid patterns equal.  320 x 240 is 300 blocks of k_subpixel (256 pixels of the pitched plane each); the 70 x 9
window at (37, 5) is three blocks, the last one partial, whose rows carry 10 padding columns of the pitch.  Then the coordinates bit for bit, the views of
one launch, the rejection from the downloaded residual plane, the consumers of the dense result, the accuracy the feature is for, the
route behind the period repair and behind sl3d_run, and the refusals."""
import ctypes

import numpy as np
import pytest

from conftest import assert_points_close, pkg

import mesh_reference as MR
import period_cases as PC
import period_repair_reference as PR
import subpixel_cases as SC
import subpixel_reference as SR

pytestmark = pytest.mark.gpu

INF = float("inf")


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _open(rig, win, max_views=1, keep=True, calibrate=True):
    s = SC.scene(rig, win)
    sc = pkg("scanner").Scanner(s["W"], s["H"], SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW, keep_stages=keep, full_size=SC.FULL, origin=s["origin"],
                                max_views=max_views)
    if calibrate:
        sc.set_calibration(*s["cal"])
    return sc


def _load(sc, cap, view=0):
    sc.set_mask(pkg("synth").default_mask(*SC.FULL), view=view)
    sc.set_frames(0, cap["planes_v"], view=view)
    sc.set_frames(1, cap["planes_h"], view=view)


def _stages345(sc, view=0):
    for a in (0, 1):
        sc.compute_wrapped_phase(a, view)
    for a in (0, 1):
        sc.unwrap_phase(a, view)
    sc.compute_c_p_map(view)


def _inputs(sc, view=0):
    """What the call reads, downloaded before it."""
    return dict(unw=(sc.unwrapped_phase(0, view), sc.unwrapped_phase(1, view)), valid_axis=(sc.valid_map(0, view), sc.valid_map(1, view)),
                valid=sc.valid_map(view=view), A=sc.projection_matrices())


def _restate(inp, cal, origin, fw=(SC.FW, SC.FW), max_residual=INF):
    xy = SR.correspondences(*inp["unw"], *inp["valid_axis"], *fw)
    return SR.triangulate(xy, inp["valid"], cal, *inp["A"], origin, max_residual)


def _outputs(sc, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid, ipoints=sc.intersection_points(view), residual=sc.residuals(view))


def _same_bits(a, b, what):
    for k in ("points", "valid", "ipoints", "residual"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _check(got, want, what):
    """The device's planes of one view against the restatement's; returns the maxima observed."""
    assert np.array_equal(got["valid"], want["valid"]), (what, "valid map", int((got["valid"] != want["valid"]).sum()))
    v = want["valid"] == 1
    assert v.sum() > 0
    assert np.array_equal(np.isnan(got["points"]).any(-1), ~v) and np.array_equal(np.isnan(got["points"]).all(-1), ~v), (what, "NaN pattern of points")
    assert (got["ipoints"][~v] == 0).all(), (what, "intersection_points of a pixel that is not valid")
    e_f = assert_points_close(got["points"], want["ipoints"], v)
    e_d = assert_points_close(got["ipoints"], want["ipoints"], v)
    assert np.array_equal(_bits(got["points"][v]), _bits(got["ipoints"][v].astype(np.float32))), (what, "points is not the float cast of intersection_points")
    t = ~np.isnan(want["residual"])
    assert np.array_equal(~np.isnan(got["residual"]), t), (what, "NaN pattern of the residuals")
    ref = want["residual"][t].astype(np.float64)
    err = np.abs(got["residual"][t].astype(np.float64) - ref)
    k = int(np.argmax(err - 1e-6 * ref))
    print(f"{what}: points {e_f:.2e} rel, intersection_points {e_d:.2e} rel, residuals max |diff| {err.max():.2e} px (at {ref[k]:.3g} px: {err[k]:.2e})")
    assert (err <= 1e-6 * ref + 1e-7).all(), (what, float(err[k]), float(ref[k]))
    return e_f, e_d, float(err.max())


# ---- 1. the device against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_device_equals_the_restatement(rig, win):
    s = SC.scene(rig, win)
    thr = SC.THRESHOLDS[(rig, win)]
    with _open(rig, win) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        inp = _inputs(sc)
        # (the planes are the oracle's: what tests/test_subpixel_arith.py asserts of the thresholds holds here)
        o = SC.oracle_scan(rig, win)
        assert np.array_equal(inp["valid"], o["valid"]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(inp["unw"], o["unw"]))
        cp = sc.c_p_map()
        want = _restate(inp, s["cal"], s["origin"])
        counts = sc.triangulate_subpixel()
        assert counts == [want["counts"]] and counts[0][1] == 0
        _check(_outputs(sc), want, (rig, win, "no rejection"))
        assert np.array_equal(sc.c_p_map(), cp) and np.array_equal(sc.valid_map(0), inp["valid_axis"][0]) and np.array_equal(sc.valid_map(1), inp["valid_axis"][1])
        assert all(np.array_equal(_bits(sc.unwrapped_phase(a)), _bits(inp["unw"][a])) for a in (0, 1))
        # with a threshold: a second call over the planes the first one left (nothing was rejected: the same inputs)
        want = _restate(inp, s["cal"], s["origin"], max_residual=thr)
        counts = sc.triangulate_subpixel(max_residual=thr)
        assert counts == [want["counts"]] and 0 < counts[0][1] < counts[0][0]
        _check(_outputs(sc), want, (rig, win, "threshold", thr))


# ---- 2. the coordinates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", SC.WINDOWS)
def test_coordinates_are_the_arguments_of_stage_5_bit_for_bit(win):
    s = SC.scene("plain", win)
    with _open("plain", win, calibrate=False) as sc:          # (no calibration, no stage 5 needed)
        _load(sc, s["cap"])
        for a in (0, 1):
            sc.compute_wrapped_phase(a)
        for a in (0, 1):
            sc.unwrap_phase(a)
        inp = dict(unw=(sc.unwrapped_phase(0), sc.unwrapped_phase(1)), valid_axis=(sc.valid_map(0), sc.valid_map(1)))
        xy = sc.correspondences_subpixel()
        want = SR.correspondences(*inp["unw"], *inp["valid_axis"], SC.FW, SC.FW)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(xy), nan) and nan.sum() < nan.size and (nan.any() or win != "full")   # (the window has no invalid pixel)
        assert np.array_equal(_bits(xy)[~nan], _bits(want)[~nan])
        sc.compute_c_p_map()
        v = sc.valid_map() == 1
        assert v.sum() > 500 and np.array_equal(np.rint(xy[v]).astype(np.int64), sc.c_p_map()[v])
        # a caller's stride, the rows' tails untouched
        wide = np.full((s["H"], s["W"] + 3, 2), -7.0)
        sc._chk(sc.L.sl3d_get_correspondences_subpixel(sc._h, 0, wide.ctypes.data, s["W"] + 3), "sl3d_get_correspondences_subpixel")
        assert np.array_equal(_bits(wide[:, :s["W"]]), _bits(xy)) and (wide[:, s["W"]:] == -7.0).all()


# ---- 3. the views of one launch -----------------------------------------------------------------------------------------------------------
def test_views_of_one_launch_and_the_views_outside_it():
    caps = [SC.scene("radial", "full", plane)["cap"] for plane in SC.VIEW_PLANES]
    thr = SC.THRESHOLDS[("radial", "full")]
    with _open("radial", "full", max_views=3) as sc:
        for v, cap in enumerate(caps):
            _load(sc, cap, view=v)
            _stages345(sc, v)
        assert len({sc.unwrapped_phase(0, v).tobytes() for v in range(3)}) == 3, "the views must differ"
        assert sc.triangulate_subpixel(0, 1, want_counts=False) is None
        assert np.isnan(sc.residuals(1)).all(), "a view no call has run over: NaN"
        view0 = _outputs(sc, 0)
        inp = [_inputs(sc, v) for v in range(3)]
        counts = sc.triangulate_subpixel(1, 2, max_residual=thr)
        _same_bits(_outputs(sc, 0), view0, "view 0 after a call over views 1, 2")
        batch = [_outputs(sc, v) for v in (1, 2)]
        s = SC.scene("radial", "full")
        for k, v in enumerate((1, 2)):
            want = _restate(inp[v], s["cal"], s["origin"], max_residual=thr)
            res = want["residual"][inp[v]["valid"] == 1].astype(np.float64)
            assert (np.abs(res - thr) > 1e-4 * thr).all(), "the threshold must stay clear of ties in this view too"
            assert counts[k] == want["counts"] and counts[k][1] > 0
            _check(batch[k], want, ("view", v, "of a launch over two"))
        assert counts[0] != counts[1]
        # the same views, one call each
        for k, v in enumerate((1, 2)):
            sc.compute_c_p_map(v)
            assert sc.triangulate_subpixel(v, 1, max_residual=thr) == [counts[k]]
            _same_bits(_outputs(sc, v), batch[k], ("view", v, "alone"))
        _same_bits(_outputs(sc, 0), view0, "view 0 at the end")


# ---- 4. the rejection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", [("plain", "full"), ("tangential", "window")])
def test_rejection_is_reproducible_from_the_downloaded_residuals(rig, win):
    s = SC.scene(rig, win)
    thr = SC.THRESHOLDS[(rig, win)]
    with _open(rig, win) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate()
        xyz0, valid0 = sc.points()
        ip0 = sc.intersection_points()
        (n_tri, n_rej), = sc.triangulate_subpixel(max_residual=thr)
        out = _outputs(sc)
        with np.errstate(invalid="ignore"):
            keep = (valid0 == 1) & (out["residual"].astype(np.float64) <= thr)
        assert np.array_equal(out["valid"] == 1, keep)
        assert n_tri == int((valid0 == 1).sum()) and n_rej == int(((valid0 == 1) & ~keep).sum()) and n_rej > 0
        assert np.array_equal(~np.isnan(out["residual"]), valid0 == 1), "a rejected pixel keeps its residual"
        gone = (valid0 == 1) & ~keep
        assert np.isnan(out["points"][gone]).all() and (out["ipoints"][gone] == 0).all()
        assert (out["residual"][gone] > thr).all() and (out["residual"][keep] <= thr).all()
        # a second call sees the rejections: it triangulates the pixels that are left, and rejects none of them
        assert sc.triangulate_subpixel(max_residual=thr) == [(n_tri - n_rej, 0)]
        assert np.array_equal(sc.valid_map() == 1, keep)
        # stage 5 undoes them, stage 7 restores the integer result
        sc.compute_c_p_map()
        sc.triangulate()
        xyz1, valid1 = sc.points()
        assert np.array_equal(valid1, valid0) and np.array_equal(_bits(xyz1), _bits(xyz0)) and np.array_equal(_bits(sc.intersection_points()), _bits(ip0))


# ---- 5. downstream ------------------------------------------------------------------------------------------------------------------------
def test_the_consumers_of_the_dense_result_see_the_subpixel_scan():
    s = SC.scene("plain", "full")
    with _open("plain", "full") as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate()
        integer = sc.cloud()
        sc.triangulate_subpixel(max_residual=SC.THRESHOLDS[("plain", "full")])
        xyz, valid = sc.points()
        cloud = sc.cloud()
        assert np.array_equal(_bits(cloud), _bits(xyz[valid == 1])) and len(cloud) < len(integer)
        assert not np.array_equal(cloud[:100], integer[:100])
        step = np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)
        median_edge = float(np.nanmedian(step))
        n_faces = []
        for max_edge in (INF, 1.25 * median_edge):
            verts, faces = sc.mesh(max_edge)
            want_v, want_f = MR.np_mesh(xyz, valid, max_edge)
            assert np.array_equal(_bits(verts), _bits(want_v)) and np.array_equal(faces, want_f), max_edge
            n_faces.append(len(faces))
        assert n_faces[0] > 100000 and 0 < n_faces[1] < n_faces[0], n_faces


# ---- 6. what the feature is for -----------------------------------------------------------------------------------------------------------
def test_plane_accuracy_of_the_device_output():
    s = SC.scene("plain", "full")
    with _open("plain", "full") as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate()
        integer = sc.intersection_points()
        good = SC.good_pixels(s["cap"], sc.c_p_map(), sc.valid_map())
        sc.triangulate_subpixel()
        sub, res = sc.intersection_points(), sc.residuals()
    assert good.sum() > 60000
    a, b = SC.plane_rms(integer, good), SC.plane_rms(sub, good)
    print(f"RMS distance to the plane: integer {a:.4f} mm, sub-pixel {b:.4f} mm, ratio {b / a:.3f}; residual on those pixels: median "
          f"{np.median(res[good]):.4f} px, max {res[good].max():.4f} px")
    assert b <= 0.5 * a


# ---- 7. behind the period repair, behind sl3d_run -----------------------------------------------------------------------------------------
def test_after_the_period_repair():
    case = PC.make_case("plain_v", 2)
    syn = pkg("synth")
    cal = syn.cal_tuple(syn.synth_rig(case["full"][0], case["full"][1], case["PW"], case["PH"]))
    with pkg("scanner").Scanner(case["W"], case["H"], case["PW"], case["PH"], case["N"], case["N"], PC.FW, PC.FW, keep_stages=True) as sc:
        sc.set_calibration(*cal)
        sc.set_mask(case["mask"])
        sc.set_frames(0, case["planes_v"])
        sc.set_frames(1, case["planes_h"])
        for a in (0, 1):
            sc.compute_wrapped_phase(a)
        for a in (0, 1):
            sc.unwrap_phase(a)
        raw = sc.unwrapped_phase(0)
        assert sc.repair_periods(0, 4)[0] > 0 and sc.repair_periods(1, 4)[0] == 0
        sc.compute_c_p_map()
        inp = _inputs(sc)
        assert not np.array_equal(_bits(inp["unw"][0]), _bits(raw))
        inside = PR.interior(inp["valid_axis"][0], 0, 4) & (inp["valid"] == 1)
        want = _restate(inp, cal, (0, 0), fw=(PC.FW, PC.FW))
        assert sc.triangulate_subpixel() == [want["counts"]]
        got = _outputs(sc)
        _check(got, want, "after the repair")
        # the repaired pixels are one fringe width away from where the unrepaired phase puts them
        moved = inside & (_bits(inp["unw"][0]) != _bits(raw))
        assert moved.sum() > 10
        assert np.allclose(np.abs(SR.continuous(inp["unw"][0], PC.FW) - SR.continuous(raw, PC.FW))[moved], PC.FW, atol=1e-3)


def test_after_the_fused_launch_of_a_keep_context():
    s = SC.scene("tangential", "full")
    with _open("tangential", "full") as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate_subpixel()
        staged = _outputs(sc)
        sc.run()
        want = _restate(_inputs(sc), s["cal"], s["origin"])
        sc.triangulate_subpixel()
        got = _outputs(sc)
        _check(got, want, "behind sl3d_run")
        _same_bits(got, staged, "behind sl3d_run against the staged route")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    S = pkg("scanner")
    s = SC.scene("plain", "window")
    counts = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    buf = np.zeros((s["H"], s["W"]), np.float32)
    with _open("plain", "window", max_views=2) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate()
        L, h = sc.L, sc._h
        assert L.sl3d_get_residuals(h, 0, buf.ctypes.data, s["W"]) == -4 and b"sl3d_triangulate_subpixel" in L.sl3d_last_error(h)
        with pytest.raises(S.Sl3dError):
            sc.residuals()
        xyz0, valid0 = sc.points()
        ip0 = sc.intersection_points()

        def unchanged(what):
            xyz, valid = sc.points()
            assert np.array_equal(valid, valid0) and np.array_equal(_bits(xyz), _bits(xyz0)) and np.array_equal(_bits(sc.intersection_points()), _bits(ip0)), what
            assert tuple(counts) == (7, 7, 7, 7), what

        for bad in (float("nan"), 0.0, -0.0, -1.0, -INF):
            assert L.sl3d_triangulate_subpixel(h, 0, 1, bad, counts) == -1 and b"max_residual" in L.sl3d_last_error(h), bad
        unchanged("max_residual")
        for first, n in ((-1, 1), (2, 1), (1, 2), (0, 0), (0, -1), (0, 3)):
            assert L.sl3d_triangulate_subpixel(h, first, n, INF, counts) == -1 and b"view" in L.sl3d_last_error(h), (first, n)
        assert L.sl3d_triangulate_subpixel(None, 0, 1, INF, counts) == -1
        unchanged("views")
        assert L.sl3d_get_residuals(h, 0, buf.ctypes.data, s["W"]) == -4, "a refused call is no first call"
        with pytest.raises(S.Sl3dError):
            sc.triangulate_subpixel(max_residual=0.0)
        # the getters' own arguments
        assert sc.triangulate_subpixel(want_counts=False) is None            # counts == NULL: asynchronous, the same result
        assert L.sl3d_get_residuals(h, 2, buf.ctypes.data, s["W"]) == -1 and L.sl3d_get_residuals(h, 0, None, s["W"]) == -1
        assert L.sl3d_get_residuals(h, 0, buf.ctypes.data, s["W"] - 1) == -1
        xy = np.zeros((s["H"], s["W"], 2))
        assert L.sl3d_get_correspondences_subpixel(h, -1, xy.ctypes.data, s["W"]) == -1 and L.sl3d_get_correspondences_subpixel(h, 0, None, s["W"]) == -1
        assert L.sl3d_get_correspondences_subpixel(h, 0, xy.ctypes.data, s["W"] - 1) == -1
        assert np.isfinite(sc.residuals()[valid0 == 1]).all() and np.isnan(sc.residuals(1)).all()
    with _open("plain", "window", keep=False) as sc:                          # no SL3D_FLAG_KEEP_STAGES
        _load(sc, s["cap"])
        sc.run()
        xyz0, valid0 = sc.points()
        assert sc.L.sl3d_triangulate_subpixel(sc._h, 0, 1, INF, counts) == -4 and b"KEEP_STAGES" in sc.L.sl3d_last_error(sc._h)
        assert sc.L.sl3d_get_correspondences_subpixel(sc._h, 0, xy.ctypes.data, s["W"]) == -4
        xyz, valid = sc.points()
        assert np.array_equal(valid, valid0) and np.array_equal(_bits(xyz), _bits(xyz0)) and tuple(counts) == (7, 7, 7, 7)
    with _open("plain", "window", calibrate=False) as sc:                     # no calibration
        _load(sc, s["cap"])
        _stages345(sc)
        assert sc.L.sl3d_triangulate_subpixel(sc._h, 0, 1, INF, counts) == -4 and b"sl3d_set_calibration" in sc.L.sl3d_last_error(sc._h)
        assert tuple(counts) == (7, 7, 7, 7)
