"""GPU tests (-m gpu) of SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL on the captures of tests/one_axis_cases.py (320 x 240
full frame: 75 blocks of the timed kernel; the 70 x 9 window at (37, 5): one partial block, 10 padding columns per row; unequal axes, a rig
per coded axis).  Only the frames of the coded axis are ever set, unless a test says otherwise.

1. The staged route (KEEP_STAGES | SUBPIXEL | ONLY_*) against the NumPy restatement (tests/one_axis_reference.py) applied to the planes
   downloaded before stage 5: valid map, c_p_map and the coordinates bit for bit, NaN patterns, points and intersection_points at the
   project's 1e-5 bar, points the float cast of intersection_points; with and without ANCHOR_PERIODS, and once with four fringes.
2. The timed context: sl3d_run equals the staged route bit for bit on every pixel of the window.  3. Three views behind an untouched slot.
4. Axis b is never read.  5. Modulated masks.  6. A group of three stripes.  7. Refusals change nothing.  8. The kernel names.
9. The accuracy of the device output against the two-axis device scan."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_points_close, pkg

import one_axis_cases as OC
import one_axis_reference as OR
import subpixel_cases as SC

pytestmark = pytest.mark.gpu

INF = float("inf")
NAMES = {(0, False): "sl3d::k_one_axis<0, false>", (0, True): "sl3d::k_one_axis<0, true>", (1, False): "sl3d::k_one_axis<1, false>",
         (1, True): "sl3d::k_one_axis<1, true>"}
CASES = [(axis, win, anchored) for axis, win in OC.SCENES for anchored in (False, True)]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _open(axis, win, *, keep=False, anchored=False, max_views=1, n_fringe=3, only=True, rig_axis=None):
    s = OC.scene(axis if rig_axis is None else rig_axis, win)
    sc = pkg("scanner").Scanner(s["W"], s["H"], OC.PW, OC.PH, OC.N[0], OC.N[1], OC.FW[0], OC.FW[1], n_fringe=n_fringe, keep_stages=keep, full_size=OC.FULL,
                                origin=s["origin"], max_views=max_views, subpixel=True, anchored=anchored, only_axis=axis if only else None)
    sc.set_calibration(*s["cal"])
    return sc


def _planes(cap, axis):
    return cap["planes_v"] if axis == 0 else cap["planes_h"]


def _load(sc, cap, axis, view=0, mask=None):
    """The frames of the coded axis alone, and the default mask."""
    sc.set_frames(axis, _planes(cap, axis), view=view)
    sc.set_mask(pkg("synth").default_mask(*OC.FULL) if mask is None else mask, view=view)


def _stages34(sc, axis, view=0):
    sc.compute_wrapped_phase(axis, view)
    sc.unwrap_phase(axis, view)


def _inputs(sc, axis, view=0):
    """What stage 5 and the solve read, downloaded before them."""
    return dict(w=sc.wrapped_phase(axis, view), code=sc.code(axis, view), unw=sc.unwrapped_phase(axis, view), sel=sc.valid_map(axis, view), A=sc.projection_matrices())


def _out(sc, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid)


def _same(got, want, what):
    for k in ("valid", "points"):
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _sane(want, what):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1} and v.any(), what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["points"]).all(-1), ~v), what


@functools.lru_cache(maxsize=None)
def _staged(axis, win, anchored, n_fringe=3):
    """Per case, computed once and left unchanged, on a KEEP_STAGES | SUBPIXEL | ONLY_* context: the planes before stage 5, what stage 5 and
    sl3d_triangulate_subpixel(+inf) leave, and the coordinates -- the yardstick of the timed context."""
    cap = OC.scene(axis, win, n_fringe=n_fringe)["cap"]
    with _open(axis, win, keep=True, anchored=anchored, n_fringe=n_fringe) as sc:
        _load(sc, cap, axis)
        _stages34(sc, axis)
        inp = _inputs(sc, axis)
        sc.compute_c_p_map()
        valid5, cp = sc.valid_map(), sc.c_p_map()
        xy = sc.correspondences_subpixel()
        counts = sc.triangulate_subpixel()
        want = _out(sc)
        ip = sc.intersection_points()
        after = dict(valid=sc.valid_map(), c_p_map=sc.c_p_map(), unw=sc.unwrapped_phase(axis), w=sc.wrapped_phase(axis), code=sc.code(axis))
    _sane(want, (axis, win, anchored))
    return dict(inp=inp, valid5=valid5, c_p_map=cp, xy=xy, counts=counts, want=want, ipoints=ip, after=after)


def _restate(axis, win, anchored, inp, n_fringe=3):
    s = OC.scene(axis, win, n_fringe=n_fringe)
    return OR.scan(inp["w"], inp["code"], inp["unw"], inp["sel"], s["cal"], *inp["A"], axis, OC.FW[axis], OC.EXTENT[axis], OC.N[axis], n_fringe, s["origin"], OC.FULL,
                   anchored)


# ---- 1. the staged route against the restatement -------------------------------------------------------------------------------------------
def _check_staged(axis, win, anchored, n_fringe=3):
    y = _staged(axis, win, anchored, n_fringe)
    want = _restate(axis, win, anchored, y["inp"], n_fringe)
    v = want["valid"] == 1
    assert v.sum() > 500
    assert np.array_equal(y["valid5"], want["valid"]) and np.array_equal(y["want"]["valid"], want["valid"]), "valid map"
    assert np.array_equal(y["c_p_map"], want["c_p_map"]), "c_p_map"
    assert (y["c_p_map"][..., 1 - axis][v] == -1).all() and (y["c_p_map"][~v] == 0).all() and (y["c_p_map"][..., axis][v] >= 0).all()
    nan = np.isnan(want["xy"])
    assert np.array_equal(np.isnan(y["xy"]), nan) and nan[..., 1 - axis].all() and not nan[..., axis].all(), "NaN pattern of the coordinates"
    assert np.array_equal(_bits(y["xy"])[~nan], _bits(want["xy"])[~nan]), int((_bits(y["xy"])[~nan] != _bits(want["xy"])[~nan]).sum())
    assert y["counts"] == [(int(v.sum()), 0)]
    assert np.array_equal(np.isnan(y["want"]["points"]).any(-1), ~v)
    e_f = assert_points_close(y["want"]["points"], want["ipoints"], v)
    e_d = assert_points_close(y["ipoints"], want["ipoints"], v)
    assert (y["ipoints"][~v] == 0).all()
    assert np.array_equal(_bits(y["want"]["points"][v]), _bits(y["ipoints"][v].astype(np.float32))), "points are the float cast of intersection_points"
    print(f"axis {axis}, {win}, anchored {anchored}, {n_fringe} fringes: {int(v.sum())} valid, points {e_f:.2e} rel, intersection_points {e_d:.2e} rel")
    # stage 5 and 7 leave the planes they read as they were
    for k in ("unw", "w", "code"):
        assert np.array_equal(_bits(y["after"][k]), _bits(y["inp"][k])), k
    assert np.array_equal(y["after"]["valid"], want["valid"]) and np.array_equal(y["after"]["c_p_map"], want["c_p_map"])
    return y, want


@pytest.mark.parametrize("axis,win,anchored", CASES)
def test_staged_route_equals_the_restatement(axis, win, anchored):
    y, want = _check_staged(axis, win, anchored)
    if anchored:
        plain = _staged(axis, win, False)
        v = want["valid"] == 1
        assert np.array_equal(plain["valid5"], y["valid5"]) and np.array_equal(plain["c_p_map"], y["c_p_map"]), "anchoring changes neither validity nor c_p_map"
        assert (y["xy"][..., axis][v] != plain["xy"][..., axis][v]).mean() > 0.9, "the anchored coordinates are not the unanchored ones"


@pytest.mark.parametrize("axis", [0, 1])
def test_staged_route_with_four_fringes(axis):
    _check_staged(axis, "window", True, n_fringe=4)


# ---- 2. the timed context ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,win,anchored", CASES)
def test_run_equals_the_staged_route(axis, win, anchored):
    cap, y = OC.scene(axis, win)["cap"], _staged(axis, win, anchored)
    name = NAMES[(axis, anchored)]
    with _open(axis, win, anchored=anchored) as sc:
        assert sc.fused_kernel_name(1) == name and sc.camera_table_bytes_per_pixel(1) == 0
        _load(sc, cap, axis)
        sc.run()
        _same(_out(sc), y["want"], (axis, win, anchored))
        assert sc.last_fused_kernel_name() == name and sc.launch_counts() == (1, 0)
    with _open(axis, win, keep=True, anchored=anchored) as sc:   # KEEP_STAGES: sl3d_run enqueues the staged route itself
        _load(sc, cap, axis)
        sc.run()
        _same(_out(sc), y["want"], (axis, win, anchored, "KEEP_STAGES"))
        assert np.array_equal(sc.c_p_map(), y["c_p_map"]) and np.array_equal(_bits(sc.intersection_points()), _bits(y["ipoints"]))
        assert np.array_equal(_bits(sc.correspondences_subpixel()), _bits(y["xy"]))


@pytest.mark.parametrize("axis", [0, 1])
def test_run_with_four_fringes(axis):
    cap, y = OC.scene(axis, "window", n_fringe=4)["cap"], _staged(axis, "window", True, 4)
    with _open(axis, "window", anchored=True, n_fringe=4) as sc:
        _load(sc, cap, axis)
        sc.run()
        _same(_out(sc), y["want"], (axis, "four fringes"))


# ---- 3. three views behind an untouched slot -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_three_views_behind_an_untouched_slot(axis):
    win = "full"
    caps = [OC.scene(axis, win, plane)["cap"] for plane in OC.VIEW_PLANES]
    want = {}
    for v, cap in enumerate(caps, start=1):                     # each view as a one-view launch
        with _open(axis, win, anchored=True) as sc:
            _load(sc, cap, axis)
            sc.run()
            want[v] = _out(sc)
        _sane(want[v], ("view", v))
    _same(want[1], _staged(axis, win, True)["want"], "view 1 is the scene's")
    assert len({w["points"].tobytes() for w in want.values()}) == 3, "the views must differ"
    with _open(axis, win, anchored=True, max_views=4) as sc:
        for v, cap in enumerate(caps, start=1):
            _load(sc, cap, axis, view=v)
        slot0 = sc.points(0)
        sc.run(1, 3)
        for v in want:
            _same(_out(sc, v), want[v], ("run(1, 3)", v))
        after = _out(sc, 0)
        assert np.array_equal(after["valid"], slot0[1]) and np.array_equal(_bits(after["points"]), _bits(slot0[0])), "slot 0 is untouched"
        assert sc.launch_counts() == (1, 0)
        assert sc.run_timed(1, 3) > 0                             # sl3d_run_timed agrees with sl3d_run
        for v in want:
            _same(_out(sc, v), want[v], ("run_timed(1, 3)", v))


# ---- 4. axis b is never read ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("keep", [False, True])
def test_the_other_axis_is_never_read(axis, keep):
    win, b = "window", 1 - axis
    s, y = OC.scene(axis, win), _staged(axis, win, True)
    n_b = 3 + 2 * OC.N[b]
    rng = np.random.default_rng(5)
    with _open(axis, win, keep=keep, anchored=True) as sc:
        _load(sc, s["cap"], axis)
        for fill in (np.full((n_b, s["H"], s["W"]), 0xAA, np.uint8), rng.integers(0, 256, (n_b, s["H"], s["W"]), dtype=np.uint8)):
            sc.set_frames(b, list(fill))
            sc.run()
            _same(_out(sc), y["want"], (axis, keep, int(fill[0, 0, 0])))
            assert all(np.array_equal(g, f) for g, f in zip(sc.frames(b), fill)), "the planes of axis b are as they were set"


@pytest.mark.parametrize("axis", [0, 1])
def test_process_views_uploads_the_coded_axis_alone(axis):
    win, b = "window", 1 - axis
    s, y = OC.scene(axis, win), _staged(axis, win, True)
    cap = s["cap"]
    n_b = 3 + 2 * OC.N[b]
    mark = [np.full((s["H"], s["W"]), 0x5C, np.uint8)] * n_b
    planes = [np.ascontiguousarray(p) for p in _planes(cap, axis)]
    mine = [p.ctypes.data for p in planes]
    order = mine + [None] * n_b if axis == 0 else [None] * n_b + mine                   # NULL for every plane of axis b
    assert len(order) == 6 + 2 * sum(OC.N)
    with _open(axis, win, anchored=True) as sc:
        sc.set_frames(b, mark)
        sc.set_mask(pkg("synth").default_mask(*OC.FULL))
        xyz, valid = np.empty((s["H"], s["W"], 3), np.float32), np.empty((s["H"], s["W"]), np.uint8)
        sc._call("process_views", 1, (ctypes.c_void_p * len(order))(*order), s["W"], xyz.ctypes.data, valid.ctypes.data)
        _same(dict(points=xyz, valid=valid), y["want"], (axis, "process_views"))
        _same(_out(sc), y["want"], (axis, "the slot's planes"))
        assert sc.last_fused_kernel_name() == NAMES[(axis, True)]
        assert all(np.array_equal(g, f) for g, f in zip(sc.frames(b), mark)), "sl3d_get_frames(axis b) is unchanged by it"
        assert all(np.array_equal(g, f) for g, f in zip(sc.frames(axis), planes)), "the planes of axis a went up"
        order[n_b if axis == 1 else 0] = None                      # a NULL plane of the coded axis is still refused
        assert sc.L.sl3d_process_views(sc._h, 1, (ctypes.c_void_p * len(order))(*order), s["W"], xyz.ctypes.data, valid.ctypes.data) == -1


# ---- 5. modulated masks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_modulated_masks_test_the_coded_axis_alone(axis):
    win, b, thr = "full", 1 - axis, 0.2
    s = OC.scene(0, win)                                         # (synth_rig's capture: part of the frame is not lit, its modulation is 0)
    cap = s["cap"]
    rng = np.random.default_rng(11)
    garbage = list(rng.integers(0, 256, (3 + 2 * OC.N[b], s["H"], s["W"]), dtype=np.uint8))
    with _open(axis, win, anchored=True, rig_axis=0) as sc:
        sc.set_frames(axis, _planes(cap, axis))
        gamma = sc.modulation(axis)
        with np.errstate(invalid="ignore"):
            select = (gamma.astype(np.float64) > thr).astype(np.uint8)
        assert min(int(select.sum()), int((select == 0).sum())) >= 1000, "both branches of the test are taken, each by a thousand pixels or more"
        sc.set_mask(select)
        sc.run()
        want = _out(sc)
        _sane(want, "selected by hand")
    with _open(axis, win, anchored=True, rig_axis=0) as sc:
        sc.set_frames(axis, _planes(cap, axis))
        sc.set_frames(b, garbage)
        sc.set_masks_modulated(thr)
        sc.run()
        _same(_out(sc), want, (axis, "set_masks_modulated"))
    with _open(axis, win, anchored=True, rig_axis=0) as sc:         # ... and with the frames of axis b absent
        sc.set_frames(axis, _planes(cap, axis))
        sc.set_masks_modulated(thr)
        sc.run()
        _same(_out(sc), want, (axis, "set_masks_modulated, no frames of axis b"))


# ---- 6. a group ----------------------------------------------------------------------------------------------------------------------------
def test_group_of_three_stripes():
    S = pkg("scanner")
    axis = 0
    s = OC.scene(axis, "full")
    single = _staged(axis, "full", True)["want"]
    W, H = OC.FULL
    with S.Group(W, H, OC.PW, OC.PH, OC.N[0], OC.N[1], OC.FW[0], OC.FW[1], devices=[0, 0, 0],
                 flags=S.SL3D_FLAG_SUBPIXEL | S.SL3D_FLAG_ANCHOR_PERIODS | S.SL3D_FLAG_ONLY_VERTICAL) as g:
        assert len(g.stripes()) == 3
        g.set_calibration(*s["cal"])
        _load(g, s["cap"], axis)
        g.run()
        xyz, valid = g.download_points()
        assert np.array_equal(valid[0], single["valid"]) and np.array_equal(_bits(xyz[0]), _bits(single["points"])), "download_points"
        g.gather()
        xyz, valid = g.points()
        assert np.array_equal(valid, single["valid"]) and np.array_equal(_bits(xyz), _bits(single["points"])), "gather + get_points"
        with pytest.raises(S.Sl3dError):
            g.run_clouds()
        g.synchronize()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_refusals_change_nothing(axis):
    win, b = "window", 1 - axis
    s, y = OC.scene(axis, win), _staged(axis, win, False)
    flag = b"SL3D_FLAG_ONLY_VERTICAL" if axis == 0 else b"SL3D_FLAG_ONLY_HORIZONTAL"
    Kc, dc, rc, tc, Kp, dp, rp, tp = s["cal"]
    skewed = Kp.copy()
    skewed[1] = 0.25
    bad = [(Kp, np.array(SC.RIGS["radial"])), (skewed, dp)]

    def stage_planes(sc):
        return [sc.wrapped_phase(a) for a in (0, 1)] + [sc.unwrapped_phase(a) for a in (0, 1)] + [sc.code(a) for a in (0, 1)] + [sc.valid_map(a) for a in (0, 1)] + \
               [sc.valid_map(), sc.c_p_map(), sc.intersection_points()]

    with _open(axis, win, keep=True) as sc:
        L, h = sc.L, sc._h
        _load(sc, s["cap"], axis)
        _stages34(sc, axis)
        sc.compute_c_p_map()
        sc.triangulate_subpixel(want_counts=False)
        before, planes = _out(sc), stage_planes(sc)
        _same(before, y["want"], "the run before the refusals")
        res = np.zeros((s["H"], s["W"]), np.float32)
        assert L.sl3d_get_residuals(h, 0, res.ctypes.data, s["W"]) == -5 and flag in L.sl3d_last_error(h) and not res.any()
        counts = (ctypes.c_uint32 * 2)(7, 7)
        assert L.sl3d_triangulate_subpixel(h, 0, 1, 1.0, counts) == -5 and b"+infinity" in L.sl3d_last_error(h) and list(counts) == [7, 7]
        assert L.sl3d_triangulate_subpixel(h, 0, 1, -1.0, None) == -1, "the arguments are checked first"
        assert L.sl3d_triangulate(h, 0) == -5 and b"sl3d_triangulate_subpixel" in L.sl3d_last_error(h)
        for call in (L.sl3d_compute_wrapped_phase, L.sl3d_unwrap_phase):
            assert call(h, 0, b) == -5 and flag in L.sl3d_last_error(h)
            assert call(h, 0, 2) == -1
        assert L.sl3d_repair_periods(h, 0, b, 4, None) == -5 and flag in L.sl3d_last_error(h)
        assert L.sl3d_run_clouds(h, 0, 1) == -4                 # (the timed mode's call, as on every KEEP_STAGES context)
        for K, d in bad:
            with pytest.raises(pkg("scanner").Sl3dError) as e:
                sc.set_calibration(Kc, dc, rc, tc, K, d, rp, tp)
            assert "unsupported" in str(e.value) and flag.decode() in str(e.value) and "a curve and not a line" in str(e.value)
        for got, want in zip(stage_planes(sc), planes):
            assert np.array_equal(_bits(got), _bits(want))
        _same(_out(sc), before, "after the refusals")
        sc.run()                                                  # the previous calibration still runs
        _same(_out(sc), before, "a run after the refused calibrations")
        for got, want in zip(stage_planes(sc), planes):
            assert np.array_equal(_bits(got), _bits(want))
    with _open(axis, win) as sc:                                # the timed context
        L, h = sc.L, sc._h
        _load(sc, s["cap"], axis)
        sc.run()
        before = _out(sc)
        _same(before, y["want"], "the run before the refusals")
        res = np.zeros((s["H"], s["W"]), np.float32)
        assert L.sl3d_get_residuals(h, 0, res.ctypes.data, s["W"]) == -5 and not res.any()
        assert L.sl3d_run_clouds(h, 0, 1) == -5 and b"sl3d_compact_views" in L.sl3d_last_error(h) and b"SL3D_FLAG_SUBPIXEL" in L.sl3d_last_error(h)
        assert L.sl3d_triangulate_subpixel(h, 0, 1, INF, None) == -4 and L.sl3d_triangulate(h, 0) == -4
        assert L.sl3d_compute_wrapped_phase(h, 0, b) == -4
        with pytest.raises(pkg("scanner").Sl3dError):
            sc.fused_kernel_name(1, clouds=True)
        for K, d in bad:
            with pytest.raises(pkg("scanner").Sl3dError):
                sc.set_calibration(Kc, dc, rc, tc, K, d, rp, tp)
        _same(_out(sc), before, "after the refusals")
        sc.run()
        _same(_out(sc), before, "a run after the refused calibrations")
    with _open(axis, win, only=False) as sc:                    # a two-axis context takes both calibrations as it always did
        for K, d in bad:
            sc.set_calibration(Kc, dc, rc, tc, K, d, rp, tp)


# ---- 8. the kernel names -------------------------------------------------------------------------------------------------------------------
def test_kernel_names_tell_the_instantiations_apart():
    names = {}
    for (axis, anchored), want in NAMES.items():
        with _open(axis, "window", anchored=anchored) as sc:
            _load(sc, OC.scene(axis, "window")["cap"], axis)
            with pytest.raises(pkg("scanner").Sl3dError):
                sc.last_fused_kernel_name()                       # no launch yet
            sc.run()
            names[(axis, anchored)] = (sc.fused_kernel_name(1), sc.last_fused_kernel_name())
            assert names[(axis, anchored)] == (want, want)
    assert len({n[0] for n in names.values()}) == 4 and all(n[0].startswith("sl3d::") for n in names.values())


# ---- 9. what it is for ---------------------------------------------------------------------------------------------------------------------
def test_accuracy_of_the_device_output():
    """Vertical only, anchored, full frame: the RMS distance to the true plane over good_pixels of the two-axis scan is at most 1.1 x the
    two-axis device scan's over the same pixels (tests/test_one_axis_arith.py (c) on the device's own planes)."""
    s = OC.scene(0, "full")
    cap = s["cap"]
    with _open(0, "full", keep=True, anchored=True, only=False) as sc:        # the two-axis scan
        sc.set_frames(0, cap["planes_v"])
        sc.set_frames(1, cap["planes_h"])
        sc.set_mask(pkg("synth").default_mask(*OC.FULL))
        sc.run()
        two, good = sc.intersection_points(), SC.good_pixels(cap, sc.c_p_map(), sc.valid_map())
    assert good.sum() > 60000
    y = _staged(0, "full", True)
    assert (y["want"]["valid"] == 1)[good].all()
    rms1, rms2 = SC.plane_rms(y["ipoints"], good), SC.plane_rms(two, good)
    print(f"RMS to the plane over {int(good.sum())} pixels: vertical only {rms1:.5f} mm, two axes {rms2:.5f} mm, ratio {rms1 / rms2:.3f}")
    assert rms1 <= 1.1 * rms2
