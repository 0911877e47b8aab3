"""GPU tests (-m gpu) of SL3D_FLAG_SUBPIXEL: sl3d_run on a flagged context leaves the sub-pixel scan.

The yardstick is the route of the definition on a SL3D_FLAG_KEEP_STAGES context with the same configuration, calibration, masks and frames:
sl3d_compute_wrapped_phase + sl3d_unwrap_phase of both axes, sl3d_compute_c_p_map, sl3d_triangulate_subpixel(+inf, NULL) -- which
tests/test_gpu_subpixel.py holds against the NumPy restatement.  "Equal" is equality of the bit patterns, NaNs included, of the points,
valid and residual planes over EVERY pixel of the window.  The scenes are those of tests/subpixel_cases.py (320 x 240 full frame; the
70 x 9 window at (37, 5): 80-column pitch with padding inside a tile, a partial last block, an origin that is no multiple of 4; plain,
radial and tangential rigs); the configurations the one kernel must cover come from synth.make_capture at 90 x 60."""
import functools

import numpy as np
import pytest

from conftest import assert_points_close, pkg

import subpixel_cases as SC

pytestmark = pytest.mark.gpu

INF = float("inf")
NAME = "k_subpixel_fused"


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _open(rig, win, *, keep=False, subpixel=False, max_views=1, eager_mask=False):
    s = SC.scene(rig, win)
    sc = pkg("scanner").Scanner(s["W"], s["H"], SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW, keep_stages=keep, full_size=SC.FULL, origin=s["origin"],
                                max_views=max_views, subpixel=subpixel, eager_mask=eager_mask)
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


def _yardstick(sc, first_view=0, n_views=1):
    """The route of the definition over views [first_view, first_view + n_views) of a KEEP_STAGES context; their planes."""
    for v in range(first_view, first_view + n_views):
        _stages345(sc, v)
    assert sc.triangulate_subpixel(first_view, n_views, want_counts=False) is None
    return [_out(sc, v) for v in range(first_view, first_view + n_views)]


def _out(sc, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid, residual=sc.residuals(view))


def _same(got, want, what):
    for k in ("valid", "points", "residual"):
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _sane(want, what, some_valid=True):
    """What every yardstick plane set satisfies by the definition (so that an empty comparison cannot pass for a full one)."""
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1}
    assert v.any() == some_valid, what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["residual"]), ~v), what


@functools.lru_cache(maxsize=None)
def _scene_yardstick(rig, win):
    """Per scene, computed once and left unchanged: the yardstick's planes, and the integer scan + c_p_map of the same context."""
    s = SC.scene(rig, win)
    with _open(rig, win, keep=True) as sc:
        _load(sc, s["cap"])
        _stages345(sc)
        sc.triangulate()
        integer = sc.points()
        cp = sc.c_p_map()
        want, = _yardstick(sc)
    _sane(want, (rig, win))
    return dict(want=want, integer=integer, c_p_map=cp)


# ---- 1. every scene -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_run_equals_the_staged_route(rig, win):
    s = SC.scene(rig, win)
    y = _scene_yardstick(rig, win)
    with _open(rig, win, subpixel=True) as sc:
        assert NAME in sc.fused_kernel_name(1) and "k_fused<" not in sc.fused_kernel_name(1)
        assert sc.camera_table_bytes_per_pixel(1) == 0
        _load(sc, s["cap"])
        sc.run()
        _same(_out(sc), y["want"], (rig, win))
        name = sc.last_fused_kernel_name()
        assert NAME in name and "k_fused<" not in name, name
        assert sc.launch_counts() == (1, 0)
    with _open(rig, win) as sc:                                # the same inputs, no flag: the integer scan by a k_fused instantiation
        _load(sc, s["cap"])
        sc.run()
        assert sc.last_fused_kernel_name().startswith("sl3d::k_fused<")
        xyz, valid = sc.points()
        assert np.array_equal(valid, y["integer"][1])
        assert_points_close(xyz, y["integer"][0].astype(np.float64), valid == 1)
        assert np.array_equal(np.isnan(xyz).any(-1), valid != 1)
        assert not np.array_equal(_bits(xyz), _bits(y["want"]["points"])), "the integer scan is not the sub-pixel scan"


# ---- 2. batches ---------------------------------------------------------------------------------------------------------------------------
def test_batches_and_the_views_outside_a_launch():
    rig, win = "radial", "full"
    caps = [SC.scene(rig, win, plane)["cap"] for plane in SC.VIEW_PLANES]
    with _open(rig, win, keep=True, max_views=3) as sc:
        for v, cap in enumerate(caps):
            _load(sc, cap, view=v)
        want = _yardstick(sc, 0, 3)
        _frames(sc, caps[2], view=1)                           # view 1 with view 2's frames
        want_swapped, = _yardstick(sc, 1, 1)
    for v in range(3):
        _sane(want[v], ("view", v))
    assert len({w["points"].tobytes() for w in want}) == 3, "the views must differ"
    with _open(rig, win, subpixel=True, max_views=3) as sc:
        for v, cap in enumerate(caps):
            _load(sc, cap, view=v)
        sc.run(0, 3)
        first = [_out(sc, v) for v in range(3)]
        for v in range(3):
            _same(first[v], want[v], ("run(0, 3)", v))
        _frames(sc, caps[2], view=1)
        sc.run(1, 1)
        _same(_out(sc, 1), want_swapped, "run(1, 1) over new frames")
        _same(_out(sc, 1), want[2], "view 1 now holds view 2's frames")
        for v in (0, 2):
            _same(_out(sc, v), first[v], ("view", v, "outside run(1, 1)"))
        _frames(sc, caps[1], view=1)
        sc.run(1, 2)
        for v in range(3):
            _same(_out(sc, v), first[v], ("after run(1, 2)", v))
        assert sc.launch_counts() == (3, 0)


# ---- 3. the configurations the one kernel must cover --------------------------------------------------------------------------------------
CONFIGS = {
    "four_step": dict(n_fringe=4, nv=5, nh=5, noise=0),
    "five_step": dict(n_fringe=5, nv=5, nh=5, noise=0),
    "unequal_axes": dict(n_fringe=3, nv=7, nh=5, noise=0),
    "thirteen_planes": dict(n_fringe=3, nv=13, nh=5, noise=0),
    "noise": dict(n_fringe=3, nv=5, nh=5, noise=2),
}


@pytest.mark.parametrize("name", CONFIGS)
def test_configurations(name):
    c = CONFIGS[name]
    W, H, PW, PH, FW = 90, 60, 128, 96, 4                       # (90 columns: a 96-column pitch, the last quad of a row half outside the window)
    syn = pkg("synth")
    cap = syn.make_capture(W, H, PW, PH, c["nv"], c["nh"], FW, FW, n_fringe=c["n_fringe"], noise=c["noise"])
    cal = syn.cal_tuple(cap["cal"])
    outs = {}
    for kind in ("yardstick", "flagged"):
        with pkg("scanner").Scanner(W, H, PW, PH, c["nv"], c["nh"], FW, FW, n_fringe=c["n_fringe"], keep_stages=kind == "yardstick",
                                    subpixel=kind == "flagged") as sc:
            sc.set_calibration(*cal)
            _frames(sc, cap)
            sc.set_mask(cap["mask"])
            if kind == "yardstick":
                outs[kind], = _yardstick(sc)
            else:
                sc.run()
                outs[kind] = _out(sc)
                assert NAME in sc.last_fused_kernel_name()
    _sane(outs["yardstick"], name, some_valid=c["n_fringe"] != 5)
    _same(outs["flagged"], outs["yardstick"], name)
    if c["n_fringe"] == 5:
        got = outs["flagged"]
        assert (got["valid"] == 0).all() and np.isnan(got["points"]).all() and np.isnan(got["residual"]).all()
    else:
        assert (outs["yardstick"]["valid"] == 1).sum() > 1000, name


# ---- 4. masks -----------------------------------------------------------------------------------------------------------------------------
def _hole_and_notch():
    """Every pixel of the frame selected -- the frame's border too, where stage 4's loop does not run -- but a hole and a notch."""
    W, H = SC.FULL
    m = np.ones((H, W), np.uint8)
    m[100:121, 150:183] = 0
    m[0:31, 201:210] = 0
    m[57, 3] = 0
    return m


MODULATION = 0.6   # min_modulation: the smaller gamma of the two axes of this capture has its quartiles at 0.54, 0.76 and 0.94


@functools.lru_cache(maxsize=None)
def _mask_yardstick(modulated):
    s = SC.scene("plain", "full")
    with _open("plain", "full", keep=True) as sc:
        _frames(sc, s["cap"])
        thr = MODULATION if modulated else None
        if modulated:
            sc.set_masks_modulated(thr, _hole_and_notch())
        else:
            sc.set_mask(_hole_and_notch())
        want, = _yardstick(sc)
    _sane(want, ("mask", modulated))
    return want, thr


@pytest.mark.parametrize("how", ["deferred", "eager", "modulated"])
def test_masks(how):
    s = SC.scene("plain", "full")
    want, thr = _mask_yardstick(how == "modulated")
    plain = _mask_yardstick(False)[0]
    n = int((want["valid"] == 1).sum())
    assert (plain["valid"][0] == 1).any() and (plain["valid"][:, 0] == 1).any(), "pixels of the frame's border are valid"
    assert (want["valid"][105:115, 160:170] == 0).all()
    if how == "modulated":
        assert 0 < n < int((plain["valid"] == 1).sum()), "the threshold removes some pixels"
    with _open("plain", "full", subpixel=True, eager_mask=how == "eager") as sc:
        _frames(sc, s["cap"])
        if how == "modulated":
            sc.set_masks_modulated(thr, _hole_and_notch())
        else:
            sc.set_mask(_hole_and_notch())                     # set and run at once on one view
        sc.run()
        _same(_out(sc), want, how)
        assert NAME in sc.last_fused_kernel_name()


# ---- 5. consumers -------------------------------------------------------------------------------------------------------------------------
def test_consumers_of_the_dense_planes():
    s = SC.scene("plain", "full")
    res = {}
    for kind in ("yardstick", "flagged"):
        with _open("plain", "full", keep=kind == "yardstick", subpixel=kind == "flagged") as sc:
            _load(sc, s["cap"])
            if kind == "yardstick":
                _yardstick(sc)
            else:
                sc.run()
            xyz, valid = sc.points()
            step = np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)
            max_edge = 1.25 * float(np.nanmedian(step))
            res[kind] = dict(cloud=sc.cloud(), max_edge=max_edge, mesh_inf=sc.mesh(INF), mesh=sc.mesh(max_edge), normals=sc.mesh_normals(max_edge))
            assert np.array_equal(_bits(res[kind]["cloud"]), _bits(xyz[valid == 1]))
    a, b = res["flagged"], res["yardstick"]
    assert a["max_edge"] == b["max_edge"]
    assert len(b["cloud"]) > 60000 and np.array_equal(_bits(a["cloud"]), _bits(b["cloud"]))
    for k in ("mesh_inf", "mesh"):
        assert np.array_equal(_bits(a[k][0]), _bits(b[k][0])) and np.array_equal(a[k][1], b[k][1]), k
    assert 0 < len(b["mesh"][1]) < len(b["mesh_inf"][1])
    assert a["normals"].shape == b["normals"].shape and np.array_equal(_bits(a["normals"]), _bits(b["normals"]))
    assert np.abs(b["normals"]).max() > 0.5


# ---- 6. KEEP_STAGES | SUBPIXEL ------------------------------------------------------------------------------------------------------------
def test_keep_stages_with_the_flag():
    rig, win = "tangential", "full"
    s = SC.scene(rig, win)
    y = _scene_yardstick(rig, win)

    def stage_planes(sc):
        return dict(c_p_map=sc.c_p_map(), valid_v=sc.valid_map(0), valid_h=sc.valid_map(1), unw_v=sc.unwrapped_phase(0), unw_h=sc.unwrapped_phase(1))

    with _open(rig, win, keep=True) as sc:
        _load(sc, s["cap"])
        sc.run()
        parity = stage_planes(sc)
    with _open(rig, win, keep=True, subpixel=True) as sc:
        _load(sc, s["cap"])
        sc.run()
        _same(_out(sc), y["want"], "KEEP_STAGES | SUBPIXEL")
        assert sc.last_fused_kernel_name().startswith("sl3d::k_fused<true")
        got = stage_planes(sc)
        for k in parity:
            assert np.array_equal(_bits(got[k]), _bits(parity[k])), k
        sc.compute_c_p_map()
        sc.triangulate()
        xyz, valid = sc.points()
        assert np.array_equal(valid, y["integer"][1]) and np.array_equal(_bits(xyz), _bits(y["integer"][0])), "the integer result is restored"


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_flagged_timed_context():
    s = SC.scene("plain", "window")
    buf = np.zeros((s["H"], s["W"]), np.float32)
    with _open("plain", "window", subpixel=True) as sc:
        L, h = sc.L, sc._h
        _load(sc, s["cap"])
        assert L.sl3d_get_residuals(h, 0, buf.ctypes.data, s["W"]) == -4 and b"sl3d_run" in L.sl3d_last_error(h)
        with pytest.raises(pkg("scanner").Sl3dError):
            sc.last_fused_kernel_name()
        sc.run()
        before = _out(sc)
        _same(before, _scene_yardstick("plain", "window")["want"], "the run before the refusals")

        def unchanged(what):
            xyz, valid = sc.points()
            assert np.array_equal(valid, before["valid"]) and np.array_equal(_bits(xyz), _bits(before["points"])), what

        assert L.sl3d_run_clouds(h, 0, 1) == -5 and b"sl3d_compact_views" in L.sl3d_last_error(h) and b"sl3d_run" in L.sl3d_last_error(h)
        unchanged("sl3d_run_clouds")
        assert L.sl3d_triangulate_subpixel(h, 0, 1, INF, None) == -4 and b"KEEP_STAGES" in L.sl3d_last_error(h)
        unchanged("sl3d_triangulate_subpixel")
        xy = np.zeros((s["H"], s["W"], 2))
        assert L.sl3d_get_correspondences_subpixel(h, 0, xy.ctypes.data, s["W"]) == -4
        assert L.sl3d_compute_c_p_map(h, 0) == -4
        unchanged("the per-stage calls")
        _same(_out(sc), before, "the end")
    with _open("plain", "window", subpixel=True) as sc:          # the residuals' refusal leaves the planes as sl3d_create left them
        _load(sc, s["cap"])
        xyz0, valid0 = sc.points()
        assert sc.L.sl3d_get_residuals(sc._h, 0, buf.ctypes.data, s["W"]) == -4
        xyz, valid = sc.points()
        assert np.array_equal(valid, valid0) and np.array_equal(_bits(xyz), _bits(xyz0))


# ---- 8. a group ---------------------------------------------------------------------------------------------------------------------------
def test_group_of_three_stripes():
    S = pkg("scanner")
    s = SC.scene("plain", "full")
    want = _scene_yardstick("plain", "full")["want"]
    with _open("plain", "full", subpixel=True) as sc:
        _load(sc, s["cap"])
        sc.run()
        single = _out(sc)
    _same(single, want, "the single flagged context")
    W, H = SC.FULL
    with S.Group(W, H, SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW, devices=[0, 0, 0], flags=S.SL3D_FLAG_SUBPIXEL) as g:
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


# ---- 9. the host pipeline -----------------------------------------------------------------------------------------------------------------
def test_process_views_equals_run():
    rig, win = "radial", "window"
    caps = [SC.scene(rig, win, plane)["cap"] for plane in SC.VIEW_PLANES[:2]]
    with _open(rig, win, subpixel=True, max_views=2) as sc:
        for v, cap in enumerate(caps):
            _load(sc, cap, view=v)
        sc.run(0, 2)
        want = [_out(sc, v) for v in range(2)]
        assert len({w["points"].tobytes() for w in want}) == 2
    with _open(rig, win, subpixel=True, max_views=2) as sc:
        for v in range(2):
            sc.set_mask(pkg("synth").default_mask(*SC.FULL), view=v)
        frames = np.stack([np.stack(cap["planes_v"] + cap["planes_h"]) for cap in caps])
        xyz, valid = sc.process_views(frames)
        for v in range(2):
            assert np.array_equal(valid[v], want[v]["valid"]) and np.array_equal(_bits(xyz[v]), _bits(want[v]["points"])), v
            _same(_out(sc, v), want[v], ("the slot's planes", v))
        assert NAME in sc.last_fused_kernel_name()


# ---- 10. what it is for -------------------------------------------------------------------------------------------------------------------
def test_plane_accuracy_of_the_flagged_run():
    s = SC.scene("plain", "full")
    y = _scene_yardstick("plain", "full")
    runs = {}
    for flagged in (False, True):
        with _open("plain", "full", subpixel=flagged) as sc:
            _load(sc, s["cap"])
            sc.run()
            runs[flagged] = sc.points()
    assert np.array_equal(runs[False][1], runs[True][1])
    good = SC.good_pixels(s["cap"], y["c_p_map"], runs[True][1])
    assert good.sum() > 60000
    a, b = SC.plane_rms(runs[False][0], good), SC.plane_rms(runs[True][0], good)
    print(f"RMS distance to the plane: unflagged run {a:.4f} mm, flagged run {b:.4f} mm, ratio {b / a:.3f}")
    assert b <= 0.5 * a
