"""GPU tests (-m gpu) of the sub-pixel launches -- k_subpixel_fused<ANCHOR>, k_one_axis<AXIS, ANCHOR> and the staged kernels behind them
(k_corr_one, k_subpixel_one, k_subpixel_coords_one, k_subpixel, k_subpixel_coords) -- on the inputs of tests/edge_frames.py: random bytes,
flat frames, a noisy capture with an unlit part, ragged sizes under random masks (one holds the value 2), a window, and three views whose
masks select different quads and lanes.  tests/test_edge_frames.py proves on the CPU that these inputs take the branches named here.

(a) A one-axis context against the ORACLE (stage 3 and 4 planes, the valid byte, c_p_map of the coded axis: exact) and against the NumPy
    restatement applied to the oracle's planes (coordinates bit for bit, points at the project's 1e-5 bar); sl3d_run of the timed context
    equals the staged route bit for bit on every pixel.
(b) The same for the two-axis sub-pixel scan, plain and anchored, residual plane included.
(c) Per-view masks in one launch, for all six timed instantiations: views 1..3 behind an untouched slot hold three captures under the
    masks A, B, C; run, run_timed and a run after A and C changed places equal each view run alone, bit for bit.  Once with eager masks,
    once with sl3d_set_masks_modulated per view.
(d) One-axis configurations on a 90 x 60 frame: F = 5, no Gray plane on the coded axis, N = 1, 5 and 16, noise, a small extent.
(e) The staged one-axis route over three views of one call, and the counts of sl3d_triangulate_subpixel over them.
(f) A group of three row stripes, horizontal only."""
import numpy as np
import pytest

from conftest import assert_points_close, pkg

import edge_frames as EF
import one_axis_cases as OC
import one_axis_reference as OR

pytestmark = pytest.mark.gpu

ONE_AXIS = {(0, False): "sl3d::k_one_axis<0, false>", (0, True): "sl3d::k_one_axis<0, true>", (1, False): "sl3d::k_one_axis<1, false>",
            (1, True): "sl3d::k_one_axis<1, true>"}
TWO_AXIS = {False: "sl3d::k_subpixel_fused<false>", True: "sl3d::k_subpixel_fused<true>"}
CASE_IDS = [f"{name}-{shape}-{p}" for name, shape, p in EF.CASES]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _same(got, want, what):
    for k in ("valid", "points"):
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _sane(want, what):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1} and v.any(), what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["points"]).all(-1), ~v), what


def _same_all(got, want, what):
    """_same, and every further plane the two dicts hold (the residuals of a two-axis context)."""
    _same(got, want, what)
    for k in set(want) - {"valid", "points"}:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, int((_bits(got[k]) != _bits(want[k])).sum()), "elements differ")


def _open(c, *, axis=None, keep=False, anchored=False, max_views=1, eager_mask=False):
    """A SUBPIXEL context of a case of tests/edge_frames.py; axis: the one coded axis, or None for the two-axis scan."""
    sc = pkg("scanner").Scanner(c["W"], c["H"], EF.PW, EF.PH, EF.N[0], EF.N[1], EF.FW[0], EF.FW[1], keep_stages=keep, full_size=c["full"], origin=c["origin"],
                                max_views=max_views, subpixel=True, anchored=anchored, only_axis=axis, eager_mask=eager_mask)
    sc.set_calibration(*c["cal"])
    return sc


def _axes(axis):
    return (0, 1) if axis is None else (axis,)


def _frames(sc, planes, axis, view=0):
    """The frames of the coded axis alone on a one-axis context, of both axes otherwise."""
    for a in _axes(axis):
        sc.set_frames(a, planes[a], view=view)


def _out(sc, axis, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid) if axis is not None else dict(points=xyz, valid=valid, residual=sc.residuals(view))


def _nothing(out):
    return (out["valid"] == 0).all() and np.isnan(out["points"]).all() and all(np.isnan(out[k]).all() for k in out if k == "residual")


def _compare_stage_planes(sc, o, a, mask, inn, what):
    """One axis of tests/test_gpu_stage_parity.py::_compare with staged=True, on the pixels `inn` of the window."""
    va = (o["valid_axis"][a] == 1) & inn
    assert np.array_equal(sc.valid_map(a)[inn], o["valid_axis"][a][inn]), f"{what}: valid map axis {a}"
    assert np.array_equal(sc.code(a)[inn], o["code"][a][inn]), f"{what}: code axis {a}"
    where = (mask == 1) & inn
    assert np.array_equal(_bits(sc.wrapped_phase(a))[where], _bits(o["w"][a])[where]), f"{what}: wrapped phase axis {a}"
    assert np.array_equal(_bits(sc.unwrapped_phase(a))[va], _bits(o["unw"][a])[va]), f"{what}: unwrapped phase axis {a}"


# ---- (a) one axis against the oracle and the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name,shape,p", EF.CASES, ids=CASE_IDS)
def test_one_axis_against_the_oracle(name, shape, p, axis, anchored):
    what = (name, shape, p, axis, anchored)
    c, o, want = EF.case(name, shape, p, axis), EF.oracle_scan(name, shape, p, axis), EF.restated_one_axis(name, shape, p, axis, anchored)
    inn, mask = EF.inner(shape), EF.window(c["mask"], shape)
    v = (want["valid"] == 1) & inn
    with _open(c, axis=axis, keep=True, anchored=anchored) as sc:
        _frames(sc, c["planes"], axis)
        sc.set_mask(c["mask"])
        sc.compute_wrapped_phase(axis)
        sc.unwrap_phase(axis)
        _compare_stage_planes(sc, o, axis, mask, inn, what)
        sc.compute_c_p_map()
        valid5, cp = sc.valid_map(), sc.c_p_map()
        xy = sc.correspondences_subpixel()
        counts = sc.triangulate_subpixel()
        staged = _out(sc, axis)
        ip = sc.intersection_points()
        _compare_stage_planes(sc, o, axis, mask, inn, (what, "after stage 5 and the solve"))
    # stage 5: the merged valid map and c_p_map are the restatement's; the coded component is the oracle's wherever the oracle has one
    assert np.array_equal(valid5[inn], want["valid"][inn]) and np.array_equal(staged["valid"][inn], want["valid"][inn]), "merged valid map"
    assert np.array_equal(cp[..., axis][v], want["c_p_map"][..., axis][v]) and np.array_equal(cp[inn], want["c_p_map"][inn]), "c_p_map"
    both = (o["valid"] == 1) & inn
    assert (want["valid"] == 1)[both].all() and np.array_equal(cp[..., axis][both], o["c_p_map"][..., axis][both]), "c_p_map against the oracle's"
    assert counts == [(int((staged["valid"] == 1).sum()), 0)]
    # the coordinates: bit for bit, NaN pattern included
    nan = np.isnan(want["xy"])
    assert np.array_equal(np.isnan(xy)[inn], nan[inn]) and nan[..., 1 - axis].all(), "NaN pattern of the coordinates"
    ok = ~nan & inn[..., None]
    assert np.array_equal(_bits(xy)[ok], _bits(want["xy"])[ok]), (int((_bits(xy)[ok] != _bits(want["xy"])[ok]).sum()), "coordinates differ")
    # the points
    assert np.array_equal(np.isnan(staged["points"]).any(-1), staged["valid"] != 1) and np.array_equal(np.isnan(staged["points"]).all(-1), staged["valid"] != 1)
    e_f = assert_points_close(staged["points"], want["ipoints"], v)
    e_d = assert_points_close(ip, want["ipoints"], v)
    assert (ip[staged["valid"] != 1] == 0).all()
    on = staged["valid"] == 1
    assert np.array_equal(_bits(staged["points"][on]), _bits(ip[on].astype(np.float32))), "points are the float cast of intersection_points"
    if inn.all() and not (want["valid"] == 1).any():
        assert _nothing(staged), "nothing is valid"
    print(f"{what}: {int(v.sum())} valid of {int(inn.sum())} compared, points {e_f:.2e} rel, intersection_points {e_d:.2e} rel")
    # the timed context
    with _open(c, axis=axis, anchored=anchored) as sc:
        assert sc.fused_kernel_name(1) == ONE_AXIS[(axis, anchored)]
        _frames(sc, c["planes"], axis)
        sc.set_mask(c["mask"])
        sc.run()
        _same(_out(sc, axis), staged, what)
        assert sc.last_fused_kernel_name() == ONE_AXIS[(axis, anchored)] and sc.launch_counts() == (1, 0)


# ---- (b) two axes, plain and anchored --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("name,shape,p", EF.CASES, ids=CASE_IDS)
def test_two_axes_against_the_oracle(name, shape, p, anchored):
    what = (name, shape, p, anchored)
    c, o, want = EF.case(name, shape, p), EF.oracle_scan(name, shape, p), EF.restated_two_axis(name, shape, p, anchored)
    inn, mask = EF.inner(shape), EF.window(c["mask"], shape)
    v = (o["valid"] == 1) & inn
    with _open(c, keep=True, anchored=anchored) as sc:
        _frames(sc, c["planes"], None)
        sc.set_mask(c["mask"])
        for a in (0, 1):
            sc.compute_wrapped_phase(a)
        for a in (0, 1):
            sc.unwrap_phase(a)
        sc.compute_c_p_map()
        for a in (0, 1):
            _compare_stage_planes(sc, o, a, mask, inn, what)
        valid5, cp = sc.valid_map(), sc.c_p_map()
        xy = sc.correspondences_subpixel()
        counts = sc.triangulate_subpixel()
        staged = _out(sc, None)
        ip = sc.intersection_points()
    assert np.array_equal(valid5[inn], o["valid"][inn]) and np.array_equal(staged["valid"][inn], o["valid"][inn]), "merged valid map"
    assert np.array_equal(cp[v], o["c_p_map"][v]), "c_p_map"
    assert counts == [(int((staged["valid"] == 1).sum()), 0)]
    nan = np.isnan(want["xy"])
    assert np.array_equal(np.isnan(xy)[inn], nan[inn]), "NaN pattern of the coordinates"
    ok = ~nan & inn[..., None]
    assert np.array_equal(_bits(xy)[ok], _bits(want["xy"])[ok]), (int((_bits(xy)[ok] != _bits(want["xy"])[ok]).sum()), "coordinates differ")
    on = staged["valid"] == 1
    assert np.array_equal(np.isnan(staged["points"]).any(-1), ~on) and np.array_equal(np.isnan(staged["points"]).all(-1), ~on) and np.array_equal(np.isnan(staged["residual"]), ~on)
    e_f = assert_points_close(staged["points"], want["ipoints"], v)
    e_d = assert_points_close(ip, want["ipoints"], v)
    ref = want["residual"][v].astype(np.float64)
    err = np.abs(staged["residual"][v].astype(np.float64) - ref)
    print(f"{what}: {int(v.sum())} valid of {int(inn.sum())} compared, points {e_f:.2e} rel, intersection_points {e_d:.2e} rel, residuals max |diff| "
          f"{err.max() if len(err) else 0.0:.2e} px (largest {ref.max() if len(ref) else 0.0:.3g} px)")
    assert (err <= 1e-6 * ref + 1e-7).all(), (float(err.max()), float(ref[np.argmax(err - 1e-6 * ref)]))
    if inn.all() and not v.any():
        assert _nothing(staged), "nothing is valid"
    with _open(c, anchored=anchored) as sc:
        assert sc.fused_kernel_name(1) == TWO_AXIS[anchored]
        _frames(sc, c["planes"], None)
        sc.set_mask(c["mask"])
        sc.run()
        _same_all(_out(sc, None), staged, what)
        assert sc.last_fused_kernel_name() == TWO_AXIS[anchored] and sc.launch_counts() == (1, 0)


# ---- (c) per-view masks in one launch --------------------------------------------------------------------------------------------------------
def _alone(c, axis, anchored, planes, select, eager):
    """One view run alone on a one-view context under the 0 / 1 selection `select`: the yardstick."""
    with _open(c, axis=axis, anchored=anchored, eager_mask=eager) as sc:
        _frames(sc, planes, axis)
        sc.set_mask(select)
        sc.run()
        return _out(sc, axis)


def _modulated_selection(c, axis, planes, mask, thr):
    """(mask == 1) && gamma > thr on every coded axis, from sl3d_get_modulation of a context that holds the frames; and the gammas."""
    with _open(c, axis=axis) as sc:
        _frames(sc, planes, axis)
        gammas = [sc.modulation(a) for a in _axes(axis)]
    select = mask == 1
    with np.errstate(invalid="ignore"):
        for g in gammas:
            select = select & (g.astype(np.float64) > thr)
    return select.astype(np.uint8), gammas


@pytest.mark.parametrize("mode", ["eager", "modulated"])
@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("axis", [None, 0, 1], ids=["two_axes", "vertical", "horizontal"])
def test_per_view_masks_in_one_launch(axis, anchored, mode):
    rig_axis = 0 if axis is None else axis
    c = EF.case("flat_17", "base", 1.0, rig_axis)               # (the shape and the calibration of the base case)
    caps, (A, B, C) = EF.view_captures(rig_axis), EF.view_masks()
    name = TWO_AXIS[anchored] if axis is None else ONE_AXIS[(axis, anchored)]
    eager = mode == "eager"
    thr = None
    if not eager:
        # a threshold from the gammas the device reports: the tenth part of the pixels fails it
        with _open(c, axis=axis) as sc:
            pooled = []
            for planes in caps:
                _frames(sc, planes, axis)
                pooled += [sc.modulation(a) for a in _axes(axis)]
        pooled = np.stack(pooled)
        thr = float(np.quantile(pooled[np.isfinite(pooled)].astype(np.float64), 0.1))

    def yardstick(view, mask):
        if eager:
            return _alone(c, axis, anchored, caps[view], mask, True)
        select, gammas = _modulated_selection(c, axis, caps[view], mask, thr)
        taken, left = int(select.sum()), int(((mask == 1) & (select == 0)).sum())
        if mask is not C:
            assert min(taken, left) >= 100, (view, taken, left, "each branch of the modulation test takes a hundred pixels or more")
        return _alone(c, axis, anchored, caps[view], select, False)

    want = {1: yardstick(0, A), 2: yardstick(1, B), 3: yardstick(2, C)}
    swapped = {1: yardstick(0, C), 2: want[2], 3: yardstick(2, A)}
    for k, w in list(want.items()) + list(swapped.items()):
        _sane(w, ("yardstick", k))
    assert len({w["points"].tobytes() for w in want.values()}) == 3, "the views must differ"

    def set_masks(sc, masks):
        for v, m in masks.items():
            if eager:
                sc.set_mask(m, view=v)
            else:
                sc.set_masks_modulated(thr, m, first_view=v, n_views=1)

    with _open(c, axis=axis, anchored=anchored, max_views=4, eager_mask=eager) as sc:
        for v, planes in enumerate(caps, start=1):
            _frames(sc, planes, axis, view=v)
        set_masks(sc, {1: A, 2: B, 3: C})
        slot0 = sc.points(0)
        sc.run(1, 3)
        assert sc.last_fused_kernel_name() == name
        for v in want:
            _same_all(_out(sc, axis, v), want[v], ("run(1, 3)", v))
        assert sc.run_timed(1, 3) > 0
        for v in want:
            _same_all(_out(sc, axis, v), want[v], ("run_timed(1, 3)", v))
        set_masks(sc, {1: C, 3: A})
        sc.run(1, 3)
        for v in swapped:
            _same_all(_out(sc, axis, v), swapped[v], ("run(1, 3) after A and C changed places", v))
        after = sc.points(0)
        assert np.array_equal(after[1], slot0[1]) and np.array_equal(_bits(after[0]), _bits(slot0[0])), "slot 0 is untouched"
        assert sc.last_fused_kernel_name() == name


# ---- (d) one-axis configurations -------------------------------------------------------------------------------------------------------------
# n_fringe, Gray planes and fringe width of the coded axis (by axis where the extents 128 and 96 ask for it), noise
CONFIGS = {
    "five_step": (5, 5, (4, 4), 0),
    "no_gray_on_the_coded_axis": (3, 0, (128, 96), 0),
    "one_plane": (3, 1, (64, 48), 0),
    "odd_planes": (3, 5, (4, 4), 0),
    "sixteen_planes": (3, 16, (4, 4), 0),                        # the extent stays 128 / 96, far below 4 * 2^16
    "noise": (3, 5, (4, 4), 2),
    "small_extent": (3, 6, (4, 4), 0),                           # 4 * 2^6 = 256 codes' worth of columns against an extent of 128 / 96
}


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", CONFIGS)
def test_one_axis_configurations(name, axis):
    F, n, fws, noise = CONFIGS[name]
    W, H, PW, PH = 90, 60, 128, 96                               # (90 columns: a 96-column pitch, the last quad of a row half outside the window)
    N, FW = [5, 5], [4, 4]
    N[axis], FW[axis] = n, fws[axis]
    extent = (PW, PH)[axis]
    syn = pkg("synth")
    cap = syn.make_capture(W, H, PW, PH, N[0], N[1], FW[0], FW[1], cal=EF.rig(axis, W, H, PW, PH), n_fringe=F, noise=noise)
    cal, planes = syn.cal_tuple(cap["cal"]), (cap["planes_v"], cap["planes_h"])
    outs, xy = {}, {}
    for kind in ("staged", "timed", "unanchored"):
        with pkg("scanner").Scanner(W, H, PW, PH, N[0], N[1], FW[0], FW[1], n_fringe=F, keep_stages=kind != "timed", subpixel=True, anchored=kind != "unanchored",
                                    only_axis=axis) as sc:
            sc.set_calibration(*cal)
            sc.set_frames(axis, planes[axis])
            sc.set_mask(cap["mask"])
            if kind == "timed":
                sc.run()
                assert sc.last_fused_kernel_name() == ONE_AXIS[(axis, True)]
            else:
                sc.compute_wrapped_phase(axis)
                sc.unwrap_phase(axis)
                if kind == "staged":
                    inp = dict(w=sc.wrapped_phase(axis), code=sc.code(axis), unw=sc.unwrapped_phase(axis), sel=sc.valid_map(axis), A=sc.projection_matrices())
                sc.compute_c_p_map()
                xy[kind] = sc.correspondences_subpixel()
                assert sc.triangulate_subpixel(want_counts=False) is None
            outs[kind] = _out(sc, axis)
    _same(outs["timed"], outs["staged"], (name, axis))
    assert np.array_equal(outs["unanchored"]["valid"], outs["staged"]["valid"])
    if F == 5:
        assert _nothing(outs["timed"]) and _nothing(outs["staged"]) and np.isnan(xy["staged"]).all()
        return
    _sane(outs["staged"], (name, axis))
    v = outs["staged"]["valid"] == 1
    assert v.sum() > 1000, (name, axis, int(v.sum()))
    want = OR.scan(inp["w"], inp["code"], inp["unw"], inp["sel"], cal, *inp["A"], axis, FW[axis], extent, n, F, (0, 0), (W, H), True)
    assert np.array_equal(outs["staged"]["valid"], want["valid"])
    nan = np.isnan(want["xy"])
    assert np.array_equal(np.isnan(xy["staged"]), nan) and np.array_equal(_bits(xy["staged"])[~nan], _bits(want["xy"])[~nan])
    assert_points_close(outs["staged"]["points"], want["ipoints"], v)
    same = np.array_equal(_bits(xy["staged"][..., axis]), _bits(xy["unanchored"][..., axis]))
    assert same == (n == 0), (name, axis, "an axis without Gray planes keeps the unanchored coordinate, an axis with them does not")
    if n == 0:
        _same(outs["staged"], outs["unanchored"], (name, axis, "no Gray planes"))
    else:
        assert not np.array_equal(_bits(outs["staged"]["points"]), _bits(outs["unanchored"]["points"]))


# ---- (e) the staged one-axis route over three views ------------------------------------------------------------------------------------------
def _staged_planes(sc, view):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid, ipoints=sc.intersection_points(view), c_p_map=sc.c_p_map(view), xy=sc.correspondences_subpixel(view))


@pytest.mark.parametrize("axis", [0, 1])
def test_staged_one_axis_route_over_three_views(axis):
    c = EF.case("flat_17", "base", 1.0, axis)
    caps, masks = EF.view_captures(axis), EF.view_masks()
    want = {}
    for v, (planes, mask) in enumerate(zip(caps, masks), start=1):
        with _open(c, axis=axis, keep=True, anchored=True) as sc:
            _frames(sc, planes, axis)
            sc.set_mask(mask)
            sc.run()
            want[v] = _staged_planes(sc, 0)
        _sane(want[v], ("view", v))
    n_valid = {v: int((w["valid"] == 1).sum()) for v, w in want.items()}
    assert len(set(n_valid.values())) == 3, (n_valid, "the counts of the views must differ")
    with _open(c, axis=axis, keep=True, anchored=True, max_views=4) as sc:
        for v, (planes, mask) in enumerate(zip(caps, masks), start=1):
            _frames(sc, planes, axis, view=v)
            sc.set_mask(mask, view=v)
        sc.run(1, 3)
        for v in want:
            _same_all(_staged_planes(sc, v), want[v], ("run(1, 3)", v))
        assert sc.triangulate_subpixel(1, 3) == [(n_valid[v], 0) for v in (1, 2, 3)]
        for v in want:
            _same_all(_staged_planes(sc, v), want[v], ("triangulate_subpixel(1, 3)", v))


# ---- (f) a horizontal-only group -------------------------------------------------------------------------------------------------------------
def test_group_of_three_stripes_horizontal_only():
    S = pkg("scanner")
    axis = 1
    s = OC.scene(axis, "full")
    W, H = OC.FULL
    mask = pkg("synth").default_mask(W, H)
    with S.Scanner(W, H, OC.PW, OC.PH, OC.N[0], OC.N[1], OC.FW[0], OC.FW[1], subpixel=True, anchored=True, only_axis=axis) as sc:
        sc.set_calibration(*s["cal"])
        sc.set_frames(axis, s["cap"]["planes_h"])
        sc.set_mask(mask)
        sc.run()
        single = _out(sc, axis)
    _sane(single, "the single context")
    with S.Group(W, H, OC.PW, OC.PH, OC.N[0], OC.N[1], OC.FW[0], OC.FW[1], devices=[0, 0, 0],
                 flags=S.SL3D_FLAG_SUBPIXEL | S.SL3D_FLAG_ANCHOR_PERIODS | S.SL3D_FLAG_ONLY_HORIZONTAL) as g:
        stripes = g.stripes()
        assert len(stripes) == 3
        row0, rows = stripes[1][0], stripes[1][1]
        assert 0 < row0 and row0 + rows < H
        # an interior stripe's first and last row hold valid pixels: there a stripe border that passed for the frame's would show
        assert (single["valid"][row0] == 1).sum() > 100 and (single["valid"][row0 + rows - 1] == 1).sum() > 100
        g.set_calibration(*s["cal"])
        g.set_frames(axis, s["cap"]["planes_h"])
        g.set_mask(mask)
        g.run()
        xyz, valid = g.download_points()
        assert np.array_equal(valid[0], single["valid"]) and np.array_equal(_bits(xyz[0]), _bits(single["points"])), "download_points"
        g.gather()
        xyz, valid = g.points()
        assert np.array_equal(valid, single["valid"]) and np.array_equal(_bits(xyz), _bits(single["points"])), "gather + get_points"
        g.synchronize()
