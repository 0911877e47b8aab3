"""GPU tests (-m gpu) of SL3D_FLAG_DIRECT_GRAY: stage 4's Gray bit against the fringe mean, no inverse Gray frame read.  Unless a
test says otherwise only the F + N fringe and Gray planes of each coded axis are ever set (Scanner.set_frames -> sl3d_set_frames_range).

The yardstick of the decode: tests/direct_gray_reference.py.  as_inverse_coded() turns a capture into one on which the reference's own bit IS
the direct bit, so the ORACLE run on it gives the stage planes of a flagged context, and the restatements that exist
(tests/subpixel_reference.py, tests/anchor_reference.py, tests/one_axis_reference.py) give the coordinates and the points from those.

1. / 5. The staged route (KEEP_STAGES) on every case of tests/edge_frames.py -- random bytes, flat frames (every bit a tie 2 g == I0 + I2,
   atan2(0, 0)), a noisy capture with an unlit part, ragged sizes, the 70 x 9 window at the odd origin (37, 5) of a 320 x 240 frame --, one
   axis or two, plain or anchored: code and phases bit for bit, the code also against the restatement itself, the sub-pixel coordinates bit
   for bit, points at the project's 1e-5 bar and at BAR_ULPS scaled float32 ulps (tests/point_bars.py).  Then sl3d_run of the same context,
   and the timed context: bit for bit the staged route's, NaN patterns included; kernel name, launch counts, table bytes.
2. / 4. All six timed instantiations against the staged route on a 90 x 60 frame over N = 0, 1, 5, 16 and unequal axes, F = 3, 4, 5 and
   noise; without noise the flagged scan equals the unflagged scan of the same context flags, bit for bit.
2c. Per-view masks (eager and modulated), three views behind an untouched slot.
3. The inverse slots filled with random bytes, then with their correct content: identical results.
6. sl3d_process_views with NULL inverse pointers.  7. Groups of three stripes.  8. sl3d_repair_periods on a flagged KEEP context.
   sl3d_process_views with a contiguous 4-D array: one copy per coded axis, the inverse slots not written.
9. The kernel names.  10. 13 frames against 23 at N = 10, fringe width 2: the same points on every good pixel, the same RMS to the plane.
Where the codes agree (no noise) k_unwrap_direct is also held to k_unwrap plane by plane: the two kernels share their text but for the bit."""
import functools

import numpy as np
import pytest

from conftest import assert_points_close, pkg
from oracle.oracle import Oracle
from point_bars import scaled_ulps

import anchor_reference as AR
import direct_gray_reference as DG
import edge_frames as EF
import one_axis_reference as OR
import subpixel_reference as SR
from period_repair_checks import check_pass

pytestmark = pytest.mark.gpu

# one float32 rounding of each of two fp64 points that agree far below a float32 ulp (fused against unfused multiply-adds: 1e-11 relative),
# plus one: the bar tests/test_gpu_instantiations.py holds the float cast of an fp64 chain to
BAR_ULPS = 2.0
MODES = [None, 0, 1]
MODE_IDS = ["two_axes", "vertical", "horizontal"]
NAMES = {(axis, anchored): "sl3d::k_direct_gray<%d, %s>" % (2 if axis is None else axis, "true" if anchored else "false") for axis in MODES for anchored in (False, True)}
UNFLAGGED = {(None, False): "sl3d::k_subpixel_fused<false>", (None, True): "sl3d::k_subpixel_fused<true>", (0, False): "sl3d::k_one_axis<0, false>",
             (0, True): "sl3d::k_one_axis<0, true>", (1, False): "sl3d::k_one_axis<1, false>", (1, True): "sl3d::k_one_axis<1, true>"}
CASE_IDS = [f"{name}-{shape}-{p}" for name, shape, p in EF.CASES]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _same(got, want, what):
    """valid, points and every further plane the two dicts hold (the residuals of a two-axis context), bit for bit."""
    assert set(got) == set(want), what
    for k in want:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _sane(want, what):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1} and v.any(), what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["points"]).all(-1), ~v), what
    if "residual" in want:
        assert np.array_equal(np.isnan(want["residual"]), ~v), what


def _nothing(out):
    return (out["valid"] == 0).all() and np.isnan(out["points"]).all() and all(np.isnan(out[k]).all() for k in out if k == "residual")


def _axes(axis):
    return (0, 1) if axis is None else (axis,)


def _scanner(W, H, PW, PH, N, FW, cal, *, axis, keep=False, anchored=False, direct=True, max_views=1, eager_mask=False, n_fringe=3, full=None, origin=(0, 0)):
    sc = pkg("scanner").Scanner(W, H, PW, PH, N[0], N[1], FW[0], FW[1], n_fringe=n_fringe, keep_stages=keep, full_size=full, origin=origin, max_views=max_views,
                                subpixel=True, anchored=anchored, only_axis=axis, eager_mask=eager_mask, direct_gray=direct)
    sc.set_calibration(*cal)
    return sc


def _open(c, **kw):
    """A SUBPIXEL | DIRECT_GRAY context of a case of tests/edge_frames.py; axis: the one coded axis, or None for the two-axis scan."""
    return _scanner(c["W"], c["H"], EF.PW, EF.PH, EF.N, EF.FW, c["cal"], full=c["full"], origin=c["origin"], **kw)


def _frames(sc, planes, axis, view=0, N=EF.N, n_fringe=3, whole=False):
    """The F + N planes a flagged context reads, per coded axis (whole: all F + 2 N, for a context without the flag)."""
    for a in _axes(axis):
        sc.set_frames(a, planes[a] if whole else DG.read_planes(planes[a], n_fringe, N[a]), view=view)


def _out(sc, axis, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid) if axis is not None else dict(points=xyz, valid=valid, residual=sc.residuals(view))


def _timed_checks(sc, axis, anchored, launches=1):
    name = NAMES[(axis, anchored)]
    assert sc.last_fused_kernel_name() == name and sc.fused_kernel_name(1) == name and sc.fused_kernel_name(3) == name
    assert sc.launch_counts() == (launches, 0) and sc.camera_table_bytes_per_pixel(1) == 0


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(name, shape, p, rig_axis):
    """EF.oracle_scan on the as_inverse_coded() planes of the case: the stage planes of a flagged context."""
    c = EF.case(name, shape, p, rig_axis)
    coded = [DG.as_inverse_coded(c["planes"][a], 3, EF.N[a]) for a in (0, 1)]
    o = Oracle(c["W"], c["H"], EF.PW, EF.PH, EF.N[0], EF.N[1], EF.FW[0], EF.FW[1], col0=c["origin"][0], row0=c["origin"][1])
    o.set_mask(EF.window(c["mask"], shape))
    o.set_calibration(*c["cal"])
    o.run_scan(*coded)
    A, B = o.projection_matrices()
    out = dict(w=(o.wrapped_phi(0), o.wrapped_phi(1)), code=(o.code(0), o.code(1)), unw=(o.unwrapped_phi(0), o.unwrapped_phi(1)),
               valid_axis=(o.valid_map(0), o.valid_map(1)), valid=o.valid_map(2), c_p_map=o.c_p_map(), ipoints=o.intersection_points(), A_cam=A, A_proj=B)
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def _restated(name, shape, p, axis, anchored):
    rig_axis = 0 if axis is None else axis
    c, o = EF.case(name, shape, p, rig_axis), _oracle(name, shape, p, rig_axis)
    if axis is not None:
        return OR.scan(o["w"][axis], o["code"][axis], o["unw"][axis], o["valid_axis"][axis], c["cal"], o["A_cam"], o["A_proj"], axis, EF.FW[axis], EF.EXTENT[axis],
                       EF.N[axis], 3, c["origin"], c["full"], anchored)
    xy = AR.correspondences(o["w"], o["code"], o["unw"], o["valid_axis"], EF.FW, 3, EF.N, c["origin"], c["full"]) if anchored else \
        SR.correspondences(*o["unw"], *o["valid_axis"], *EF.FW)
    return dict(SR.triangulate(xy, o["valid"], c["cal"], o["A_cam"], o["A_proj"], c["origin"]), xy=xy)


def _compare_stage_planes(sc, c, o, a, mask, inn, what):
    """One axis of the stage planes against the oracle's, on the pixels `inn` of the window; the code against the restatement itself."""
    va = (o["valid_axis"][a] == 1) & inn
    code = sc.code(a)
    assert np.array_equal(sc.valid_map(a)[inn], o["valid_axis"][a][inn]), f"{what}: valid map axis {a}"
    assert np.array_equal(code[inn], o["code"][a][inn]), f"{what}: code axis {a}"
    sel = sc.valid_map(a) == 1
    assert np.array_equal(code[sel], DG.code_of_planes(c["planes"][a], 3, EF.N[a])[sel]) and (code[~sel] == -1).all(), f"{what}: code axis {a} against the restatement"
    where = (mask == 1) & inn
    assert np.array_equal(_bits(sc.wrapped_phase(a))[where], _bits(o["w"][a])[where]), f"{what}: wrapped phase axis {a}"
    assert np.array_equal(_bits(sc.unwrapped_phase(a))[va], _bits(o["unw"][a])[va]), f"{what}: unwrapped phase axis {a}"
    loop = AR.applies(a, code.shape, c["origin"], c["full"], 1)    # where stage 4's loop runs: elsewhere the absolute phase stays 0
    unw = sc.unwrapped_phase(a)
    assert np.array_equal(_bits(unw)[sel & loop], _bits(DG.absolute(sc.wrapped_phase(a), code))[sel & loop]) and (unw[sel & ~loop] == 0).all(), \
        f"{what}: the absolute phase is stage 4's float of the shifted phase and the direct code"


# ---- 1. / 5. the staged route against the restatement; the timed context against the staged route -------------------------------------------
@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,shape,p", EF.CASES, ids=CASE_IDS)
def test_edge_frames_against_the_restatement(name, shape, p, axis, anchored):
    what = (name, shape, p, axis, anchored)
    rig_axis = 0 if axis is None else axis
    c, o, want = EF.case(name, shape, p, rig_axis), _oracle(name, shape, p, rig_axis), _restated(name, shape, p, axis, anchored)
    inn, mask = EF.inner(shape), EF.window(c["mask"], shape)
    v = (want["valid"] == 1) & inn
    # where the two decodes differ, and where both are ties
    differ = [DG.code_of_planes(c["planes"][a], 3, EF.N[a]) != DG.inverse_code(*DG.split(c["planes"][a], 3, EF.N[a])[1:]) for a in _axes(axis)]
    if name.startswith("flat_"):
        assert not any(d.any() for d in differ), "a flat frame is a tie in both decodes: every bit 1"
    else:
        for d, a in zip(differ, _axes(axis)):
            sel = o["valid_axis"][a] == 1
            assert sel.any() and d[sel].mean() > 0.05, "the direct code is not the inverse-based one here"
    with _open(c, axis=axis, keep=True, anchored=anchored) as sc:
        _frames(sc, c["planes"], axis)
        sc.set_mask(c["mask"])
        for a in _axes(axis):
            sc.compute_wrapped_phase(a)
        for a in _axes(axis):
            sc.unwrap_phase(a)
        for a in _axes(axis):
            _compare_stage_planes(sc, c, o, a, mask, inn, what)
        sc.compute_c_p_map()
        valid5, cp = sc.valid_map(), sc.c_p_map()
        xy = sc.correspondences_subpixel()
        counts = sc.triangulate_subpixel()
        staged = _out(sc, axis)
        ip = sc.intersection_points()
        stage4 = [(sc.code(a), sc.wrapped_phase(a), sc.unwrapped_phase(a)) for a in _axes(axis)]
        # sl3d_run of the same context enqueues the staged route itself (never the parity kernel, which reads the inverse planes)
        sc.run()
        _same(_out(sc, axis), staged, (what, "sl3d_run on the KEEP_STAGES context"))
        assert np.array_equal(sc.c_p_map(), cp) and np.array_equal(_bits(sc.intersection_points()), _bits(ip)) and np.array_equal(_bits(sc.correspondences_subpixel()), _bits(xy))
        for a, planes in zip(_axes(axis), stage4):
            for got, before in zip((sc.code(a), sc.wrapped_phase(a), sc.unwrapped_phase(a)), planes):
                assert np.array_equal(_bits(got), _bits(before)), (what, "the stage getters after sl3d_run", a)
    assert np.array_equal(valid5[inn], want["valid"][inn]) and np.array_equal(staged["valid"][inn], want["valid"][inn]), "merged valid map"
    if axis is None:
        assert np.array_equal(cp[v], o["c_p_map"][v]), "c_p_map"
    else:
        assert np.array_equal(cp[inn], want["c_p_map"][inn]), "c_p_map"
    assert counts == [(int((staged["valid"] == 1).sum()), 0)]
    nan = np.isnan(want["xy"])
    assert np.array_equal(np.isnan(xy)[inn], nan[inn]), "NaN pattern of the coordinates"
    ok = ~nan & inn[..., None]
    assert np.array_equal(_bits(xy)[ok], _bits(want["xy"])[ok]), (int((_bits(xy)[ok] != _bits(want["xy"])[ok]).sum()), "coordinates differ")
    on = staged["valid"] == 1
    assert np.array_equal(np.isnan(staged["points"]).any(-1), ~on) and np.array_equal(np.isnan(staged["points"]).all(-1), ~on)
    ulps = float(scaled_ulps(staged["points"][v], want["ipoints"][v]).max()) if v.any() else 0.0
    e_f = assert_points_close(staged["points"], want["ipoints"], v)
    e_d = assert_points_close(ip, want["ipoints"], v)
    print(f"{what}: {int(v.sum())} valid of {int(inn.sum())} compared, points {e_f:.2e} rel, {ulps:.2f} scaled ulps, intersection_points {e_d:.2e} rel")
    assert ulps <= BAR_ULPS
    assert np.array_equal(_bits(staged["points"][on]), _bits(ip[on].astype(np.float32))), "points are the float cast of intersection_points"
    if axis is None:
        assert np.array_equal(np.isnan(staged["residual"]), ~on)
        ref = want["residual"][v].astype(np.float64)
        err = np.abs(staged["residual"][v].astype(np.float64) - ref)
        assert (err <= 1e-6 * ref + 1e-7).all(), (float(err.max()), "residuals")
    if inn.all() and not (want["valid"] == 1).any():
        assert _nothing(staged), "nothing is valid"
    with _open(c, axis=axis, anchored=anchored) as sc:                # the timed context: one launch of k_direct_gray
        assert sc.fused_kernel_name(1) == NAMES[(axis, anchored)]
        _frames(sc, c["planes"], axis)
        sc.set_mask(c["mask"])
        sc.run()
        _same(_out(sc, axis), staged, what)
        _timed_checks(sc, axis, anchored)


# ---- 2. / 4. every timed instantiation against the staged route, over the configurations -----------------------------------------------------
# n_fringe, Gray planes (v, h), fringe widths (v, h), noise -- on a 128 x 96 projector: fw * 2^N covers the extent in each
CONFIGS = {
    "five_step": (5, (5, 5), (4, 4), 0),
    "four_step": (4, (5, 5), (4, 4), 0),
    "no_gray": (3, (0, 0), (128, 96), 0),
    "one_plane": (3, (1, 1), (64, 48), 0),
    "sixteen_planes": (3, (16, 16), (4, 4), 0),
    "unequal_axes_noise": (3, (5, 6), (4, 2), 2),
    "unequal_axes_four_step_noise": (4, (6, 5), (2, 4), 2),
}


@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", CONFIGS)
def test_timed_instantiations_over_the_configurations(name, axis, anchored):
    F, N, FW, noise = CONFIGS[name]
    W, H, PW, PH = 90, 60, 128, 96                               # (90 columns: a 96-column pitch, the last quad of a row half outside the window)
    syn = pkg("synth")
    cap = syn.make_capture(W, H, PW, PH, N[0], N[1], FW[0], FW[1], cal=EF.rig(0 if axis is None else axis, W, H, PW, PH), n_fringe=F, noise=noise)
    cal, planes = syn.cal_tuple(cap["cal"]), (cap["planes_v"], cap["planes_h"])
    kw = dict(axis=axis, anchored=anchored, n_fringe=F)
    with _scanner(W, H, PW, PH, N, FW, cal, keep=True, **kw) as sc:
        _frames(sc, planes, axis, N=N, n_fringe=F)
        sc.set_mask(cap["mask"])
        sc.run()
        staged = _out(sc, axis)
        stage4 = {}
        for a in _axes(axis):
            sel = sc.valid_map(a) == 1
            code = sc.code(a)
            assert np.array_equal(code[sel], DG.code_of_planes(planes[a], F, N[a])[sel]) and (code[~sel] == -1).all(), (name, "the stage getter shows the direct code", a)
            stage4[a] = (code, sc.wrapped_phase(a), sc.unwrapped_phase(a), sc.debug_image(4, a), sc.valid_map(a))
    with _scanner(W, H, PW, PH, N, FW, cal, **kw) as sc:
        _frames(sc, planes, axis, N=N, n_fringe=F)
        sc.set_mask(cap["mask"])
        sc.run()
        timed = _out(sc, axis)
        _timed_checks(sc, axis, anchored)
    _same(timed, staged, (name, axis, anchored))
    if F == 5:
        assert _nothing(timed), "with five steps nothing is valid"
    else:
        _sane(staged, (name, axis, anchored))
        assert (staged["valid"] == 1).sum() > 1000
    if noise == 0:                                                # the flagged scan is the unflagged scan of the same context flags
        for a in _axes(axis):
            if N[a]:
                assert np.array_equal(DG.code_of_planes(planes[a], F, N[a]), DG.inverse_code(*DG.split(planes[a], F, N[a])[1:])), "the condition: without noise the codes agree"
        with _scanner(W, H, PW, PH, N, FW, cal, direct=False, **kw) as sc:
            _frames(sc, planes, axis, whole=True)
            sc.set_mask(cap["mask"])
            sc.run()
            assert sc.last_fused_kernel_name() == UNFLAGGED[(axis, anchored)]
            _same(_out(sc, axis), timed, (name, axis, anchored, "the unflagged scan"))
        # ... and k_unwrap_direct leaves what k_unwrap leaves, plane by plane: the two kernels share their text but for the bit
        with _scanner(W, H, PW, PH, N, FW, cal, keep=True, direct=False, **kw) as sc:
            _frames(sc, planes, axis, whole=True)
            sc.set_mask(cap["mask"])
            for a in _axes(axis):
                sc.compute_wrapped_phase(a)
                sc.unwrap_phase(a)
                got = (sc.code(a), sc.wrapped_phase(a), sc.unwrapped_phase(a), sc.debug_image(4, a), sc.valid_map(a))
                for g, w, what in zip(got, stage4[a], ("code", "wrapped phase", "absolute phase", "stage 4's debug image", "valid map")):
                    assert np.array_equal(_bits(g), _bits(w)), (name, axis, a, what, "k_unwrap_direct against k_unwrap")


# ---- 2c. per-view masks in one launch, three views behind an untouched slot ------------------------------------------------------------------
def _alone(c, axis, anchored, planes, select, eager):
    with _open(c, axis=axis, anchored=anchored, eager_mask=eager) as sc:
        _frames(sc, planes, axis)
        sc.set_mask(select)
        sc.run()
        return _out(sc, axis)


def _modulated_selection(c, axis, planes, mask, thr):
    with _open(c, axis=axis) as sc:
        _frames(sc, planes, axis)
        gammas = [sc.modulation(a) for a in _axes(axis)]
    select = mask == 1
    with np.errstate(invalid="ignore"):
        for g in gammas:
            select = select & (g.astype(np.float64) > thr)
    return select.astype(np.uint8)


@pytest.mark.parametrize("mode", ["eager", "modulated"])
@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
def test_per_view_masks_in_one_launch(axis, anchored, mode):
    rig_axis = 0 if axis is None else axis
    c = EF.case("flat_17", "base", 1.0, rig_axis)               # (the shape and the calibration of the base case)
    caps, (A, B, C) = EF.view_captures(rig_axis), EF.view_masks()
    eager = mode == "eager"
    thr = None
    if not eager:                                               # a threshold from the gammas the device reports: the tenth part of the pixels fails it
        with _open(c, axis=axis) as sc:
            pooled = []
            for planes in caps:
                _frames(sc, planes, axis)
                pooled += [sc.modulation(a) for a in _axes(axis)]
        pooled = np.stack(pooled)
        thr = float(np.quantile(pooled[np.isfinite(pooled)].astype(np.float64), 0.1))

    def yardstick(view, mask):
        return _alone(c, axis, anchored, caps[view], mask if eager else _modulated_selection(c, axis, caps[view], mask, thr), eager)

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
        assert sc.last_fused_kernel_name() == NAMES[(axis, anchored)]
        for v in want:
            _same(_out(sc, axis, v), want[v], ("run(1, 3)", v))
        assert sc.run_timed(1, 3) > 0
        for v in want:
            _same(_out(sc, axis, v), want[v], ("run_timed(1, 3)", v))
        set_masks(sc, {1: C, 3: A})
        sc.run(1, 3)
        for v in swapped:
            _same(_out(sc, axis, v), swapped[v], ("run(1, 3) after A and C changed places", v))
        after = sc.points(0)
        assert np.array_equal(after[1], slot0[1]) and np.array_equal(_bits(after[0]), _bits(slot0[0])), "slot 0 is untouched"
        assert sc.launch_counts()[1] == 0


# ---- 3. the inverse slots are never read -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True], ids=["timed", "staged"])
@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
def test_the_inverse_slots_are_never_read(axis, keep):
    name, shape, p = "noise3", "base", 1.0
    c = EF.case(name, shape, p, 0 if axis is None else axis)
    rng = np.random.default_rng(7)
    with _open(c, axis=axis, keep=keep, anchored=True) as sc:
        _frames(sc, c["planes"], axis)
        sc.set_mask(c["mask"])
        sc.run()
        want = _out(sc, axis)
        _sane(want, (axis, keep))
        for fill in ("random", "correct"):
            for a in _axes(axis):
                n = EF.N[a]
                inv = list(rng.integers(0, 256, (n, c["H"], c["W"]), dtype=np.uint8)) if fill == "random" else DG.split(c["planes"][a], 3, n)[2]
                sc.set_frames_range(a, 3 + n, inv)
            sc.run()
            _same(_out(sc, axis), want, (axis, keep, fill))
        for a in _axes(axis):                                    # ... and the frame stack holds what was set: F + 2 N planes per axis, as always
            assert all(np.array_equal(g, f) for g, f in zip(sc.frames(a), c["planes"][a]))


# ---- 6. sl3d_process_views with NULL inverse pointers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
def test_process_views_with_null_inverse_pointers(axis):
    c = EF.case("noise3", "base", 1.0, 0 if axis is None else axis)
    caps = EF.view_captures(0 if axis is None else axis)
    mask = EF.window(c["mask"], "base")
    want = [_alone(c, axis, True, planes, mask, False) for planes in caps]
    assert len({w["points"].tobytes() for w in want}) == 3

    def listed(planes):
        """planes_per_view entries: the planes the context reads, None for the inverse planes and for the axis it does not code."""
        out = []
        for a in (0, 1):
            fr, gray, inv = DG.split(planes[a], 3, EF.N[a])
            out += (fr + gray if a in _axes(axis) else [None] * (3 + EF.N[a])) + [None] * EF.N[a]
        return out

    with _open(c, axis=axis, anchored=True, max_views=2) as sc:   # three views through two slots
        for v in range(2):
            sc.set_mask(c["mask"], view=v)
        assert sc.device_buffers().planes_per_view == len(listed(caps[0])) == 6 + 2 * sum(EF.N)
        xyz, valid = sc.process_views([listed(p) for p in caps])
        for v, w in enumerate(want):
            got = dict(points=xyz[v], valid=valid[v])           # (process_views hands out points and valid)
            _same(got, {k: w[k] for k in got}, ("process_views", v))
        assert sc.last_fused_kernel_name() == NAMES[(axis, True)]
        a = _axes(axis)[0]
        up = sc.frames(a, view=0)                                  # slot 0 holds view 2: its F + N planes went up
        assert all(np.array_equal(g, f) for g, f in zip(up[:3 + EF.N[a]], caps[2][a]))
        broken = listed(caps[0])
        broken[(0 if a == 0 else 3 + 2 * EF.N[0]) + 3] = None      # a NULL Gray plane of a coded axis is still refused
        with pytest.raises(pkg("scanner").Sl3dError) as e:
            sc.process_views([broken])
        assert "null plane" in str(e.value)


@pytest.mark.parametrize("axis", MODES, ids=MODE_IDS)
def test_process_views_uploads_a_contiguous_view_in_one_copy_per_axis(axis):
    """A 4-D array whose rows are the device's own pitch (96 columns): the planes of a view are back to back, so the F + N planes of each
    coded axis go up as ONE copy -- and the inverse slots between and behind them are not written."""
    W, H, PW, PH, N, FW = 96, 60, 128, 96, (5, 6), (4, 2)
    syn = pkg("synth")
    caps = [syn.make_capture(W, H, PW, PH, N[0], N[1], FW[0], FW[1], cal=EF.rig(0 if axis is None else axis, W, H, PW, PH), noise=2, view=v, plane=pl)
            for v, pl in enumerate(EF.VIEW_PLANES)]
    cal = syn.cal_tuple(caps[0]["cal"])
    want = []
    for cap in caps:
        with _scanner(W, H, PW, PH, N, FW, cal, axis=axis, anchored=True) as sc:
            _frames(sc, (cap["planes_v"], cap["planes_h"]), axis, N=N)
            sc.set_mask(cap["mask"])
            sc.run()
            want.append(_out(sc, axis))
        _sane(want[-1], "a view alone")
    rng = np.random.default_rng(9)
    ppv = 6 + 2 * sum(N)
    stack = rng.integers(0, 256, (3, ppv, H, W), dtype=np.uint8)   # random bytes wherever the context does not read
    base = (0, 3 + 2 * N[0])
    for v, cap in enumerate(caps):
        for a in _axes(axis):
            stack[v, base[a]:base[a] + 3 + N[a]] = np.stack(DG.read_planes((cap["planes_v"], cap["planes_h"])[a], 3, N[a]))
    marker = np.full((H, W), 0x5C, np.uint8)
    with _scanner(W, H, PW, PH, N, FW, cal, axis=axis, anchored=True, max_views=2) as sc:
        b = sc.device_buffers()
        assert b.frame_pitch == W == stack.strides[2] and b.plane_stride == W * H == stack.strides[1] and b.planes_per_view == ppv, "the one-copy condition holds"
        for v in range(2):
            sc.set_mask(caps[0]["mask"], view=v)
            for a in (0, 1):
                sc.set_frames(a, [marker] * (3 + 2 * N[a]), view=v)
        xyz, valid = sc.process_views(stack)
        for v, w in enumerate(want):
            got = dict(points=xyz[v], valid=valid[v])
            _same(got, {k: w[k] for k in got}, ("process_views", v))
        assert sc.last_fused_kernel_name() == NAMES[(axis, True)]
        for a in (0, 1):                                         # slot 0 holds view 2: its read planes went up, nothing else was written
            up = sc.frames(a, view=0)
            n_up = 3 + N[a] if a in _axes(axis) else 0
            assert all(np.array_equal(g, stack[2, base[a] + i]) for i, g in enumerate(up[:n_up])), ("the planes read", a)
            assert all(np.array_equal(g, marker) for g in up[n_up:]), ("the slots not read keep what they held", a)


# ---- 7. groups of three stripes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, 0], ids=["two_axes", "vertical"])
def test_group_of_three_stripes(axis):
    S = pkg("scanner")
    c = EF.case("noise3", "base", 1.0, 0)
    planes, mask = c["planes"], EF.window(c["mask"], "base")
    single = _alone(c, axis, True, planes, mask, False)
    _sane(single, "the single context")
    W, H = c["W"], c["H"]
    rng = np.random.default_rng(3)
    flags = S.SL3D_FLAG_SUBPIXEL | S.SL3D_FLAG_ANCHOR_PERIODS | S.SL3D_FLAG_DIRECT_GRAY | (S.SL3D_FLAG_ONLY_VERTICAL if axis == 0 else 0)
    with S.Group(W, H, EF.PW, EF.PH, EF.N[0], EF.N[1], EF.FW[0], EF.FW[1], devices=[0, 0, 0], flags=flags) as g:
        stripes = g.stripes()
        assert len(stripes) == 3
        row0, rows = stripes[1][0], stripes[1][1]
        assert 0 < row0 and row0 + rows < H and (single["valid"][row0] == 1).any() and (single["valid"][row0 + rows - 1] == 1).any()
        g.set_calibration(*c["cal"])
        for a in _axes(axis):                                     # (sl3d_group_set_frames takes F + 2 N planes: the inverse slots get random bytes)
            g.set_frames(a, DG.read_planes(planes[a], 3, EF.N[a]) + list(rng.integers(0, 256, (EF.N[a], H, W), dtype=np.uint8)))
        g.set_mask(mask)
        g.run()
        xyz, valid = g.download_points()
        assert np.array_equal(valid[0], single["valid"]) and np.array_equal(_bits(xyz[0]), _bits(single["points"])), "download_points"
        g.gather()
        xyz, valid = g.points()
        assert np.array_equal(valid, single["valid"]) and np.array_equal(_bits(xyz), _bits(single["points"])), "gather + get_points"
        with pytest.raises(S.Sl3dError):
            g.run_clouds()
        # sl3d_group_process_views: NULL for every plane the stripes do not read
        listed = []
        for a in (0, 1):
            listed += (DG.read_planes(planes[a], 3, EF.N[a]) if a in _axes(axis) else [None] * (3 + EF.N[a])) + [None] * EF.N[a]
        xyz, valid = g.process_views([listed])
        assert np.array_equal(valid[0], single["valid"]) and np.array_equal(_bits(xyz[0]), _bits(single["points"])), "group_process_views"
        g.synchronize()


# ---- 8. sl3d_repair_periods on a flagged KEEP_STAGES context ---------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_repair_periods_on_the_direct_code(axis):
    """The repair touches the code and phase planes only: on a flagged context it repairs the DIRECT code (not anchored: the repair and the
    anchoring exclude each other).  tests/test_gpu_repair_edges.py does the same on random / base / 0.9 and steps / base / 0.9."""
    c = EF.case("noise3", "base", 1.0, 0)
    with _open(c, axis=None, keep=True) as sc:
        _frames(sc, c["planes"], None)
        sc.set_mask(c["mask"])
        for a in (0, 1):
            sc.compute_wrapped_phase(a)
            sc.unwrap_phase(a)
        sel = sc.valid_map(axis) == 1
        assert np.array_equal(sc.code(axis)[sel], DG.code_of_planes(c["planes"][axis], 3, EF.N[axis])[sel])
        rep, unrep = check_pass(sc, EF.N[axis], axis, 4, what="the direct code")
        print(f"axis {axis}: {rep} repaired, {unrep} unrepairable of {int(sel.sum())} selected")
        assert rep > 0


# ---- 9. the kernel names ---------------------------------------------------------------------------------------------------------------------
def test_kernel_names_tell_the_instantiations_apart():
    c = EF.case("random", "64x5", 0.5)
    seen = set()
    for (axis, anchored), want in NAMES.items():
        with _open(c, axis=axis, anchored=anchored) as sc:
            _frames(sc, c["planes"], axis)
            sc.set_mask(c["mask"])
            with pytest.raises(pkg("scanner").Sl3dError):
                sc.last_fused_kernel_name()                       # no launch yet
            assert sc.fused_kernel_name(1) == want
            with pytest.raises(pkg("scanner").Sl3dError):
                sc.fused_kernel_name(1, clouds=True)
            assert sc.L.sl3d_run_clouds(sc._h, 0, 1) == -5        # refused as on every SUBPIXEL context
            sc.run()
            assert sc.last_fused_kernel_name() == want
            seen.add(want)
    assert len(seen) == 6 and all(n.startswith("sl3d::k_direct_gray<") for n in seen)
    with _open(c, axis=None, direct=False) as sc:                # a context without the flag reports what it always did
        assert sc.fused_kernel_name(1) == UNFLAGGED[(None, False)]


# ---- 10. what it is for: 13 frames against 23 ------------------------------------------------------------------------------------------------
def test_a_13_frame_scan_is_as_accurate_as_the_23_frame_scan():
    """The headline configuration on the device: 3 phase-shift + 10 Gray-code frames.  320 x 240 camera, 2048 x 1536 projector, N = 10, fringe
    width 2, noise +-2, vertical only, anchored: the timed scan of a flagged context that holds 13 frames against the timed scan of an
    unflagged context that holds all 23 -- the same points on every good pixel of the two-axis scan, so the same RMS to the true plane."""
    import subpixel_cases as SC
    syn = pkg("synth")
    W, H, PW, PH, N, FW = 320, 240, 2048, 1536, (10, 10), (2, 2)
    cap = syn.make_capture(W, H, PW, PH, N[0], N[1], FW[0], FW[1], noise=2)
    cal, planes = syn.cal_tuple(cap["cal"]), (cap["planes_v"], cap["planes_h"])
    assert len(planes[0]) == 23 and len(DG.read_planes(planes[0], 3, 10)) == 13
    with _scanner(W, H, PW, PH, N, FW, cal, axis=None, keep=True, anchored=True, direct=False) as sc:     # the two-axis scan: where to measure
        _frames(sc, planes, None, whole=True)
        sc.set_mask(cap["mask"])
        sc.run()
        good = SC.good_pixels(cap, sc.c_p_map(), sc.valid_map())
    assert good.sum() > 0.5 * cap["lit"].sum()
    out = {}
    for direct in (False, True):
        with _scanner(W, H, PW, PH, N, FW, cal, axis=0, anchored=True, direct=direct) as sc:
            _frames(sc, planes, 0, N=N, whole=not direct)
            sc.set_mask(cap["mask"])
            sc.run()
            assert sc.last_fused_kernel_name() == (NAMES if direct else UNFLAGGED)[(0, True)]
            out[direct] = _out(sc, 0)
        assert (out[direct]["valid"] == 1)[good].all()
    assert np.array_equal(_bits(out[True]["points"])[good], _bits(out[False]["points"])[good])
    rms13, rms23 = SC.plane_rms(out[True]["points"], good), SC.plane_rms(out[False]["points"], good)
    print(f"RMS to the plane over {int(good.sum())} pixels: {rms13:.6f} mm from 13 frames, {rms23:.6f} mm from 23 frames")
    assert rms13 == rms23 and rms13 < 0.1
