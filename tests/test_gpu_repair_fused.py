"""GPU tests (-m gpu) of SL3D_FLAG_REPAIR_PERIODS: sl3d_run on a flagged context leaves the period-repaired scan.

The yardstick is the staged route on a SL3D_FLAG_KEEP_STAGES context with the same configuration, calibration, masks and frames:
sl3d_compute_wrapped_phase + sl3d_unwrap_phase of both axes, sl3d_repair_periods(view, axis, 4) once for each axis that has Gray planes,
sl3d_compute_c_p_map, then sl3d_triangulate -- or, in sub-pixel mode, sl3d_triangulate_subpixel(+inf, NULL).
tests/test_gpu_period_repair.py holds that route against the NumPy restatement.  "Equal" is equality of the bit patterns, NaNs included,
of the points and valid planes (sub-pixel mode: and the residual plane) over EVERY pixel of the window.  The captures are those of
tests/period_cases.py; tests/test_repair_fused_cases.py asserts that they cover every seam of the new kernel's tile.  Every yardstick is
computed once and checked for what it is there for BEFORE a device result is compared with it: the staged call reports repaired pixels,
and the repaired scan differs from the unrepaired one of the same context.
What these smooth captures cannot see -- random and flat frames, ragged sizes, a mask holding the value 2, per-view masks at the tile's
seams, sl3d_set_masks_modulated -- is in tests/test_gpu_repair_edges.py."""
import functools

import numpy as np
import pytest

from conftest import pkg

import period_cases as PC

pytestmark = pytest.mark.gpu

RADIUS = 4
MODES = ("integer", "subpixel")
NAMES = {"integer": "sl3d::k_repair_fused<false>", "subpixel": "sl3d::k_repair_fused<true>"}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _open(case, *, keep=False, repaired=False, subpixel=False, max_views=1, eager_mask=False):
    S, syn = pkg("scanner"), pkg("synth")
    sc = S.Scanner(case["W"], case["H"], case["PW"], case["PH"], case["N"], case["N"], PC.FW, PC.FW, keep_stages=keep, full_size=case["full"],
                   origin=case["origin"], max_views=max_views, repaired=repaired, subpixel=subpixel, eager_mask=eager_mask)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(case["full"][0], case["full"][1], case["PW"], case["PH"])))
    return sc


def _frames(sc, case, view=0):
    sc.set_frames(0, case["planes_v"], view=view)
    sc.set_frames(1, case["planes_h"], view=view)


def _load(sc, case, view=0):
    sc.set_mask(case["mask"], view=view)
    _frames(sc, case, view)


def _out(sc, mode, view=0):
    xyz, valid = sc.points(view)
    out = dict(points=xyz, valid=valid)
    if mode == "subpixel":
        out["residual"] = sc.residuals(view)
    return out


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _differ(a, b):
    return any(not np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _sane(want, what, some_valid=True):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1} and v.any() == some_valid, what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v), what
    if "residual" in want:
        assert np.array_equal(np.isnan(want["residual"]), ~v), what


def _staged(sc, view=0, repair=True, axes=(0, 1)):
    """The staged route over one view of a KEEP_STAGES context; axes: those that have Gray planes.  Returns {mode: planes}, the counts per
    axis (None where the axis was not repaired) and the repaired code planes."""
    for a in (0, 1):
        sc.compute_wrapped_phase(a, view)
    for a in (0, 1):
        sc.unwrap_phase(a, view)
    counts = [sc.repair_periods(a, RADIUS, view) if repair and a in axes else None for a in (0, 1)]
    codes = [sc.code(a, view) for a in (0, 1)]
    sc.compute_c_p_map(view)
    assert sc.triangulate_subpixel(view, 1, want_counts=False) is None
    outs = {"subpixel": _out(sc, "subpixel", view)}
    sc.triangulate(view)
    outs["integer"] = _out(sc, "integer", view)
    return outs, counts, codes


def _make(name):
    kind, _, arg = name.partition(":")
    if kind in PC.GRID_CASES:
        return PC.make_grid_case(kind, control=arg == "control")
    if kind == "fuzz":
        return PC.make_fuzz_case(int(arg))
    if kind == "jacobi":
        return PC.make_jacobi_case()
    if kind == "wide":
        return PC.make_wide_case()
    return PC.make_case(kind, int(arg))


@functools.lru_cache(maxsize=None)
def _case(name):
    return _make(name)


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """Per capture, computed once and left unchanged: the staged route without and with the repair, on one KEEP_STAGES context."""
    case = _case(name)
    with _open(case, keep=True) as sc:
        _load(sc, case)
        raw, _, raw_codes = _staged(sc, repair=False)
        want, counts, codes = _staged(sc)
    for mode in MODES:
        _sane(want[mode], (name, mode))
    return dict(raw=raw, want=want, counts=counts, raw_codes=raw_codes, codes=codes)


# name: (repaired pixels expected on the vertical axis, on the horizontal axis, unrepairable pixels expected)
CASES = {
    "grid": (True, True, True), "sliver": (True, True, True), "grid_window": (True, True, True),
    "jacobi": (True, False, False),
    "wide": (True, False, False),                       # |j| = 128: no byte plane to overflow in the fused kernel
    "border_lo_v:2": (True, False, True), "border_hi_v:-2": (True, False, True),      # the unrepairable branch, both ends, both axes
    "border_lo_h:2": (False, True, True), "border_hi_h:-2": (False, True, True),
    "mask_v:2": (True, False, False), "mask_v:-2": (True, False, False),              # runs of n < 5 samples between the holes
    "mask_h:2": (False, True, False), "mask_h:-2": (False, True, False),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_run_equals_the_staged_route(name, mode):
    case, y = _case(name), _yardstick(name)
    rep_v, rep_h, unrep = CASES[name]
    # the yardstick first: it repairs what the case is for, and the repair shows in the scan
    assert (y["counts"][0][0] > 0) == rep_v and (y["counts"][1][0] > 0) == rep_h, (name, y["counts"])
    assert (y["counts"][0][1] + y["counts"][1][1] > 0) == unrep, (name, y["counts"])
    assert _differ(y["want"][mode], y["raw"][mode]), "the repaired scan is not the unrepaired scan"
    if name == "wide":
        assert np.abs(y["codes"][0].astype(np.int64) - y["raw_codes"][0]).max() >= 128
    with _open(case, repaired=True, subpixel=mode == "subpixel") as sc:
        assert sc.fused_kernel_name(1) == NAMES[mode]
        assert sc.camera_table_bytes_per_pixel(1) == 0
        _load(sc, case)
        sc.run()
        _same(_out(sc, mode), y["want"][mode], (name, mode))
        assert sc.last_fused_kernel_name() == NAMES[mode]
        assert sc.launch_counts() == (1, 0)


@pytest.mark.parametrize("mode", MODES)
def test_nothing_to_repair_is_the_unflagged_route(mode):
    """The control capture of `grid` -- no line shifted, no point error: the flagged run equals the staged route WITHOUT the repair."""
    name = "grid:control"
    case, y = _case(name), _yardstick(name)
    assert y["counts"][0][0] == 0 and y["counts"][1][0] == 0
    _same(y["want"][mode], y["raw"][mode], "the yardstick of the control")
    with _open(case, repaired=True, subpixel=mode == "subpixel") as sc:
        _load(sc, case)
        sc.run()
        _same(_out(sc, mode), y["raw"][mode], (name, mode))
    assert _differ(_yardstick("grid")["want"][mode], y["raw"][mode]), "the capture with errors is another scan"


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_yardstick():
    cases = [_case(f"fuzz:{seed}") for seed in PC.FUZZ_SEEDS]
    with _open(cases[0], keep=True, max_views=3) as sc:
        for v, c in enumerate(cases):
            _load(sc, c, view=v)
        staged = [_staged(sc, view=v) for v in range(3)]
        _frames(sc, cases[2], view=1)                           # view 1: its own mask over view 2's frames
        swapped = _staged(sc, view=1)
    for outs, counts, _ in staged + [swapped]:
        assert counts[0][0] > 0 and counts[1][0] > 0
    return [s[0] for s in staged], swapped[0]


@pytest.mark.parametrize("eager_mask", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_batches_and_the_views_outside_a_launch(mode, eager_mask):
    cases = [_case(f"fuzz:{seed}") for seed in PC.FUZZ_SEEDS]
    want, swapped = _batch_yardstick()
    assert len({w[mode]["points"].tobytes() for w in want}) == 3, "the views must differ"
    assert _differ(swapped[mode], want[1][mode]) and _differ(swapped[mode], want[2][mode])
    with _open(cases[0], repaired=True, subpixel=mode == "subpixel", max_views=3, eager_mask=eager_mask) as sc:
        for v, c in enumerate(cases):
            _load(sc, c, view=v)
        sc.run(0, 3)                                            # (without eager_mask: behind the preparation of three deferred masks)
        first = [_out(sc, mode, v) for v in range(3)]
        for v in range(3):
            _same(first[v], want[v][mode], ("run(0, 3)", v))
        _frames(sc, cases[2], view=1)
        sc.run(1, 1)
        _same(_out(sc, mode, 1), swapped[mode], "run(1, 1) over changed frames")
        for v in (0, 2):
            _same(_out(sc, mode, v), first[v], ("view", v, "outside run(1, 1)"))
        assert sc.launch_counts() == (2, 0)


# ---- the configurations the one kernel must cover -----------------------------------------------------------------------------------------
CONFIGS = {
    "unequal_axes": dict(n_fringe=3, nv=5, nh=3),
    "no_gray_v": dict(n_fringe=3, nv=3, nh=3, drop=0),          # N = 0 on the vertical axis: skipped, the horizontal one is repaired
    "no_gray_h": dict(n_fringe=3, nv=3, nh=3, drop=1),
    "four_step": dict(n_fringe=4, nv=3, nh=3),
    "five_step": dict(n_fringe=5, nv=3, nh=3),                  # nothing is valid
}


@functools.lru_cache(maxsize=None)
def _config(name):
    """A 90 x 60 capture (a 96-column pitch: the last quad of a row half outside the window, two column tiles, four row tiles) whose Gray
    frames are moved by one camera pixel along the coded direction: the code edges no longer fall on the wraps.  The yardstick with it."""
    c = CONFIGS[name]
    W, H, PW, PH, FW = 90, 60, 128, 96, 16
    syn = pkg("synth")
    F, nv, nh = c["n_fringe"], c["nv"], c["nh"]
    cap = syn.make_capture(W, H, PW, PH, nv, nh, FW, FW, n_fringe=F)
    pv = cap["planes_v"][:F] + [np.ascontiguousarray(np.roll(p, 1, axis=1)) for p in cap["planes_v"][F:]]
    ph = cap["planes_h"][:F] + [np.ascontiguousarray(np.roll(p, 1, axis=0)) for p in cap["planes_h"][F:]]
    if c.get("drop") == 0:
        pv, nv = pv[:F], 0
    if c.get("drop") == 1:
        ph, nh = ph[:F], 0
    cfg = dict(size=(W, H, PW, PH, nv, nh, FW, FW), F=F, cal=syn.cal_tuple(cap["cal"]), mask=cap["mask"], planes_v=pv, planes_h=ph,
               axes=tuple(a for a, n in ((0, nv), (1, nh)) if n))
    with _config_open(cfg, keep=True) as sc:
        raw, _, _ = _staged(sc, repair=False)
        want, counts, _ = _staged(sc, axes=cfg["axes"])
    return cfg, dict(raw=raw, want=want, counts=counts)


def _config_open(cfg, **flags):
    sc = pkg("scanner").Scanner(*cfg["size"], n_fringe=cfg["F"], **{{"keep": "keep_stages"}.get(k, k): v for k, v in flags.items()})
    sc.set_calibration(*cfg["cal"])
    sc.set_mask(cfg["mask"])
    sc.set_frames(0, cfg["planes_v"])
    sc.set_frames(1, cfg["planes_h"])
    return sc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CONFIGS)
def test_configurations(name, mode):
    cfg, y = _config(name)
    five = cfg["F"] == 5
    _sane(y["want"][mode], name, some_valid=not five)
    for a in (0, 1):
        if a not in cfg["axes"]:
            assert y["counts"][a] is None                       # (the staged call refuses the axis: tests/test_gpu_period_repair.py)
        else:
            assert (y["counts"][a][0] > 0) == (not five), (name, a, y["counts"])
    assert _differ(y["want"][mode], y["raw"][mode]) == (not five)
    with _config_open(cfg, repaired=True, subpixel=mode == "subpixel") as sc:
        sc.run()
        got = _out(sc, mode)
        assert sc.last_fused_kernel_name() == NAMES[mode]
    _same(got, y["want"][mode], (name, mode))
    if five:
        assert (got["valid"] == 0).all() and all(np.isnan(got[k]).all() for k in got if k != "valid")
    else:
        assert (got["valid"] == 1).sum() > 1000, name


# ---- KEEP_STAGES | REPAIR_PERIODS -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_keep_stages_with_the_flag(mode):
    name = "grid_window"
    case, y = _case(name), _yardstick(name)
    assert any(not np.array_equal(y["codes"][a], y["raw_codes"][a]) for a in (0, 1))
    with _open(case, keep=True, repaired=True, subpixel=mode == "subpixel") as sc:
        _load(sc, case)
        sc.run()
        _same(_out(sc, mode), y["want"][mode], ("KEEP_STAGES | REPAIR_PERIODS", mode))
        assert sc.last_fused_kernel_name().startswith("sl3d::k_fused<true")
        for a in (0, 1):
            assert np.array_equal(sc.code(a), y["codes"][a]), ("the stage getters show the repaired code", a)
        sc.repair_periods(0, RADIUS)                            # the per-stage calls go on working behind it
        assert sc.launch_counts() == (1, 0)


# ---- the interface --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_flagged_timed_context():
    S = pkg("scanner")
    name = "border_lo_v:2"
    case, y = _case(name), _yardstick(name)
    with _open(case, repaired=True) as sc:
        L, h = sc.L, sc._h
        _load(sc, case)
        with pytest.raises(S.Sl3dError):
            sc.last_fused_kernel_name()                         # no launch yet
        sc.run()
        before = _out(sc, "integer")
        _same(before, y["want"]["integer"], "the run before the refusals")
        assert L.sl3d_run_clouds(h, 0, 1) == -5
        err = L.sl3d_last_error(h)
        assert b"sl3d_compact_views" in err and b"sl3d_run" in err and b"SL3D_FLAG_REPAIR_PERIODS" in err
        with pytest.raises(S.Sl3dError):
            sc.fused_kernel_name(1, clouds=True)
        assert b"sl3d_compact_views" in L.sl3d_last_error(h)
        assert L.sl3d_repair_periods(h, 0, 0, RADIUS, None) == -4 and b"KEEP_STAGES" in L.sl3d_last_error(h)
        assert L.sl3d_compute_wrapped_phase(h, 0, 0) == -4 and L.sl3d_unwrap_phase(h, 0, 0) == -4
        assert L.sl3d_compute_c_p_map(h, 0) == -4 and L.sl3d_triangulate(h, 0) == -4
        buf = np.zeros((case["H"], case["W"]), np.float32)
        assert L.sl3d_get_residuals(h, 0, buf.ctypes.data, case["W"]) == -4        # no SL3D_FLAG_SUBPIXEL: no residual plane
        _same(_out(sc, "integer"), before, "after the refusals")
        assert sc.launch_counts() == (1, 0)


def test_a_group_refuses_the_flag():
    S = pkg("scanner")
    case = _case("border_lo_h:2")
    for flags in (S.SL3D_FLAG_REPAIR_PERIODS, S.SL3D_FLAG_REPAIR_PERIODS | S.SL3D_FLAG_SUBPIXEL | S.SL3D_FLAG_KEEP_STAGES):
        with pytest.raises(S.Sl3dError) as e:
            S.Group(case["W"], case["H"], case["PW"], case["PH"], case["N"], case["N"], PC.FW, PC.FW, devices=[0, 0], flags=flags)
        text = str(e.value)
        assert "SL3D_FLAG_REPAIR_PERIODS" in text and "clipped" in text and "seam" in text, text


def test_run_timed_and_process_views_follow_run():
    cases = [_case(f"fuzz:{seed}") for seed in PC.FUZZ_SEEDS[:2]]
    want, _ = _batch_yardstick()
    with _open(cases[0], repaired=True, max_views=2) as sc:
        for v, c in enumerate(cases):
            _load(sc, c, view=v)
        assert sc.run_timed(0, 2) > 0
        for v in range(2):
            _same(_out(sc, "integer", v), want[v]["integer"], ("run_timed", v))
    with _open(cases[0], repaired=True, max_views=2) as sc:
        for v, c in enumerate(cases):
            sc.set_mask(c["mask"], view=v)
        frames = np.stack([np.stack(c["planes_v"] + c["planes_h"]) for c in cases])
        xyz, valid = sc.process_views(frames)
        for v in range(2):
            assert np.array_equal(valid[v], want[v]["integer"]["valid"]) and np.array_equal(_bits(xyz[v]), _bits(want[v]["integer"]["points"])), v
        assert sc.last_fused_kernel_name() == NAMES["integer"]


def test_consumers_see_the_repaired_scan():
    name = "grid"
    case, y = _case(name), _yardstick(name)
    with _open(case, repaired=True) as sc:
        _load(sc, case)
        sc.run()
        xyz, valid = sc.points()
        cloud = sc.cloud()
    assert len(cloud) > 10000 and np.array_equal(_bits(cloud), _bits(y["want"]["integer"]["points"][valid == 1]))
