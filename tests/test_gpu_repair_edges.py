"""GPU tests (-m gpu) of the period repair -- k_period_jumps<AXIS, R>, k_period_apply (sl3d_repair_periods) and
k_repair_fused<SUB> (SL3D_FLAG_REPAIR_PERIODS) -- on the inputs of tests/edge_frames.py (EF.REPAIR_CASES): random bytes, flat
frames, a noisy capture with an unlit part, `steps` (ties between different periods), ragged sizes under random masks (one holds the value
2), a window under two masks, and three views whose masks select different quads and lanes on both sides of the seams of k_repair_fused's
64 x 16 tile.  tests/test_repair_edge_cases.py proves on the CPU, from the restatement alone, that these inputs take the branches named here.
tests/test_gpu_period_repair.py and tests/test_gpu_repair_fused.py run the same kernels on smooth crafted captures.

(a) The staged kernels against the NumPy restatement (tests/period_repair_reference.py): per radius stages 3 - 4 again, then per axis one
    call against the restatement applied to the planes downloaded before it (tests/period_repair_checks.py: code and absolute phase bit
    for bit, counts equal, everything else untouched), the result also against the restatement applied to the ORACLE's planes
    (EF.stage_planes: a yardstick that does not pass through the device at all; on the window the oracle's planes of the grown window
    under the valid byte of the whole frame's mask, so every selected pixel of the window is compared, its border lines included), then
    a second pass.
(b) Stages 5 and 7 behind one radius-4 pass per axis: the merged valid map and c_p_map against stage 5 restated from the repaired phases
    (EF.stage5), sl3d_triangulate against tests/subpixel_reference.py at the integer coordinates, sl3d_triangulate_subpixel(+inf) against
    it at the continuous ones -- coordinates bit for bit, points at the project's 1e-5 bar and at BAR_ULPS scaled float32 ulps, residuals
    within 1e-6 * ref + 1e-7.  The restated side is computed from the oracle's planes alone.
(c) k_repair_fused<false> and <true>: a timed flagged context equals the staged route of (b) bit for bit on every window pixel; the same
    for sl3d_run on a KEEP_STAGES | REPAIR_PERIODS context, whose stage getters show the repaired code.  Each yardstick is first checked
    for what its case is there for (EF.REPAIRS).
(d) Per-view masks in one launch, both instantiations, eager masks and sl3d_set_masks_modulated: views 1..3 behind an untouched slot 0
    under the masks A, B, C; run, run_timed and a run after A and C changed places equal every view run alone.  Once with the three view
    captures, once (eager masks: the fringes of `steps` are flat, their modulation is one value) with `random` in view 1 and `steps` in
    view 2: consecutive views stage very different phases into the same LDS rows.
(e) sl3d_repair_periods behind the direct Gray decode (SL3D_FLAG_DIRECT_GRAY | KEEP_STAGES): the same kernels behind another stage-4
    producer, on random / base / 0.9 and steps / base / 0.9."""
import functools

import numpy as np
import pytest

from conftest import assert_points_close, pkg
from period_repair_checks import bits, check_pass, planes, stages34
from point_bars import scaled_ulps
from test_gpu_direct_gray import BAR_ULPS      # the bar of the float cast of an fp64 chain; the reason is given there

import direct_gray_reference as DG
import edge_frames as EF
import subpixel_reference as SR

pytestmark = pytest.mark.gpu

RADIUS = 4
MODES = ("integer", "subpixel")
NAMES = {"integer": "sl3d::k_repair_fused<false>", "subpixel": "sl3d::k_repair_fused<true>"}
CASE_IDS = [f"{name}-{shape}-{p}" for name, shape, p in EF.REPAIR_CASES]
EVERY_RADIUS = (("random", "base", 1.0), ("steps", "base", 1.0), ("steps", "base", 0.9))       # all 16 instantiations of k_period_jumps
KEEP_AND_FLAG = (("random", "base", 0.9), ("random", "window", 0.9), ("steps", "base", 0.9))


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _open(c, *, keep=False, repaired=False, subpixel=False, max_views=1, eager_mask=False, direct=False):
    sc = pkg("scanner").Scanner(c["W"], c["H"], EF.PW, EF.PH, EF.N[0], EF.N[1], EF.FW[0], EF.FW[1], keep_stages=keep, full_size=c["full"], origin=c["origin"],
                                max_views=max_views, repaired=repaired, subpixel=subpixel, eager_mask=eager_mask, direct_gray=direct)
    sc.set_calibration(*c["cal"])
    return sc


def _frames(sc, frames, view=0):
    for a in (0, 1):
        sc.set_frames(a, frames[a], view=view)


def _load(sc, c):
    sc.set_mask(c["mask"])
    _frames(sc, c["planes"])


def _out(sc, mode, view=0):
    xyz, valid = sc.points(view)
    return dict(points=xyz, valid=valid, residual=sc.residuals(view)) if mode == "subpixel" else dict(points=xyz, valid=valid)


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), "elements differ")


def _differ(a, b):
    return any(not np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _sane(want, what, some_valid=True):
    v = want["valid"] == 1
    assert set(np.unique(want["valid"])) <= {0, 1} and (v.any() or not some_valid), what
    assert np.array_equal(np.isnan(want["points"]).any(-1), ~v) and np.array_equal(np.isnan(want["points"]).all(-1), ~v), what
    if "residual" in want:
        assert np.array_equal(np.isnan(want["residual"]), ~v), what


# ---- (a) the staged kernels against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,p", EF.REPAIR_CASES, ids=CASE_IDS)
def test_staged_kernels_against_the_restatement(name, shape, p):
    c, o = EF.case(name, shape, p), EF.stage_planes(name, shape, p)
    total = [0, 0]
    with _open(c, keep=True) as sc:
        _load(sc, c)
        for radius in (range(1, 9) if (name, shape, p) in EVERY_RADIUS else (1, 4, 8)):
            what = (name, shape, p, "radius", radius)
            stages34(sc)
            counts = [check_pass(sc, EF.N[a], a, radius, what=what) for a in (0, 1)]
            want = EF.restated_repair(name, shape, p, radius)
            for a in (0, 1):
                total[a] += counts[a][0] if radius == RADIUS else 0
                code, _, unw, valid = planes(sc, a)
                va = o["valid_axis"][a] == 1
                assert np.array_equal(valid, o["valid_axis"][a]), (what, a, "valid byte")
                assert np.array_equal(code[va], want["code"][a][va]), (what, a, "code against the oracle's planes repaired")
                assert np.array_equal(bits(unw)[va], bits(want["unw"][a])[va]), (what, a, "absolute phase against the oracle's planes repaired")
                assert counts[a] == want["counts"][0][a], (what, a, counts[a], want["counts"][0][a])
            for a in (0, 1):
                check_pass(sc, EF.N[a], a, radius, what=(what, "second pass"))
    assert tuple(n > 0 for n in total) == EF.REPAIRS[(name, shape, p)], (total, "what the case is there for, at radius 4")


# ---- the staged route: the yardstick of (c), held to the restatement by (b) ------------------------------------------------------------------
def _staged_outs(sc, view=0):
    """Stage 5 and both forms of stage 7 over what stages 3 - 4 (and the repair) left."""
    sc.compute_c_p_map(view)
    out = dict(valid5=sc.valid_map(view=view), c_p_map=sc.c_p_map(view), xy=sc.correspondences_subpixel(view))
    out["counts7"] = sc.triangulate_subpixel(view, 1)
    out["subpixel"], out["ip_subpixel"] = _out(sc, "subpixel", view), sc.intersection_points(view)
    sc.triangulate(view)
    out["integer"], out["ip_integer"] = _out(sc, "integer", view), sc.intersection_points(view)
    return out


@functools.lru_cache(maxsize=None)
def _yardstick(name, shape, p):
    """Per case, computed once and left unchanged: the staged route without and with one radius-4 pass per axis, on one KEEP_STAGES
    context.  dict(raw, want: _staged_outs; counts; raw_codes, codes, unw, valid_axis: pairs)."""
    c = EF.case(name, shape, p)
    with _open(c, keep=True) as sc:
        _load(sc, c)
        stages34(sc)
        raw_codes = [sc.code(a) for a in (0, 1)]
        raw = _staged_outs(sc)
        stages34(sc)
        counts = [sc.repair_periods(a, RADIUS) for a in (0, 1)]
        codes, unw, valid_axis = ([f(a) for a in (0, 1)] for f in (sc.code, sc.unwrapped_phase, sc.valid_map))
        want = _staged_outs(sc)
    return dict(raw=raw, want=want, counts=counts, raw_codes=raw_codes, codes=codes, unw=unw, valid_axis=valid_axis)


def _what_the_case_is_there_for(key, y, mode):
    """The staged counts are > 0 on the axes the CPU test names, the repaired code differs from the unrepaired one exactly there, and the
    repaired scan is another scan than the unrepaired one -- or, on flat frames, the same."""
    repairs = EF.REPAIRS[key]
    for a in (0, 1):
        assert (y["counts"][a][0] > 0) == repairs[a], (key, a, y["counts"])
        assert np.array_equal(y["codes"][a], y["raw_codes"][a]) == (not repairs[a]), (key, a)
    assert _differ(y["want"][mode], y["raw"][mode]) == any(repairs), (key, mode)


# ---- (b) stages 5 and 7 behind the repair ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,p", EF.REPAIR_CASES, ids=CASE_IDS)
def test_stages_5_and_7_behind_the_repair(name, shape, p):
    key = (name, shape, p)
    c, o, y = EF.case(*key), EF.stage_planes(*key), _yardstick(*key)
    got = y["want"]
    r = EF.restated_repaired_scan(*key, RADIUS)                   # the restated side: from the oracle's planes alone
    unw, valid_axis, want_valid, want_cp = r["unw"], o["valid_axis"], r["valid"], r["c_p_map"]
    assert tuple(y["counts"]) == tuple(r["counts"])
    v = want_valid == 1
    assert np.array_equal(y["raw"]["valid5"], r["valid_before"]), "merged valid map before the repair"
    # stage 5
    assert np.array_equal(got["valid5"], want_valid), "merged valid map (every pixel: EF.inner() and the lines outside it)"
    assert np.array_equal(got["c_p_map"][v], want_cp[v]), "c_p_map"
    assert got["counts7"] == [(int(v.sum()), 0)]
    # the sub-pixel coordinates: bit for bit, NaN pattern included
    xy = SR.correspondences(*unw, *valid_axis, *EF.FW)
    nan = np.isnan(xy)
    assert np.array_equal(np.isnan(got["xy"]), nan), "NaN pattern of the coordinates"
    assert np.array_equal(_bits(got["xy"])[~nan], _bits(xy)[~nan]), (int((_bits(got["xy"])[~nan] != _bits(xy)[~nan]).sum()), "coordinates differ")
    want = {"integer": SR.triangulate(want_cp.astype(np.float64), want_valid, c["cal"], o["A_cam"], o["A_proj"], c["origin"]),
            "subpixel": SR.triangulate(xy, want_valid, c["cal"], o["A_cam"], o["A_proj"], c["origin"])}
    for mode in MODES:
        out, ip = got[mode], got["ip_" + mode]
        _sane(out, (key, mode), some_valid=bool(v.any()))
        assert np.array_equal(out["valid"], want_valid), (mode, "points are NaN exactly where valid != 1")
        ulps = float(scaled_ulps(out["points"][v], want[mode]["ipoints"][v]).max()) if v.any() else 0.0
        e_f = assert_points_close(out["points"], want[mode]["ipoints"], v)
        e_d = assert_points_close(ip, want[mode]["ipoints"], v)
        line = f"{key} {mode}: {int(v.sum())} valid, points {e_f:.2e} rel, {ulps:.2f} scaled ulps, intersection_points {e_d:.2e} rel"
        assert np.array_equal(_bits(out["points"][v]), _bits(ip[v].astype(np.float32))), "points are the float cast of intersection_points"
        if mode == "subpixel":
            ref = want[mode]["residual"][v].astype(np.float64)
            err = np.abs(out["residual"][v].astype(np.float64) - ref)
            line += f", residuals max |diff| {err.max() if len(err) else 0.0:.2e} px (largest {ref.max() if len(ref) else 0.0:.3g} px)"
        print(line)
        assert ulps <= BAR_ULPS
        if mode == "subpixel":
            assert (err <= 1e-6 * ref + 1e-7).all(), (float(err.max()), float(ref[np.argmax(err - 1e-6 * ref)]))


# ---- (c) k_repair_fused<false> / <true> against the staged route ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,shape,p", EF.REPAIR_CASES, ids=CASE_IDS)
def test_run_equals_the_staged_route(name, shape, p, mode):
    key = (name, shape, p)
    c, y = EF.case(*key), _yardstick(*key)
    _what_the_case_is_there_for(key, y, mode)
    _sane(y["want"][mode], (key, mode), some_valid=True)
    with _open(c, repaired=True, subpixel=mode == "subpixel") as sc:
        assert sc.fused_kernel_name(1) == NAMES[mode] and sc.camera_table_bytes_per_pixel(1) == 0
        _load(sc, c)
        sc.run()
        _same(_out(sc, mode), y["want"][mode], (key, mode))
        assert sc.last_fused_kernel_name() == NAMES[mode] and sc.launch_counts() == (1, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,shape,p", KEEP_AND_FLAG, ids=[f"{n}-{s}-{p}" for n, s, p in KEEP_AND_FLAG])
def test_keep_stages_with_the_flag(name, shape, p, mode):
    key = (name, shape, p)
    c, y = EF.case(*key), _yardstick(*key)
    _what_the_case_is_there_for(key, y, mode)
    with _open(c, keep=True, repaired=True, subpixel=mode == "subpixel") as sc:
        _load(sc, c)
        sc.run()
        _same(_out(sc, mode), y["want"][mode], (key, mode, "KEEP_STAGES | REPAIR_PERIODS"))
        for a in (0, 1):
            assert np.array_equal(sc.code(a), y["codes"][a]), ("the stage getters show the repaired code", a)
            assert np.array_equal(bits(sc.unwrapped_phase(a)), bits(y["unw"][a])), ("... and the repaired phase", a)
        assert np.array_equal(sc.c_p_map(), y["want"]["c_p_map"]) and np.array_equal(sc.valid_map(), y["want"]["valid5"])


# ---- (d) per-view masks in one launch --------------------------------------------------------------------------------------------------------
def _alone(c, mode, frames, select, eager, repaired=True):
    """One view run alone on a one-view context under the 0 / 1 selection `select`: the yardstick."""
    with _open(c, repaired=repaired, subpixel=mode == "subpixel", eager_mask=eager) as sc:
        _frames(sc, frames)
        sc.set_mask(select)
        sc.run()
        return _out(sc, mode)


def _modulated_selection(c, frames, mask, thr):
    """(mask == 1) && gamma > thr on both axes, from sl3d_get_modulation of a context that holds the frames."""
    with _open(c, repaired=True) as sc:
        _frames(sc, frames)
        gammas = [sc.modulation(a) for a in (0, 1)]
    select = mask == 1
    with np.errstate(invalid="ignore"):
        for g in gammas:
            select = select & (g.astype(np.float64) > thr)
    return select.astype(np.uint8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frames,masks", [("captures", "eager"), ("captures", "modulated"), ("random_steps", "eager")])
def test_per_view_masks_in_one_launch(frames, masks, mode):
    c = EF.case("flat_17", "base", 1.0)                          # (the shape and the calibration of the base case)
    caps, (A, B, C) = list(EF.view_captures(0)), EF.view_masks()
    if frames == "random_steps":                                 # view 1 random bytes under A, view 2 `steps` under B
        caps[0], caps[1] = EF.frames("random", "base"), EF.frames("steps", "base")
    eager = masks == "eager"
    thr = None
    if not eager:
        # a threshold from the gammas the device reports: the tenth part of the pixels fails it
        with _open(c, repaired=True) as sc:
            pooled = []
            for planes_ in caps:
                _frames(sc, planes_)
                pooled += [sc.modulation(a) for a in (0, 1)]
        pooled = np.stack(pooled)
        thr = float(np.quantile(pooled[np.isfinite(pooled)].astype(np.float64), 0.1))

    def selection(view, mask):
        if eager:
            return mask
        select = _modulated_selection(c, caps[view], mask, thr)
        taken, left = int(select.sum()), int(((mask == 1) & (select == 0)).sum())
        if mask is not C:
            assert min(taken, left) >= 100, (view, taken, left, "each branch of the modulation test takes a hundred pixels or more")
        return select

    def yardstick(view, mask, repaired=True):
        return _alone(c, mode, caps[view], selection(view, mask), eager, repaired)

    want = {1: yardstick(0, A), 2: yardstick(1, B), 3: yardstick(2, C)}
    swapped = {1: yardstick(0, C), 2: want[2], 3: yardstick(2, A)}
    for k, w in list(want.items()) + list(swapped.items()):
        _sane(w, ("yardstick", k))
    assert len({w["points"].tobytes() for w in want.values()}) == 3, "the views must differ"
    for v, mask in ((1, A), (2, B)):
        assert _differ(want[v], yardstick(v - 1, mask, repaired=False)), (v, "the repaired scan of the view is not its unrepaired scan")

    def set_masks(sc, which):
        for v, m in which.items():
            if eager:
                sc.set_mask(m, view=v)
            else:
                sc.set_masks_modulated(thr, m, first_view=v, n_views=1)

    with _open(c, repaired=True, subpixel=mode == "subpixel", max_views=4, eager_mask=eager) as sc:
        for v, planes_ in enumerate(caps, start=1):
            _frames(sc, planes_, view=v)
        set_masks(sc, {1: A, 2: B, 3: C})
        slot0 = sc.points(0)
        sc.run(1, 3)
        assert sc.last_fused_kernel_name() == NAMES[mode]
        for v in want:
            _same(_out(sc, mode, v), want[v], ("run(1, 3)", v))
        assert sc.run_timed(1, 3) > 0
        for v in want:
            _same(_out(sc, mode, v), want[v], ("run_timed(1, 3)", v))
        set_masks(sc, {1: C, 3: A})
        sc.run(1, 3)
        for v in swapped:
            _same(_out(sc, mode, v), swapped[v], ("run(1, 3) after A and C changed places", v))
        after = sc.points(0)
        assert np.array_equal(after[1], slot0[1]) and np.array_equal(_bits(after[0]), _bits(slot0[0])), "slot 0 is untouched"
        assert sc.last_fused_kernel_name() == NAMES[mode] and sc.launch_counts()[1] == 0


# ---- (e) the repair behind the direct Gray decode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,p", [("random", "base", 0.9), ("steps", "base", 0.9)], ids=["random-base-0.9", "steps-base-0.9"])
def test_repair_periods_on_the_direct_code(name, shape, p):
    c = EF.case(name, shape, p)
    direct = [DG.code_of_planes(c["planes"][a], 3, EF.N[a]) for a in (0, 1)]
    differs = [bool((direct[a] != DG.inverse_code(*DG.split(c["planes"][a], 3, EF.N[a])[1:])).any()) for a in (0, 1)]
    assert differs == [name == "random"] * 2, "random bytes: another code than the inverse-based one; `steps`: the same"
    total = [0, 0]
    with _open(c, keep=True, subpixel=True, direct=True) as sc:
        sc.set_mask(c["mask"])
        for a in (0, 1):
            sc.set_frames(a, DG.read_planes(c["planes"][a], 3, EF.N[a]))
        for radius in (1, 4, 8):
            stages34(sc)
            for a in (0, 1):
                sel = sc.valid_map(a) == 1
                assert sel.any() and np.array_equal(sc.code(a)[sel], direct[a][sel]), "stage 4 left the direct code"
                total[a] += check_pass(sc, EF.N[a], a, radius, what=(name, "direct Gray", radius))[0]
            for a in (0, 1):
                check_pass(sc, EF.N[a], a, radius, what=(name, "direct Gray", radius, "second pass"))
    assert min(total) > 0, total
