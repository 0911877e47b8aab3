"""GPU tests (-m gpu) of sl3d_repair_periods / Scanner.repair_periods on the crafted captures of tests/period_cases.py: the
planes stage 4 left on the device, repaired by k_period_jumps / k_period_apply, against the NumPy restatement of the definition
(tests/period_repair_reference.py) applied to the very planes downloaded before the call -- code and absolute phase bit for bit (floats
compared as uint32), the two counts equal, the wrapped phase and the valid maps untouched.  Then end to end through stages 5 and 7, the
Jacobi rule, the refusals and the other views of a context.

The strips of PC.CASES never leave one tile of a kernel across the coded direction, and each of their lines is a copy of the next one.
The captures in two dimensions (PC.GRID_CASES, PC.make_fuzz_case, PC.make_wide_case with a size) are there for what that cannot see: they
span several tiles of k_period_jumps<0> (256 x 8) and <1> (64 x 32, 8 rows per wave) both ways, with partial last tiles and padding
columns of the pitch inside a launched tile, both axes carry jumps, and no two lines of a tile ask for the same correction
(tests/test_period_repair_arith.py asserts that of the restatement) -- so a window read from the wrong row of a tile or the wrong lane, or
a jump written to another line, cannot equal the restatement.

All of these captures are smooth planes: nothing in them is random, flat, ragged in size or under a mask that holds a value other than
0 / 1.  tests/test_gpu_repair_edges.py runs the same check (tests/period_repair_checks.py) on the edge frames of tests/edge_frames.py."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import pkg

import period_cases as PC
import period_repair_reference as PR
from period_repair_checks import assert_same_planes as _assert_same_planes, bits as _bits, check_pass, planes as _planes, stages34 as _stages34

pytestmark = pytest.mark.gpu

RADII = (1, 4, 8)


def _open(case, max_views=1, keep=True, calibrate=False):
    S, syn = pkg("scanner"), pkg("synth")
    sc = S.Scanner(case["W"], case["H"], case["PW"], case["PH"], case["N"], case["N"], PC.FW, PC.FW, keep_stages=keep, full_size=case["full"],
                   origin=case["origin"], max_views=max_views)
    if calibrate:
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(case["full"][0], case["full"][1], case["PW"], case["PH"])))
    return sc


def _load(sc, case, view=0):
    sc.set_mask(case["mask"], view=view)
    sc.set_frames(0, case["planes_v"], view=view)
    sc.set_frames(1, case["planes_h"], view=view)


def _check_pass(sc, case, axis, radius, view=0, what=""):
    return check_pass(sc, case["N"], axis, radius, view, what)


@functools.lru_cache(maxsize=None)
def _grid(name, control=False):
    """a capture in two dimensions, built once per module (inputs only: nothing the device wrote is ever kept)"""
    return PC.make_fuzz_case(name) if isinstance(name, int) else PC.make_grid_case(name, control)


def _special(name):
    return PC.make_jacobi_case() if name == "jacobi" else PC.make_wide_case()


# ---- 1. bit for bit, every case, every shift, radius 1 / 4 / 8 ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", PC.SHIFTS)
@pytest.mark.parametrize("name", PC.CASES)
def test_device_equals_the_restatement(name, s):
    case = PC.make_case(name, s)
    repaired = 0
    with _open(case) as sc:
        _load(sc, case)
        for radius in RADII:
            _stages34(sc)
            for axis in (case["axis"], 1 - case["axis"]):
                rep, unrep = _check_pass(sc, case, axis, radius, what=(name, s))
                repaired += rep if axis == case["axis"] else 0
                assert axis == case["axis"] or rep == 0
            # a second pass is a pass over the result of the first
            _check_pass(sc, case, case["axis"], radius, what=(name, s, "second pass"))
    assert (repaired > 0) == (s != 0), (name, s, repaired)


@pytest.mark.parametrize("name", ["jacobi", "wide"])
def test_device_equals_the_restatement_on_the_special_cases(name):
    case = _special(name)
    with _open(case) as sc:
        _load(sc, case)
        for radius in (1, 2, 3, 4, 5, 6, 7, 8):          # every instantiation of k_period_jumps<0, R>
            _stages34(sc)
            rep, _ = _check_pass(sc, case, 0, radius, what=(name,))
            assert rep > 0
    if name == "wide":
        code = PC.oracle_stage4(case)[0][0]
        assert np.abs(PR.repair_periods(*PC.oracle_stage4(case)[0], 0, 4, case["N"])[0].astype(np.int64) - code).max() >= 128


# ---- 1b. two dimensions: several tiles both ways, partial last tiles, no line a copy of another ------------------------------------------------
@pytest.mark.parametrize("name", PC.GRID_CASES)
def test_device_equals_the_restatement_in_two_dimensions(name):
    case = _grid(name)
    with _open(case) as sc:
        _load(sc, case)
        for radius in (1, 2, 3, 4, 5, 6, 7, 8):          # all 16 instantiations with blockIdx.x, blockIdx.y > 0
            _stages34(sc)
            for axis in (0, 1):
                rep, unrep = _check_pass(sc, case, axis, radius, what=(name,))
                assert rep > 0 and (unrep > 0 or name == "sliver"), (name, axis, radius, rep, unrep)
            for axis in (0, 1):
                _check_pass(sc, case, axis, radius, what=(name, "second pass"))


@pytest.mark.parametrize("seed", PC.FUZZ_SEEDS)
def test_device_equals_the_restatement_on_random_captures(seed):
    case = _grid(seed)
    with _open(case) as sc:
        _load(sc, case)
        for radius in RADII:
            _stages34(sc)
            for axis in (0, 1):
                rep, _ = _check_pass(sc, case, axis, radius, what=("fuzz", seed))
                assert rep > 0


def test_wide_jumps_on_the_horizontal_axis_and_in_a_later_view():
    """N = 8: |j| = 128 along the columns (the wide plane written by k_period_jumps<1>, in lanes >= 8 of the second column tile and in
    every wave) in view 2, then along the rows in view 1: the jump and the wide plane are scratch of the context, shared by all calls --
    what the first call left there must not show in the second."""
    size = (80, 44)
    cases = [PC.make_wide_case(0, size, 2), PC.make_wide_case(0, size, 1), PC.make_wide_case(1, size, 0)]
    with _open(cases[0], max_views=3) as sc:
        for v, c in enumerate(cases):
            _load(sc, c, view=v)
            _stages34(sc, view=v)
        for view, axis in ((2, 1), (1, 0)):
            before = [[_planes(sc, a, v) for a in (0, 1)] for v in range(3)]
            rep, _ = _check_pass(sc, cases[view], axis, 4, view=view, what=("wide", "view", view))
            assert rep >= 2 * (size[1 - axis] - 2)
            assert np.abs(sc.code(axis, view).astype(np.int64) - before[view][axis][0]).max() >= 128
            for v in range(3):
                if v != view:
                    for a in (0, 1):
                        _assert_same_planes(_planes(sc, a, v), before[v][a], ("view", v, "after the repair of view", view))


def test_counts_are_per_call():
    """The two words of a (view, axis) are cleared by every call, whether the caller reads them or not, and many blocks add to them:
    each returned pair is that of its call alone."""
    case = _grid("grid")
    for radius in (1, 4):
        with _open(case) as sc:
            _load(sc, case)
            _stages34(sc)
            first = PR.repair_periods(*_planes(sc, 0), 0, radius, case["N"])
            assert sc.repair_periods(0, radius, want_counts=False) is None        # counts == NULL
            code, _, unw, _ = _planes(sc, 0)
            assert np.array_equal(code, first[0]) and np.array_equal(_bits(unw), _bits(first[1]))
            rep1, unrep1 = _check_pass(sc, case, 1, radius, what="counts, axis 1")
            again = _check_pass(sc, case, 0, radius, what="counts, axis 0 again")
            # (the pairs differ, so one that had been added to another, or left from another call, would show)
            assert first[2] > 0 and first[3] > 0 and rep1 > 0 and len({first[2:], (rep1, unrep1), again}) == 3


def test_every_radius_on_the_horizontal_axis():
    case = PC.make_case("mask_h", 2)
    with _open(case) as sc:
        _load(sc, case)
        for radius in (1, 2, 3, 4, 5, 6, 7, 8):          # every instantiation of k_period_jumps<1, R>
            _stages34(sc)
            _check_pass(sc, case, 1, radius, what=("mask_h", 2))


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------------
def _scan(case, repair):
    with _open(case, calibrate=True) as sc:
        _load(sc, case)
        _stages34(sc)
        if repair:
            for axis in (0, 1):
                sc.repair_periods(axis, 4)
        sc.compute_c_p_map()
        sc.triangulate()
        xyz, valid = sc.points()
        return sc.c_p_map(), valid, xyz, sc.valid_map(case["axis"]) if case["axis"] is not None else [sc.valid_map(a) for a in (0, 1)]


@pytest.mark.parametrize("s", [-2, 2])
@pytest.mark.parametrize("name", PC.CASES)
def test_end_to_end_the_repaired_scan_is_the_unshifted_scan(name, s):
    control = _scan(PC.make_case(name, 0), False)
    case = PC.make_case(name, s)
    axis = case["axis"]
    inside = PR.interior(control[3], axis, 4)
    assert inside.sum() > 100
    # without the repair: correspondences off by exactly one fringe width along the coded direction, nothing else
    raw = _scan(case, False)
    both = inside & (raw[1] == 1) & (control[1] == 1)
    diff = np.abs(raw[0][both] - control[0][both])
    assert set(np.unique(diff[:, axis]).tolist()) == {0, PC.FW}, np.unique(diff[:, axis])
    assert (diff[:, 1 - axis] == 0).all()
    # with it: the unshifted scan
    got = _scan(case, True)
    assert np.array_equal(got[1][inside], control[1][inside])
    assert np.array_equal(got[0][inside], control[0][inside])
    v = inside & (control[1] == 1)
    assert v.sum() > 100 and np.array_equal(_bits(got[2][v]), _bits(control[2][v]))


def test_end_to_end_the_repaired_grid_is_the_capture_without_shifts_and_point_errors():
    control = _scan(_grid("grid", control=True), False)
    case = _grid("grid")
    inside = PR.interior(control[3][0], 0, 4) & PR.interior(control[3][1], 1, 4)
    assert inside.sum() > 10000
    # without the repair: correspondences off by whole fringe widths, on both axes
    raw = _scan(case, False)
    both = inside & (raw[1] == 1) & (control[1] == 1)
    diff = np.abs(raw[0][both] - control[0][both])
    for axis in (0, 1):
        found = set(np.unique(diff[:, axis]).tolist())
        assert found <= {0, PC.FW, 2 * PC.FW, 3 * PC.FW} and {PC.FW, 3 * PC.FW} <= found, (axis, found)
    # with it: the control
    got = _scan(case, True)
    assert np.array_equal(got[1][inside], control[1][inside])
    assert np.array_equal(got[0][inside], control[0][inside])
    v = inside & (control[1] == 1)
    assert v.sum() > 10000 and np.array_equal(_bits(got[2][v]), _bits(control[2][v]))


def test_repair_behind_the_fused_launch_of_a_keep_context():
    """After sl3d_run on a KEEP_STAGES context the same planes exist: repair + stage 5 + stage 7 there equals the staged route."""
    case = PC.make_case("plain_v", 2)
    staged = _scan(case, True)
    with _open(case, calibrate=True) as sc:
        _load(sc, case)
        sc.run()
        for axis in (0, 1):
            _check_pass(sc, case, axis, 4, what="behind sl3d_run")
        sc.compute_c_p_map()
        sc.triangulate()
        xyz, valid = sc.points()
        inside = PR.interior(sc.valid_map(0), 0, 4)
        assert np.array_equal(valid[inside], staged[1][inside]) and np.array_equal(sc.c_p_map()[inside], staged[0][inside])


# ---- 3. Jacobi ---------------------------------------------------------------------------------------------------------------------------
def test_the_pass_is_a_jacobi_pass():
    case = PC.make_jacobi_case()
    with _open(case) as sc:
        _load(sc, case)
        _stages34(sc)
        before = _planes(sc, 0)
        jac = PR.repair_periods(*before, 0, 4, case["N"])
        swp = PR.repair_periods(*before, 0, 4, case["N"], in_place=True)
        assert not np.array_equal(jac[0], swp[0]), "the case must tell the two apart"
        counts = sc.repair_periods(0, 4)
        code, _, unw, _ = _planes(sc, 0)
    assert np.array_equal(code, jac[0]) and np.array_equal(_bits(unw), _bits(jac[1])) and counts == jac[2:]
    assert not np.array_equal(code, swp[0])


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    S = pkg("scanner")
    case = PC.make_case("plain_v", 2)
    counts = (ctypes.c_uint32 * 2)(7, 7)
    with _open(case, max_views=2) as sc:
        _load(sc, case)
        _stages34(sc)
        before = [_planes(sc, a) for a in (0, 1)]
        L, h = sc.L, sc._h
        assert L.sl3d_repair_periods(h, 0, 0, 0, counts) == -1 and b"radius" in L.sl3d_last_error(h)
        assert L.sl3d_repair_periods(h, 0, 0, 9, counts) == -1
        assert L.sl3d_repair_periods(h, 0, 2, 4, counts) == -1 and b"axis" in L.sl3d_last_error(h)
        assert L.sl3d_repair_periods(h, 0, -1, 4, counts) == -1
        assert L.sl3d_repair_periods(h, 2, 0, 4, counts) == -1 and L.sl3d_repair_periods(h, -1, 0, 4, counts) == -1
        assert L.sl3d_repair_periods(None, 0, 0, 4, counts) == -1
        assert tuple(counts) == (7, 7)
        for a in (0, 1):
            _assert_same_planes(_planes(sc, a), before[a], ("after the refusals", a))
        with pytest.raises(S.Sl3dError):
            sc.repair_periods(0, radius=0)
        # counts == NULL: the call stays asynchronous and does the same
        want = PR.repair_periods(*before[0], 0, 4, case["N"])
        assert L.sl3d_repair_periods(h, 0, 0, 4, None) == 0
        code, _, unw, _ = _planes(sc, 0)
        assert np.array_equal(code, want[0]) and np.array_equal(_bits(unw), _bits(want[1]))
    with _open(case, keep=False) as sc:                       # no SL3D_FLAG_KEEP_STAGES
        _load(sc, case)
        assert sc.L.sl3d_repair_periods(sc._h, 0, 0, 4, counts) == -4 and b"KEEP_STAGES" in sc.L.sl3d_last_error(sc._h)
    # N_a == 0: nothing to repair on that axis (SL3D_E_UNSUPPORTED); the other axis works
    with S.Scanner(case["W"], case["H"], case["PW"], case["PH"], 0, case["N"], PC.FW, PC.FW, keep_stages=True) as sc:
        sc.set_mask(case["mask"])
        sc.set_frames(0, case["planes_v"][:3])
        sc.set_frames(1, case["planes_h"])
        _stages34(sc)
        before = [_planes(sc, a) for a in (0, 1)]
        assert sc.L.sl3d_repair_periods(sc._h, 0, 0, 4, counts) == -5 and b"Gray" in sc.L.sl3d_last_error(sc._h)
        assert tuple(counts) == (7, 7)
        for a in (0, 1):
            _assert_same_planes(_planes(sc, a), before[a], ("after the refusal", a))
        _check_pass(sc, dict(case, N=case["N"]), 1, 4, what="N_v == 0, axis 1")


# ---- 5. the other views of the context -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain_v", "plain_h"])
def test_a_view_other_than_0_leaves_the_other_views_alone(name):
    cases = [PC.make_case(name, s) for s in (2, -1, 1)]
    axis = cases[0]["axis"]
    with _open(cases[0], max_views=3) as sc:
        for v, c in enumerate(cases):
            _load(sc, c, view=v)
            _stages34(sc, view=v)
        before = [[_planes(sc, a, v) for a in (0, 1)] for v in range(3)]
        for view in (1, 2):
            rep, _ = _check_pass(sc, cases[view], axis, 4, view=view, what=(name, "view", view))
            assert rep > 0
            for v in range(3):
                if v > view or v == 0:
                    for a in (0, 1):
                        _assert_same_planes(_planes(sc, a, v), before[v][a], (name, "view", v, "after the repair of view", view))
