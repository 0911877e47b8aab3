"""CPU tests of the period repair (sl3d_repair_periods), before any GPU time is spent.

(1) The definition does what it is for: on every crafted capture whose Gray frames are shifted by s != 0 against the fringes
(tests/period_cases.py), the NumPy restatement (tests/period_repair_reference.py) turns the oracle's stage-4 planes of the shifted capture
into exactly the oracle's stage-4 planes of the s = 0 capture, on EVERY sample with at least `radius` samples on each side within its run
(radius 4); on s = 0 it changes nothing; a second pass changes nothing.
(2) The header the kernels compile (3dscan_amd/csrc/sl3d_period.h: the selection by counting, the jump, the range test, the byte of the
jump plane, the argument checks of the entry point) equals the restatement, through a stand-alone program (tests/native/period_check.cpp),
also under the address and undefined-behaviour sanitizers.  No GPU call is reached.
(3) The captures in two dimensions (GRID_CASES, the seeded random ones, the N = 8 one along either axis) contain what they are for: on the
restatement's own result, every branch of the definition on both axes at radius 1 / 4 / 8, a correction in every tile the kernels launch
and on both sides of every tile, wave and block seam, and no two lines of a tile with the same correction -- without which a kernel that
mixes up the rows of a tile or the lanes of a wave would still equal the restatement on the device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import period_cases as PC
import period_repair_reference as PR

SRC = os.path.join(ROOT, "tests", "native", "period_check.cpp")
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
RADIUS = 4


def _bits(a):
    return a.view(np.uint32)


@pytest.fixture(scope="module")
def stage4():
    """The oracle's stage-4 planes of every case and shift, computed once."""
    return {(name, s): PC.oracle_stage4(PC.make_case(name, s)) for name in PC.CASES for s in PC.SHIFTS}


@pytest.mark.parametrize("name", PC.CASES)
def test_control_needs_no_repair(stage4, name):
    case = PC.make_case(name, 0)
    for axis in (0, 1):
        code, wrapped, unw, valid = stage4[(name, 0)][axis]
        c2, u2, rep, _ = PR.repair_periods(code, wrapped, unw, valid, axis, RADIUS, case["N"])
        assert rep == 0 and np.array_equal(c2, code) and np.array_equal(_bits(u2), _bits(unw)), (name, axis)


@pytest.mark.parametrize("s", [s for s in PC.SHIFTS if s != 0])
@pytest.mark.parametrize("name", PC.CASES)
def test_shifted_gray_edges_are_repaired_completely(stage4, name, s):
    case = PC.make_case(name, s)
    axis = case["axis"]
    code, wrapped, unw, valid = stage4[(name, s)][axis]
    code0, wrapped0, unw0, valid0 = stage4[(name, 0)][axis]
    assert np.array_equal(valid, valid0) and np.array_equal(_bits(wrapped), _bits(wrapped0))   # the same fringes, the same mask
    inside = PR.interior(valid, axis, RADIUS)
    assert inside.sum() > 100, "the case must have interior samples"
    wrong = inside & (code != code0)
    assert wrong.sum() >= abs(s) * 3 and np.array_equal(wrong, inside & (_bits(unw) != _bits(unw0))), "the shift must show, as whole periods"
    c2, u2, rep, unrep = PR.repair_periods(code, wrapped, unw, valid, axis, RADIUS, case["N"])
    assert np.array_equal(c2[inside], code0[inside]), (name, s, int((c2 != code0)[inside].sum()))
    assert np.array_equal(_bits(u2)[inside], _bits(unw0)[inside])
    assert rep >= wrong.sum()
    if name.startswith("border"):
        assert unrep > 0, "a period no code can hold lies against the border"
    c3, u3, rep3, unrep3 = PR.repair_periods(c2, wrapped, u2, valid, axis, RADIUS, case["N"])
    assert rep3 == 0 and unrep3 == unrep and np.array_equal(c3, c2) and np.array_equal(_bits(u3), _bits(u2)), "a second pass changes nothing"
    # the other axis was not shifted: nothing to repair there
    oc, ow, ou, ov = stage4[(name, s)][1 - axis]
    assert PR.repair_periods(oc, ow, ou, ov, 1 - axis, RADIUS, case["N"])[2] == 0


def test_mask_case_has_short_runs_and_clipped_neighbourhoods():
    """What the hole-and-notch mask is there for: runs shorter than radius + 1 (left alone) and runs that end inside the image."""
    for name in ("mask_v", "mask_h"):
        case = PC.make_case(name, 2)
        axis = case["axis"]
        valid = PC.oracle_stage4(case)[axis][3]
        smp = PR.samples(valid, axis)
        lines = smp if axis == 0 else smp.T
        runs = []
        for line in lines:
            edges = np.flatnonzero(np.diff(np.concatenate(([0], line.astype(np.int8), [0]))))
            runs += list(edges[1::2] - edges[0::2])
        assert any(r < RADIUS + 1 for r in runs) and any(r > 2 * RADIUS for r in runs) and len(runs) > len(lines), runs


def test_jacobi_and_sweep_differ_on_adjacent_bands():
    case = PC.make_jacobi_case()
    code, wrapped, unw, valid = PC.oracle_stage4(case)[0]
    jac = PR.repair_periods(code, wrapped, unw, valid, 0, RADIUS, case["N"])
    swp = PR.repair_periods(code, wrapped, unw, valid, 0, RADIUS, case["N"], in_place=True)
    assert not np.array_equal(jac[0], swp[0])


def test_wide_case_has_a_jump_beyond_a_byte():
    case = PC.make_wide_case()
    code, wrapped, unw, valid = PC.oracle_stage4(case)[0]
    c2, u2, rep, unrep = PR.repair_periods(code, wrapped, unw, valid, 0, RADIUS, case["N"])
    assert np.abs(c2.astype(np.int64) - code).max() >= 128 and rep > 0


# ---- the captures in two dimensions contain what they are for -------------------------------------------------------------------------
# What keeps the GPU tests on them from passing by accident: conditions on the restatement's own result, not measurements of the device.
GRID_RADII = (1, 4, 8)
TILE = {0: (256, 8), 1: (64, 32)}        # k_period_jumps<AXIS>: columns x rows of a block's tile (PERIOD_ROWS, PERIOD_BAND)
# (direction, last position before the seam): 0 a seam between two columns, 1 between two rows
SEAMS = {0: ((0, 255), (1, 7)), 1: ((1, 31), (1, 7), (0, 63))}


@pytest.fixture(scope="module")
def grids():
    """Per 2-D case: the case, the oracle's stage-4 planes and, per (axis, radius), the restatement's result."""
    out = {}
    for name in PC.GRID_CASES:
        case = PC.make_grid_case(name)
        planes = PC.oracle_stage4(case)
        res = {(axis, radius): PR.repair_periods(*planes[axis], axis, radius, case["N"]) for axis in (0, 1) for radius in GRID_RADII}
        out[name] = case, planes, res
    return out


def _correction(planes, res):
    return res[0].astype(np.int64) - planes[0]


def _samples_around(smp, axis, radius):
    """n of the definition for every pixel: the samples among the 2 * radius + 1 pixels around it along the coded direction."""
    pad = np.pad(smp.astype(np.int32), ((0, 0), (radius, radius)) if axis == 0 else ((radius, radius), (0, 0)))
    L = smp.shape[1 - axis]
    return sum(pad[:, d:d + L] if axis == 0 else pad[d:d + L, :] for d in range(2 * radius + 1))


def _tiles(axis, W, H):
    """The tiles k_period_jumps<axis> is launched on: (rows, columns) slices clipped to the window."""
    tw, th = TILE[axis]
    pitch = (W + 15) // 16 * 16
    return [(slice(r, min(r + th, H)), slice(c, min(c + tw, W))) for r in range(0, H, th) for c in range(0, pitch, tw)]


def test_grid_geometry():
    for name, n0, n1 in (("grid", (2, 10), (5, 3)), ("sliver", (2, 5), (5, 2)), ("grid_window", (2, 10), (5, 3))):
        case = PC.make_grid_case(name)
        W, H = case["W"], case["H"]
        assert len(_tiles(0, W, H)) == n0[0] * n0[1] and len(_tiles(1, W, H)) == n1[0] * n1[1], name
        assert case["planes_v"][0].shape == (H, W) and case["mask"].shape == case["full"][::-1] and len(case["planes_v"]) == 3 + 2 * case["N"]
    case = PC.make_grid_case("grid_window")
    assert all(o % 8 for o in case["origin"]) and all(f % 8 for f in case["full"])
    # the lines: neighbours and the lines of one tile get different shifts and origins; edges on the seam, one pixel before it, period -1
    for i in range(300):
        assert PC.line_shift(i) != PC.line_shift(i + 1) and PC.line_origin(i) != PC.line_origin(i + 1)
        assert len({(PC.line_origin(k) % PC.FW, PC.line_shift(k)) for k in range(i, i + 8)}) == 8
    for seam, lines in ((256, 75), (32, 280)):
        at = {(seam + PC.line_origin(i)) % PC.FW for i in range(lines)}
        assert 0 in at and 1 in at
        assert any(PC.line_origin(i) < 0 for i in range(lines))
    # the point errors: all four corners of every seam crossing, every k within +-1 .. +-3 and different from its neighbours' on both axes
    for axis, k in enumerate(PC.grid_points(280, 75)):
        assert all(1 <= abs(v) <= 3 for v in k.values()) and all(0 <= r < 75 and 0 <= c < 280 for r, c in k)
        for r in PC.SEAM_ROWS:
            for c in PC.SEAM_COLS:
                assert (r, c) in k
        for (r, c), v in k.items():              # along the coded direction no two neighbours alike, around a seam crossing neither way
            assert k.get((r, c + 1) if axis == 0 else (r + 1, c), 0) != v, (r, c)
            assert not (r in PC.SEAM_ROWS and c in PC.SEAM_COLS) or (k.get((r, c + 1), 0) != v and k.get((r + 1, c), 0) != v), (r, c)
        assert any(r == 74 for r, c in k) and any(c == 279 for r, c in k)
        ends = (1, 278) if axis == 0 else (1, 73)
        assert all(any(p[1 - axis] == e for p in k) for e in ends), "the first and the last sample of a line"
    # the signatures of the lines of a tile differ, wherever the line lies on the projector
    for origin in (0, 13, 48, 79):
        sig = [tuple(PC.line_signature(i, np.arange(34) + origin)) for i in range(64)]
        assert len(set(sig)) == 64 and all(abs(p - q) >= 4 for s in sig for (p, _), (q, _) in zip(s, s[1:]))


@pytest.mark.parametrize("name", PC.GRID_CASES)
def test_grid_cases_repair_refuse_and_leave_alone_on_both_axes(grids, name):
    case, planes, res = grids[name]
    for axis in (0, 1):
        smp = PR.samples(planes[axis][3], axis)
        assert 2 * smp.sum() >= case["W"] * case["H"], "the mask has not eaten the case"
        for radius in GRID_RADII:
            _, _, rep, unrep = res[(axis, radius)]
            assert rep > 0, (name, axis, radius)
            assert unrep > 0 or name == "sliver", (name, axis, radius)
            assert (smp & (_samples_around(smp, axis, radius) < radius + 1)).any(), (name, axis, radius, "no sample with n < radius + 1")


@pytest.mark.parametrize("name", PC.GRID_CASES)
def test_grid_cases_correct_something_in_every_tile_and_beside_every_seam(grids, name):
    case, planes, res = grids[name]
    W, H = case["W"], case["H"]
    for axis in (0, 1):
        smp = PR.samples(planes[axis][3], axis)
        for radius in GRID_RADII:
            corr = _correction(planes[axis], res[(axis, radius)])
            for rows, cols in _tiles(axis, W, H):
                if smp[rows, cols].sum(1 - axis).max(initial=0) >= 2 * radius + 1:
                    assert corr[rows, cols].any(), (name, axis, radius, rows, cols)
            for direction, last in SEAMS[axis]:
                c = corr if direction == 0 else corr.T
                if last + 1 < c.shape[1]:
                    assert c[:, max(0, last - radius + 1):last + 1].any() and c[:, last + 1:last + 1 + radius].any(), (name, axis, radius, direction, last)


@pytest.mark.parametrize("name", PC.GRID_CASES)
def test_grid_cases_have_no_two_equal_lines_in_a_tile(grids, name):
    """What tells a line taken from the wrong row of a tile (the wrong lane of a wave) from the right one."""
    case, planes, res = grids[name]
    for axis in (0, 1):
        smp = PR.samples(planes[axis][3], axis)
        for radius in GRID_RADII:
            corr = _correction(planes[axis], res[(axis, radius)])
            lines, has = (corr, smp.any(1)) if axis == 0 else (corr.T, smp.any(0))
            step = TILE[axis][1 - axis]       # 8 rows of a tile of <0>, 64 columns of a tile of <1>
            for t in range(0, len(lines), step):
                seen = {lines[i].tobytes() for i in range(t, min(t + step, len(lines))) if has[i]}
                assert len(seen) == int(has[t:t + step].sum()), (name, axis, radius, t)


def test_rows_that_are_copies_are_noticed():
    """The condition above is no formality: the strips of CASES, whose rows are copies of each other, do not meet it."""
    case = PC.make_case("plain_v", 2)
    planes = PC.oracle_stage4(case)[0]
    corr = _correction(planes, PR.repair_periods(*planes, 0, RADIUS, case["N"]))
    assert corr.any() and len({row.tobytes() for row in corr}) == 1


def test_grid_is_repaired_to_its_control(grids):
    """Radius 4 on both axes turns `grid` into the capture without shifts and point errors wherever a sample has 4 samples on each side."""
    case, planes, res = grids["grid"]
    control = PC.oracle_stage4(PC.make_grid_case("grid", control=True))
    for axis in (0, 1):
        code, wrapped, unw, valid = planes[axis]
        assert np.array_equal(valid, control[axis][3]) and np.array_equal(_bits(wrapped), _bits(control[axis][1]))
        inside = PR.interior(valid, axis, RADIUS)
        assert np.array_equal(PR.repair_periods(*control[axis], axis, RADIUS, case["N"])[0][inside], control[axis][0][inside]), "the control needs no repair"
        assert inside.sum() > 10000 and (code != control[axis][0])[inside].sum() > 500
        c2, u2 = res[(axis, RADIUS)][:2]
        assert np.array_equal(c2[inside], control[axis][0][inside]) and np.array_equal(_bits(u2)[inside], _bits(control[axis][2])[inside]), axis


def test_jacobi_and_sweep_differ_on_the_grid(grids):
    case, planes, res = grids["grid"]
    for axis in (0, 1):
        swp = PR.repair_periods(*planes[axis], axis, RADIUS, case["N"], in_place=True)
        assert not np.array_equal(res[(axis, RADIUS)][0], swp[0]), axis


@pytest.mark.parametrize("seed", PC.FUZZ_SEEDS)
def test_fuzz_cases_repair_on_both_axes_and_differ(seed):
    case = PC.make_fuzz_case(seed)
    planes = PC.oracle_stage4(case)
    other = PC.oracle_stage4(PC.make_fuzz_case(seed + 100))
    for axis in (0, 1):
        smp = PR.samples(planes[axis][3], axis)
        assert 2 * smp.sum() >= case["W"] * case["H"]
        assert not np.array_equal(planes[axis][0], other[axis][0]) and not np.array_equal(planes[axis][3], other[axis][3])
        for radius in GRID_RADII:
            _, _, rep, unrep = PR.repair_periods(*planes[axis], axis, radius, case["N"])
            assert rep > 100, (seed, axis, radius)


def test_wide_case_along_either_axis():
    """|j| = 128 and a narrow jump in every line, at places that differ between neighbouring lines; on the horizontal axis in a lane >= 8 of
    the second column tile and in every wave of k_period_jumps<1>."""
    W, H = 80, 44
    pos = PC.wide_positions(H, W, 0)
    assert all(8 <= p < H - 8 and p != q for pq in pos for p, q in (pq, pq[::-1])) and all(a != b for a, b in zip(pos, pos[1:]))
    assert {(pw % 32) // 8 for pw, _ in pos[72:80]} >= {1, 2, 3} and {pw // 32 for pw, _ in pos[64:80]} == {0, 1}
    for axis, variant in ((1, 0), (0, 1), (0, 2)):
        case = PC.make_wide_case(axis, (W, H), variant)
        code, wrapped, unw, valid = PC.oracle_stage4(case)[axis]
        c2, _, rep, _ = PR.repair_periods(code, wrapped, unw, valid, axis, RADIUS, case["N"])
        d = np.abs(c2.astype(np.int64) - code)
        lines = d if axis == 0 else d.T
        assert all((line == 128).sum() == 1 and (line == 3).sum() == 1 for line in lines), (axis, variant)
        oc, ow, ou, ov = PC.oracle_stage4(case)[1 - axis]
        assert PR.repair_periods(oc, ow, ou, ov, 1 - axis, RADIUS, case["N"])[2] == 0
    a, b = (PC.oracle_stage4(PC.make_wide_case(0, (W, H), v))[0][0] for v in (1, 2))
    assert not np.array_equal(a, b)
    # the strip of before is what it was
    old = PC.make_wide_case()
    assert (old["W"], old["H"], old["axis"]) == (96, 8, 0)


# ---- the header the kernels compile ---------------------------------------------------------------------------------------------------
def _write_case(d, tag, planes, axis, radius, n_gray):
    code, wrapped, unw, valid = planes
    H, W = valid.shape
    p = d / f"{tag}.bin"
    with open(p, "wb") as f:
        np.array([W, H, axis, radius, n_gray], np.int32).tofile(f)
        code.astype(np.int32).tofile(f); wrapped.tofile(f); unw.tofile(f); valid.tofile(f)
    return str(p), (H, W)


def _run_check(exe, d, tag, planes, axis, radius, n_gray, env=None):
    src, (H, W) = _write_case(d, tag, planes, axis, radius, n_gray)
    out = str(d / f"{tag}.out")
    subprocess.check_call([exe, src, out], timeout=120, env=env)
    with open(out, "rb") as f:
        code = np.fromfile(f, np.int32, H * W).reshape(H, W)
        unw = np.fromfile(f, np.float32, H * W).reshape(H, W)
        counts = np.fromfile(f, np.uint32, 2)
    want = PR.repair_periods(*planes, axis, radius, n_gray)
    assert np.array_equal(code, want[0]) and np.array_equal(_bits(unw), _bits(want[1])) and tuple(counts) == want[2:], (tag, radius)


def _check_inputs():
    """(tag, case, axis, radii)"""
    every = (1, 2, 3, 4, 5, 6, 7, 8)
    for tag, case in (("plain_v", PC.make_case("plain_v", 2)), ("mask_h", PC.make_case("mask_h", -2)), ("border_lo_v", PC.make_case("border_lo_v", 2)),
                      ("border_hi_h", PC.make_case("border_hi_h", 1)), ("jacobi", PC.make_jacobi_case()), ("wide", PC.make_wide_case())):
        yield tag, case, case["axis"], every
    # two dimensions: more than one tile each way, partial last tiles, lines that differ
    for tag, case, radii in (("grid", PC.make_grid_case("grid"), every), ("fuzz", PC.make_fuzz_case(PC.FUZZ_SEEDS[0]), GRID_RADII),
                             ("wide_h", PC.make_wide_case(1, (80, 44)), GRID_RADII)):
        for axis in (0, 1):
            yield f"{tag}_{axis}", case, axis, radii


def test_header_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "period_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    for tag, case, axis, radii in _check_inputs():
        planes = PC.oracle_stage4(case)[axis]
        for radius in radii:
            _run_check(exe, tmp_path, f"{tag}_{radius}", planes, axis, radius, case["N"])
    # random phases with ties, infinities never among the samples: the selection by counting against the sort
    rng = np.random.default_rng(5)
    H, W = 12, 70
    valid = (rng.random((H, W)) < 0.8).astype(np.uint8)
    code = rng.integers(0, 32, (H, W)).astype(np.int32)
    wrapped = (rng.integers(0, 8, (H, W)) * 0.75).astype(np.float32)          # few distinct values: many equal floats
    unw = (wrapped.astype(np.float64) + code * PR.TWO_PI_REF).astype(np.float32)
    for axis in (0, 1):
        for radius in (1, 4, 8):
            _run_check(exe, tmp_path, f"rand_{axis}_{radius}", (code, wrapped, unw, valid), axis, radius, 5)


def test_header_and_argument_checks_are_clean_under_asan_and_ubsan(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers; without an input file it runs the argument
    checks of sl3d_repair_periods (period_check_args) over every refusal the header documents and exits 0 iff the statuses are right."""
    exe = str(tmp_path / "period_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([exe], timeout=60, env=env)
    grid = PC.make_grid_case("grid")
    for tag, case, axis in (("border_lo_v", PC.make_case("border_lo_v", -2), 0), ("wide", PC.make_wide_case(), 0), ("mask_h", PC.make_case("mask_h", 2), 1),
                            ("grid_0", grid, 0), ("grid_1", grid, 1)):
        planes = PC.oracle_stage4(case)[axis]
        for radius in (1, 4, 8):
            _run_check(exe, tmp_path, f"{tag}_{radius}", planes, axis, radius, case["N"], env=env)


def test_argument_checks_without_sanitizers(tmp_path):
    exe = str(tmp_path / "period_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    subprocess.check_call([exe], timeout=60)
