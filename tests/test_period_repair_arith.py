"""CPU tests of the period repair (sl3d_repair_periods), before any GPU time is spent.

(1) The definition does what it is for: on every crafted capture whose Gray frames are shifted by s != 0 against the fringes
(tests/period_cases.py), the NumPy restatement (tests/period_repair_reference.py) turns the oracle's stage-4 planes of the shifted capture
into exactly the oracle's stage-4 planes of the s = 0 capture, on EVERY sample with at least `radius` samples on each side within its run
(radius 4); on s = 0 it changes nothing; a second pass changes nothing.
(2) The header the kernels compile (3dscan_amd/csrc/sl3d_period.h: the selection by counting, the jump, the range test, the byte of the
jump plane, the argument checks of the entry point) equals the restatement, through a stand-alone program (tests/native/period_check.cpp),
also under the address and undefined-behaviour sanitizers.  No GPU call is reached."""
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
    yield "plain_v", PC.make_case("plain_v", 2)
    yield "mask_h", PC.make_case("mask_h", -2)
    yield "border_lo_v", PC.make_case("border_lo_v", 2)
    yield "border_hi_h", PC.make_case("border_hi_h", 1)
    yield "jacobi", PC.make_jacobi_case()
    yield "wide", PC.make_wide_case()


def test_header_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "period_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    for tag, case in _check_inputs():
        planes = PC.oracle_stage4(case)[case["axis"]]
        for radius in (1, 2, 3, 4, 5, 6, 7, 8):
            _run_check(exe, tmp_path, f"{tag}_{radius}", planes, case["axis"], radius, case["N"])
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
    for tag, case in (("border_lo_v", PC.make_case("border_lo_v", -2)), ("wide", PC.make_wide_case()), ("mask_h", PC.make_case("mask_h", 2))):
        planes = PC.oracle_stage4(case)[case["axis"]]
        for radius in (1, 4, 8):
            _run_check(exe, tmp_path, f"{tag}_{radius}", planes, case["axis"], radius, case["N"], env=env)


def test_argument_checks_without_sanitizers(tmp_path):
    exe = str(tmp_path / "period_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    subprocess.check_call([exe], timeout=60)
