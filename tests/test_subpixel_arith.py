"""CPU tests of the sub-pixel triangulation (sl3d_triangulate_subpixel), before any GPU time is spent.

(a) The NumPy restatement (tests/subpixel_reference.py) is pinned on the oracle: fed the oracle's integer c_p_map instead of the
    continuous coordinates it reproduces the oracle's intersection_points to 1e-11 relative, on every rig of tests/subpixel_cases.py.
(b) rint of the continuous coordinates is the oracle's c_p_map on every valid pixel: they are the doubles stage 5 hands to lrint.
(c) What the feature is for: on the synthetic plane the sub-pixel points lie at most half as far (RMS) from the true plane as the integer
    ones, over the pixels decoded within 1.5 px of the analytic coordinates.  The bar is the integer path, not the code under test.
(d) The rejection thresholds the GPU tests use take both branches and stay clear of ties, on the restatement alone.
(e) The header the kernel and the entry point compile (3dscan_amd/csrc/sl3d_subpixel.h: argument checks, rejection rule, residual)
    through a stand-alone program (tests/native/subpixel_check.cpp), also under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import subpixel_cases as SC
import subpixel_reference as SR

SRC = os.path.join(ROOT, "tests", "native", "subpixel_check.cpp")
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]


def _restated(rig, win, integer=False, max_residual=np.inf):
    s, o = SC.scene(rig, win), SC.oracle_scan(rig, win)
    xy = o["c_p_map"].astype(np.float64) if integer else SR.correspondences(*o["unw"], *o["valid_axis"], SC.FW, SC.FW)
    return SR.triangulate(xy, o["valid"], s["cal"], o["A_cam"], o["A_proj"], s["origin"], max_residual)


@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_restatement_is_pinned_on_the_oracle(rig, win):
    o = SC.oracle_scan(rig, win)
    r = _restated(rig, win, integer=True)
    m = o["valid"] == 1
    assert m.sum() > 500
    ref = o["ipoints"][m]
    rel = np.linalg.norm(r["ipoints"][m] - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
    print(f"{rig} {win}: max relative difference to the oracle {rel.max():.3e}")
    assert rel.max() <= 1e-11
    assert np.array_equal(r["valid"], o["valid"]) and r["counts"] == (int(m.sum()), 0)


@pytest.mark.parametrize("win", SC.WINDOWS)
def test_rint_of_the_continuous_coordinates_is_stage_5(win):
    o = SC.oracle_scan("plain", win)
    xy = SR.correspondences(*o["unw"], *o["valid_axis"], SC.FW, SC.FW)
    m = o["valid"] == 1
    assert np.isfinite(xy[m]).all() and np.array_equal(np.rint(xy[m]).astype(np.int64), o["c_p_map"][m])
    both = (o["valid_axis"][0] == 1) & (o["valid_axis"][1] == 1)
    assert np.array_equal(np.isnan(xy[..., 0]), ~both) and np.array_equal(np.isnan(xy[..., 1]), ~both)
    assert (np.abs(xy[m] - np.rint(xy[m])) > 0.01).mean() > 0.9, "the coordinates must be continuous for the test to see anything"


def test_plane_accuracy_against_the_integer_path():
    s, o = SC.scene("plain", "full"), SC.oracle_scan("plain", "full")
    good = SC.good_pixels(s["cap"], o["c_p_map"], o["valid"])
    assert good.sum() > 60000
    integer, sub = SC.plane_rms(o["ipoints"], good), SC.plane_rms(_restated("plain", "full")["ipoints"], good)
    print(f"RMS distance to the plane: integer {integer:.4f} mm, sub-pixel {sub:.4f} mm, ratio {sub / integer:.3f}")
    assert sub <= 0.5 * integer


@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_thresholds_take_both_branches_clear_of_ties(rig, win):
    thr = SC.THRESHOLDS[(rig, win)]
    free = _restated(rig, win)
    res = free["residual"][SC.oracle_scan(rig, win)["valid"] == 1].astype(np.float64)
    assert np.isfinite(res).all()
    rejected = ~(res <= thr)
    assert rejected.sum() >= 1 and (~rejected).mean() >= 0.8, (rig, win, int(rejected.sum()), float((~rejected).mean()))
    assert (np.abs(res - thr) > 1e-4 * thr).all()
    r = _restated(rig, win, max_residual=thr)
    assert r["counts"] == (len(res), int(rejected.sum())) and int((r["valid"] == 1).sum()) == len(res) - int(rejected.sum())
    gone = (SC.oracle_scan(rig, win)["valid"] == 1) & (r["valid"] == 0)
    assert np.isnan(r["points"][gone]).all() and (r["ipoints"][gone] == 0).all() and np.isfinite(r["residual"][gone]).all()
    assert np.array_equal(r["residual"].view(np.uint32), free["residual"].view(np.uint32))


# ---- the header the kernel and the entry point compile ---------------------------------------------------------------------------------
def _residual_case(d, exe, env=None):
    """The residual of sl3d_subpixel.h on the solves of a scene against the restatement: within 1e-6 * ref + 1e-7 px."""
    rig, win = "tangential", "full"
    s, o = SC.scene(rig, win), SC.oracle_scan(rig, win)
    xy = SR.correspondences(*o["unw"], *o["valid_axis"], SC.FW, SC.FW)
    m = o["valid"] == 1
    rows, cols = np.nonzero(m)
    Kc, dc, _, _, Kp, dp, _, _ = s["cal"]
    u, v = SR.undistort_reproject(cols.astype(np.float64), rows.astype(np.float64), Kc, dc)
    up, vp = SR.undistort_reproject(xy[m][:, 0], xy[m][:, 1], Kp, dp)
    X = SR.solve(o["A_cam"], o["A_proj"], u, v, up, vp)
    want = np.sqrt(SR.reprojection_error2(o["A_cam"], X, u, v) + SR.reprojection_error2(o["A_proj"], X, up, vp)).astype(np.float32)
    src, out = str(d / "res.bin"), str(d / "res.out")
    with open(src, "wb") as f:
        np.ascontiguousarray(o["A_cam"], np.float64).tofile(f); np.ascontiguousarray(o["A_proj"], np.float64).tofile(f)
        np.array([len(X)], np.int64).tofile(f)
        np.ascontiguousarray(np.column_stack([X, u, v, up, vp]), np.float64).tofile(f)
    subprocess.check_call([exe, src, out], timeout=120, env=env)
    got = np.fromfile(out, np.float32)
    assert got.shape == want.shape and len(got) > 50000
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 1e-6 * want + 1e-7).all(), float(err.max())


def test_header_checks_and_residual(tmp_path):
    exe = str(tmp_path / "subpixel_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    subprocess.check_call([exe], timeout=60)
    _residual_case(tmp_path, exe)


def test_header_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program with the address and undefined-behaviour sanitizers (nothing here runs inside Python)."""
    exe = str(tmp_path / "subpixel_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([exe], timeout=60, env=env)
    _residual_case(tmp_path, exe, env=env)
