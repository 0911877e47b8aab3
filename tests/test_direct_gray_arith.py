"""CPU tests of the Gray decode of SL3D_FLAG_DIRECT_GRAY, before any GPU time is spent, on the NumPy restatement
(tests/direct_gray_reference.py).

(a) The header every kernel and the refusals compile (3dscan_amd/csrc/sl3d_direct_gray.h) through a stand-alone program
    (tests/native/direct_gray_check.cpp): its own checks, and its codes -- scalar and packed -- against the restatement over every
    (gray, I0 + I2) with gray in 0..255 and I0 + I2 in 0..510 and over random stacks of 5 and 16 planes; the same program also under the
    address and undefined-behaviour sanitizers.
(b) The equivalence condition the feature rests on, on synth.make_capture scenes: the direct code equals the inverse-based code on EVERY
    LIT pixel, and with noise 0 on every pixel.  90 x 60 and 320 x 240; 3 and 4 fringe steps; noise 0 and +-2; gain 0.8 / 0.3 / 0.05 at
    offset 10.  Unlit pixels under noise differ, both decodes being noise there (asserted too: the condition is not vacuous).
    The restated inverse-based code is tied to the oracle's, and the oracle run on as_inverse_coded() planes to the restated direct code.
    Both on the optics of the other sub-pixel tests (N = 7, fringe width 4) and on the timed configuration's (N = 10, fringe width 2 on a
    2048 x 1536 projector).  The generator samples each pixel at a point: a camera blur that is large against a 2-pixel fringe is not modelled.
(c) What the feature is for: the vertical-only anchored scan from F + N frames is as accurate against the true plane as the one from
    F + 2 N frames -- the same RMS over good_pixels, to the last bit, because the codes agree on every pixel it is taken over: 13 frames
    against 23 at N = 10 (the headline configuration), and 10 against 17 on the scene of tests/one_axis_cases.py."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import direct_gray_reference as DG
import one_axis_cases as OC
import one_axis_reference as OR
import subpixel_cases as SC
from oracle.oracle import Oracle

SRC = os.path.join(ROOT, "tests", "native", "direct_gray_check.cpp")
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
PW, PH, N, FW = 512, 384, 7, 4
# (projector width, height, Gray planes, fringe width): the scenes of the other sub-pixel tests, and the timed configuration's optics -- ten
# Gray planes over fringes 2 projector pixels wide, every plane carrying information (2 * 2^10 = 2048 columns)
OPTICS = {"N7_fw4": (512, 384, 7, 4), "N10_fw2": (2048, 1536, 10, 2)}


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
def _stacks():
    """(name, i0, i2, gray planes) of the pixel lists the program decodes; every list a multiple of 4 long."""
    g, s = np.meshgrid(np.arange(256), np.arange(511), indexing="ij")
    i0 = np.minimum(s, 255)
    every = ("every (gray, I0 + I2)", i0.ravel().astype(np.uint8), (s - i0).ravel().astype(np.uint8), [g.ravel().astype(np.uint8)])
    assert len(every[1]) == 256 * 511 and len(every[1]) % 4 == 0
    rng = np.random.default_rng(20)
    out = [every]
    for n_gray in (0, 5, 16):
        n = 4096
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        mean = (a.astype(np.int32) + b) // 2
        # Gray bytes around the pixel's own threshold, ties included, so that both bits and the tie occur everywhere
        gray = [np.clip(mean + rng.integers(-3, 4, n), 0, 255).astype(np.uint8) for _ in range(n_gray)]
        out.append((f"{n_gray} random planes", a, b, gray))
    return out


def _decode_cases(d, exe, env=None):
    for k, (name, i0, i2, gray) in enumerate(_stacks()):
        src, out = str(d / f"dg{k}.bin"), str(d / f"dg{k}.out")
        with open(src, "wb") as f:
            np.array([len(i0)], np.int64).tofile(f)
            np.array([len(gray)], np.int32).tofile(f)
            i0.tofile(f)
            i2.tofile(f)
            for g in gray:
                g.tofile(f)
        subprocess.check_call([exe, src, out], timeout=120, env=env)
        got = np.fromfile(out, np.int32).reshape(2, -1)
        want = DG.code(gray, i0, i2)
        assert got.shape == (2, len(i0))
        assert np.array_equal(got[0], want), f"{name}: direct_gray_code against the restatement"
        assert np.array_equal(got[1], want), f"{name}: the packed forms against the restatement"
        if len(gray) == 1:
            assert 0 < want.sum() < len(want) and np.array_equal(want == 1, 2 * gray[0].astype(np.int32) >= i0.astype(np.int32) + i2), "ties -> 1"
        print(f"{name}: {len(i0)} pixels, {len(gray)} planes, codes 0..{int(want.max())}")


def test_header_agrees_with_the_restatement(tmp_path):
    exe = str(tmp_path / "direct_gray_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    subprocess.check_call([exe], timeout=120)
    _decode_cases(tmp_path, exe)


def test_header_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program with the address and undefined-behaviour sanitizers (nothing here runs inside Python)."""
    exe = str(tmp_path / "direct_gray_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([exe], timeout=300, env=env)
    _decode_cases(tmp_path, exe, env=env)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def _capture(size, n_fringe, noise, gain, optics="N7_fw4"):
    syn = importlib.import_module("3dscan_amd.synth")
    pw, ph, n, fw = OPTICS[optics]
    return syn.make_capture(size[0], size[1], pw, ph, n, n, fw, fw, n_fringe=n_fringe, noise=noise, gain=gain, offset=10.0)


@pytest.mark.parametrize("gain", [0.8, 0.3, 0.05])
@pytest.mark.parametrize("noise", [0, 2])
@pytest.mark.parametrize("n_fringe", [3, 4])
@pytest.mark.parametrize("size", [(90, 60), (320, 240)])
@pytest.mark.parametrize("optics", list(OPTICS))
def test_direct_code_equals_inverse_code_on_every_lit_pixel(optics, size, n_fringe, noise, gain):
    N = OPTICS[optics][2]
    cap = _capture(size, n_fringe, noise, gain, optics)
    lit = cap["lit"]
    assert 0.5 * lit.size < lit.sum() < lit.size, "the scene has lit and unlit pixels"
    differing_unlit = 0
    for planes in (cap["planes_v"], cap["planes_h"]):
        fr, gray, inv = DG.split(planes, n_fringe, N)
        direct, inverse = DG.code(gray, fr[0], fr[2]), DG.inverse_code(gray, inv)
        n_diff = int((direct != inverse)[lit].sum())
        print(f"{optics} {size} F={n_fringe} noise={noise} gain={gain}: {n_diff} differing lit pixels of {int(lit.sum())}, {int((direct != inverse)[~lit].sum())} unlit of {int((~lit).sum())}")
        assert n_diff == 0
        if noise == 0:
            assert np.array_equal(direct, inverse), "without noise the two decodes agree on every pixel (an unlit pixel is a tie in both)"
        differing_unlit += int((direct != inverse)[~lit].sum())
    if noise:
        assert differing_unlit > 0, "under noise the unlit pixels decode to noise in both, and differently"


@pytest.mark.parametrize("n_fringe", [3, 4])
def test_the_restated_codes_are_the_oracles(n_fringe):
    """inverse_code is the oracle's code of the capture; code is the oracle's code of the as_inverse_coded() planes -- on the pixels the
    oracle decodes (elsewhere it leaves -1) -- and there the oracle's whole scan agrees between the two plane sets on the lit pixels."""
    W, H = 320, 240
    cap = _capture((W, H), n_fringe, 2, 0.8)
    cal = importlib.import_module("3dscan_amd.synth").cal_tuple(cap["cal"])
    scans = []
    for coded in (False, True):
        pv, ph = ([DG.as_inverse_coded(p, n_fringe, N) for p in (cap["planes_v"], cap["planes_h"])] if coded else (cap["planes_v"], cap["planes_h"]))
        o = Oracle(W, H, PW, PH, N, N, FW, FW, F=n_fringe)
        o.set_mask(cap["mask"])
        o.set_calibration(*cal)
        o.run_scan(pv, ph)
        scans.append(dict(code=(o.code(0).copy(), o.code(1).copy()), sel=(o.valid_map(0).copy(), o.valid_map(1).copy()), valid=o.valid_map(2).copy(),
                          unw=(o.unwrapped_phi(0).copy(), o.unwrapped_phi(1).copy()), w=(o.wrapped_phi(0).copy(), o.wrapped_phi(1).copy()),
                          ipoints=o.intersection_points().copy()))
        o.close()
    plain, coded = scans
    for axis, planes in enumerate((cap["planes_v"], cap["planes_h"])):
        fr, gray, inv = DG.split(planes, n_fringe, N)
        sel = plain["sel"][axis] == 1
        assert sel.sum() > 60000 and np.array_equal(plain["sel"][axis], coded["sel"][axis]), "stage 3 does not look at the Gray planes"
        assert np.array_equal(plain["code"][axis][sel], DG.inverse_code(gray, inv)[sel]) and (plain["code"][axis][~sel] == -1).all()
        direct = DG.code(gray, fr[0], fr[2])
        assert np.array_equal(coded["code"][axis][sel], direct[sel]) and (coded["code"][axis][~sel] == -1).all()
        assert np.array_equal(coded["unw"][axis][sel].view(np.uint32), DG.absolute(coded["w"][axis], direct)[sel].view(np.uint32)), "absolute() is stage 4's float"
    lit = cap["lit"] & (plain["valid"] == 1)
    assert np.array_equal((coded["valid"] == 1)[cap["lit"]], (plain["valid"] == 1)[cap["lit"]])
    assert np.array_equal(coded["ipoints"][lit], plain["ipoints"][lit]), "on the lit pixels the 13 + 13 frames give the scan of the 23 + 23"


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def test_a_scan_without_inverse_frames_is_as_accurate():
    """The vertical-only anchored scan of tests/one_axis_cases.py (3 fringe + 7 Gray frames read instead of 3 + 14) against the true plane."""
    s, o = OC.scene(0, "full"), OC.oracle_scan(0, "full")
    cap = s["cap"]
    good = SC.good_pixels(cap, o["c_p_map"], o["valid"])
    assert good.sum() > 60000
    sel = o["valid_axis"][0]
    direct = DG.code_of_planes(DG.read_planes(cap["planes_v"], 3, OC.N[0]), 3, OC.N[0])
    assert np.array_equal(direct[good], o["code"][0][good])
    code_d = np.where(sel == 1, direct, -1).astype(np.int32)
    unw_d = np.where(sel == 1, DG.absolute(o["w"][0], direct), np.float32(0)).astype(np.float32)   # (the mask's border keeps columns 0 and W - 1 out)
    rms = []
    for code, unw in ((o["code"][0], o["unw"][0]), (code_d, unw_d)):
        r = OR.scan(o["w"][0], code, unw, sel, s["cal"], o["A_cam"], o["A_proj"], 0, OC.FW[0], OC.EXTENT[0], OC.N[0], 3, s["origin"], OC.FULL, True)
        assert (r["valid"] == 1)[good].all()
        rms.append(SC.plane_rms(r["ipoints"], good))
    print(f"RMS to the plane over {int(good.sum())} pixels: {rms[0]:.6f} mm from 3 + 14 frames, {rms[1]:.6f} mm from 3 + 7 frames")
    assert rms[1] == rms[0]


def test_a_13_frame_scan_is_as_accurate_as_the_23_frame_scan():
    """The headline configuration: 3 phase-shift + 10 Gray-code frames.  320 x 240 camera, 2048 x 1536 projector, N = 10, fringe width 2,
    noise +-2; vertical only, anchored: the scan from the 13 frames a flagged context reads against the scan from all 23, RMS distance to the
    true plane over the good_pixels of the two-axis scan."""
    syn = importlib.import_module("3dscan_amd.synth")
    W, H = 320, 240
    pw, ph, n, fw = OPTICS["N10_fw2"]
    cap = _capture((W, H), 3, 2, 0.8, "N10_fw2")
    cal = syn.cal_tuple(cap["cal"])
    assert len(cap["planes_v"]) == 23 and len(DG.read_planes(cap["planes_v"], 3, n)) == 13
    o = Oracle(W, H, pw, ph, n, n, fw, fw)
    o.set_mask(cap["mask"])
    o.set_calibration(*cal)
    o.run_scan(cap["planes_v"], cap["planes_h"])
    A, B = o.projection_matrices()
    w, code23, unw23, sel = o.wrapped_phi(0).copy(), o.code(0).copy(), o.unwrapped_phi(0).copy(), o.valid_map(0).copy()
    good = SC.good_pixels(cap, o.c_p_map(), o.valid_map(2))
    o.close()
    # (a precondition of the scene, not a bar on the decode: under +-2 noise on a 2-pixel fringe fewer integer correspondences lie within
    # 1.5 px of the analytic ones than at fringe width 4 -- the figure is taken over more than half of the lit pixels)
    assert good.sum() > 0.5 * cap["lit"].sum()
    direct = DG.code_of_planes(DG.read_planes(cap["planes_v"], 3, n), 3, n)
    assert direct.max() > 512, "the upper Gray planes carry information"
    assert np.array_equal(direct[good], code23[good]) and np.array_equal(direct[cap["lit"]], DG.inverse_code(*DG.split(cap["planes_v"], 3, n)[1:])[cap["lit"]])
    code13 = np.where(sel == 1, direct, -1).astype(np.int32)
    unw13 = np.where(sel == 1, DG.absolute(w, direct), np.float32(0)).astype(np.float32)   # (the mask's border keeps columns 0 and W - 1 out)
    rms = []
    for code, unw in ((code23, unw23), (code13, unw13)):
        r = OR.scan(w, code, unw, sel, cal, A, B, 0, fw, pw, n, 3, (0, 0), (W, H), True)
        assert (r["valid"] == 1)[good].all()
        rms.append(SC.plane_rms(r["ipoints"], good))
    print(f"RMS to the plane over {int(good.sum())} pixels: {rms[0]:.6f} mm from 3 + 20 frames, {rms[1]:.6f} mm from 3 + 10 frames")
    assert rms[1] == rms[0] and rms[0] < 0.1
