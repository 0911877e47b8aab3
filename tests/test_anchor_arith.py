"""CPU tests of the anchored projector coordinate (SL3D_FLAG_ANCHOR_PERIODS), before any GPU time is spent.

(a) The restatement's inputs are stage 4's: on the oracle's planes of every scene of tests/subpixel_cases.py float(w + code * 2 * 22/7)
    reproduces the unwrapped plane on the valid pixels.
(b) What the feature is for, on ("plain", "full"): with S the lit valid pixels whose anchored coordinates lie within 0.5 px of the analytic
    ones on both axes, S holds at least 99.5 % of the lit valid pixels (the cap that keeps the selection from hiding failures; today's
    coordinates: 95.5 %), the RMS distance to the true plane over S is at most 0.1 of the sub-pixel figure over good_pixels, and the median
    reprojection residual over S is at most 0.01 px.
(c) The 4-step constant c_4 on ideal, unquantised 4-step patterns: |mean error| <= 5e-4 px with it, > 2e-3 px without.
(d) The header every kernel and sl3d_create compile (3dscan_amd/csrc/sl3d_anchor.h) through a stand-alone program
    (tests/native/anchor_check.cpp): bit for bit the restatement over a lattice of codes, phases and both fringe counts, the phases either
    side of every tie of m included; the same program also under the address and undefined-behaviour sanitizers.
(e) Report only: how often m differs from the code on the crops of a real capture (tests/golden/real_*.npz)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from oracle.oracle import Oracle

import anchor_reference as AR
import subpixel_cases as SC
import subpixel_reference as SR

SRC = os.path.join(ROOT, "tests", "native", "anchor_check.cpp")
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]


@functools.lru_cache(maxsize=None)
def stage4_planes(win):
    """The wrapped-phase and code planes the oracle's stage 4 leaves (the decode does not depend on the rig): dict(w (v, h), code (v, h)),
    a window's cut out of the whole frame's as in subpixel_cases.oracle_scan."""
    if win != "full":
        (W, H), (col0, row0) = SC.WINDOWS[win]
        return {k: tuple(np.ascontiguousarray(a[row0:row0 + H, col0:col0 + W]) for a in v) for k, v in stage4_planes("full").items()}
    s = SC.scene("plain", "full")
    o = Oracle(s["W"], s["H"], SC.PW, SC.PH, SC.N, SC.N, SC.FW, SC.FW)
    o.set_mask(s["cap"]["mask"])
    o.set_calibration(*s["cal"])
    o.run_scan(s["cap"]["planes_v"], s["cap"]["planes_h"])
    out = dict(w=(o.wrapped_phi(0).copy(), o.wrapped_phi(1).copy()), code=(o.code(0).copy(), o.code(1).copy()))
    o.close()
    return out


def anchored_xy(rig, win):
    s, o, p = SC.scene(rig, win), SC.oracle_scan(rig, win), stage4_planes(win)
    return AR.correspondences(p["w"], p["code"], o["unw"], o["valid_axis"], (SC.FW, SC.FW), 3, (SC.N, SC.N), s["origin"], SC.FULL)


def accuracy(cap, valid, xy, ipoints, residual):
    """(share of the lit valid pixels in S, RMS plane distance over S in mm, median residual over S in px, |S|) -- the figures of (b)."""
    lit = (valid == 1) & cap["lit"]
    with np.errstate(invalid="ignore"):
        S = lit & (np.abs(xy[..., 0] - cap["xp"]) <= 0.5) & (np.abs(xy[..., 1] - cap["yp"]) <= 0.5)
    return S.sum() / lit.sum(), SC.plane_rms(ipoints, S), float(np.median(residual[S])), int(S.sum())


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,win", SC.SCENES)
def test_the_inputs_are_stage_4s(rig, win):
    s, o, p = SC.scene(rig, win), SC.oracle_scan(rig, win), stage4_planes(win)
    m = o["valid"] == 1
    assert m.sum() > 500
    for axis in (0, 1):
        w, code, unw = p["w"][axis], p["code"][axis], o["unw"][axis]
        assert w.dtype == np.float32 and unw.dtype == np.float32
        where = m & AR.applies(axis, m.shape, s["origin"], SC.FULL, SC.N)
        assert where.sum() == m.sum(), "every valid pixel of these scenes lies where stage 4's loop runs"
        again = (w.astype(np.float64) + ((code.astype(np.float64) * 2.0) * 22.0) / 7.0).astype(np.float32)
        assert np.array_equal(again[where].view(np.uint32), unw[where].view(np.uint32)), (rig, win, axis)
        assert (code[where] >= 0).all() and (w[where] >= 0).all() and (w[where] < AR.P2 + 1e-3).all()


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def test_accuracy_against_the_subpixel_coordinates():
    s, o = SC.scene("plain", "full"), SC.oracle_scan("plain", "full")
    cap = s["cap"]
    lit = (o["valid"] == 1) & cap["lit"]
    assert lit.sum() > 70000
    plain_xy = SR.correspondences(*o["unw"], *o["valid_axis"], SC.FW, SC.FW)
    plain = SR.triangulate(plain_xy, o["valid"], s["cal"], o["A_cam"], o["A_proj"], s["origin"])
    xy = anchored_xy("plain", "full")
    anch = SR.triangulate(xy, o["valid"], s["cal"], o["A_cam"], o["A_proj"], s["origin"])
    assert np.array_equal(anch["valid"], o["valid"]), "validity does not change"
    good = SC.good_pixels(cap, o["c_p_map"], o["valid"])
    bar = SC.plane_rms(plain["ipoints"], good)
    share0, rms0, med0, _ = accuracy(cap, o["valid"], plain_xy, plain["ipoints"], plain["residual"])
    share, rms, med, n = accuracy(cap, o["valid"], xy, anch["ipoints"], anch["residual"])
    with np.errstate(invalid="ignore"):
        off = lambda c: int((lit & ((np.abs(c[..., 0] - cap["xp"]) > SC.FW / 2) | (np.abs(c[..., 1] - cap["yp"]) > SC.FW / 2))).sum())
    print(f"lit valid {int(lit.sum())}; off by more than fw/2: as it is {off(plain_xy)}, anchored {off(xy)}; within 0.5 px on both axes: as it is "
          f"{share0:.4%}, anchored {share:.4%} ({n}); RMS to the plane: sub-pixel over good_pixels {bar:.4f} mm, anchored over S {rms:.4f} mm, ratio "
          f"{rms / bar:.3f}; median residual: as it is {med0:.4f} px, anchored {med:.4f} px; max anchored ys {np.nanmax(xy[..., 1]):.3f}")
    assert share >= 0.995
    assert share0 < 0.97, "today's coordinates must miss the cap for the test to see the feature"
    assert rms <= 0.1 * bar
    assert med <= 0.01


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def test_the_four_step_constant():
    fw, Pi = 16, 22.0 / 7.0
    p = np.arange(1, 1900 * 4 + 1, dtype=np.float64) / 4.0                       # quarter pixels up to 1900
    I = [127.0 + 128.0 * np.cos((p / fw) * (2.0 * Pi) - Pi + k * (Pi / 2.0)) for k in range(4)]
    phi = np.arctan2(I[3] - I[1], I[0] - I[2]).astype(np.float32)               # stage 3, 4 steps: atan2(I3 - I1, I0 - I2)
    w = (phi.astype(np.float64) + Pi).astype(np.float32)                        # stage 4: += Pi
    code = np.floor(p / fw).astype(np.int64)
    means = {}
    for name, offset in (("c_4", None), ("zero", 0.0)):
        err = AR.coordinate(w, code, fw, 4, offset=offset) - p
        inside = np.abs(err) <= fw / 2
        assert inside.mean() > 0.98                                               # (1 position in 64 sits on a cell's edge: a tie by construction)
        means[name] = float(err[inside].mean())
        print(f"4 steps, {name}: mean error {means[name]:.3e} px, RMS {np.sqrt(np.mean(err[inside] ** 2)):.3e} px, off by a period {int((~inside).sum())} of {len(p)}")
    assert abs(means["c_4"]) <= 5e-4
    assert abs(means["zero"]) > 2e-3
    # the 3-step form needs none
    I = [127.0 + 128.0 * np.cos((p / fw) * 2.0 * Pi - Pi - Pi / 2.0 + (Pi / 2.0) * k) for k in range(3)]
    w = (np.arctan2(I[0] - I[2], 2.0 * I[1] - I[0] - I[2]).astype(np.float32).astype(np.float64) + Pi).astype(np.float32)
    err = AR.coordinate(w, code, fw, 3) - p
    inside = np.abs(err) <= fw / 2
    print(f"3 steps: mean error {err[inside].mean():.3e} px, RMS {np.sqrt(np.mean(err[inside] ** 2)):.3e} px, off by a period {int((~inside).sum())}")
    assert inside.mean() > 0.98 and abs(err[inside].mean()) <= 5e-4


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------
CODES = np.array(list(range(128)) + [65535], np.int32)


def lattice():
    """About 4,000 floats in [0, 2 * 22/7): an even spread, and for every code and fringe count the phase at which m ties and its two
    neighbours."""
    ws = [np.linspace(0.0, AR.P2, 2500, endpoint=False).astype(np.float32), np.array([0.0, np.nextafter(np.float32(AR.P2), np.float32(0))], np.float32)]
    for n_fringe in (3, 4):
        for code in CODES:
            centre = (float(code) + 0.5) * AR.P2
            k = np.floor(centre * AR.INV)                                        # the ties: a = centre - (k + 0.5) * TWOPI
            for kk in (k - 1, k, k + 1):
                a = centre - (kk + 0.5) * AR.TWOPI
                t = np.float32(a - AR.phase_offset(n_fringe))
                if 0.0 <= t < AR.P2:
                    ws.append(np.array([np.nextafter(t, np.float32(-1)), t, np.nextafter(t, np.float32(9))], np.float32))
    w = np.unique(np.concatenate(ws))
    return w[(w >= 0) & (w < np.float32(AR.P2))]


def _lattice_case(d, exe, env=None):
    w, fw = lattice(), 16
    assert 3000 < len(w) < 5000
    src, out = str(d / "lattice.bin"), str(d / "lattice.out")
    with open(src, "wb") as f:
        np.array([len(w), len(CODES)], np.int64).tofile(f)
        np.array([fw], np.int32).tofile(f)
        w.tofile(f)
        CODES.tofile(f)
    subprocess.check_call([exe, src, out], timeout=120, env=env)
    got = np.fromfile(out, np.float64).reshape(2, len(CODES), len(w))
    ties = 0
    for i, n_fringe in enumerate((3, 4)):
        want = AR.coordinate(np.broadcast_to(w, (len(CODES), len(w))), np.broadcast_to(CODES.astype(np.int64)[:, None], (len(CODES), len(w))), fw, n_fringe)
        assert np.array_equal(got[i].view(np.uint64), want.view(np.uint64)), (n_fringe, int((got[i].view(np.uint64) != want.view(np.uint64)).sum()))
        m = AR.period(np.broadcast_to(w, want.shape), np.broadcast_to(CODES.astype(np.int64)[:, None], want.shape), n_fringe)
        ties += int((np.diff(m, axis=1) != 0).sum())
    assert ties >= 2 * len(CODES), "the lattice must cross a tie of m for every code and fringe count"


def test_header_equals_the_restatement_bit_for_bit(tmp_path):
    exe = str(tmp_path / "anchor_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    subprocess.check_call([exe], timeout=60)
    _lattice_case(tmp_path, exe)


def test_header_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program with the address and undefined-behaviour sanitizers (nothing here runs inside Python)."""
    exe = str(tmp_path / "anchor_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([exe], timeout=60, env=env)
    _lattice_case(tmp_path, exe, env=env)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real_edge", "real_inside"])
def test_report_on_the_real_crops(name):
    """Report only: the share of valid pixels whose fringe period differs from the Gray code on a crop of a real capture."""
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    if not all(k in d.files for k in ("wrapped_v", "wrapped_h", "code_v", "code_h", "valid")):
        print(f"{name}: the crop does not hold the wrapped phase and the code")
        return
    v = d["valid"] == 1
    for axis, s in enumerate("vh"):
        m = AR.period(d["wrapped_" + s][v], d["code_" + s][v].astype(np.int64), 3)
        print(f"{name}, axis {axis}: m != code on {int((m != d['code_' + s][v]).sum())} of {int(v.sum())} valid pixels ({(m != d['code_' + s][v]).mean():.2%})")
