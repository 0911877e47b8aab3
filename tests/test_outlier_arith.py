"""CPU tests of the outlier filter's arithmetic (3dscan_amd/csrc/sl3d_outlier.h -- the header k_outlier_support and k_outlier_apply compile,
free of HIP) and of the NumPy restatement of the rule (tests/outlier_reference.py).

The header runs through tests/native/outlier_check.cpp, a stand-alone program built by g++ twice: plainly, and with
-fsanitize=address,undefined (every check runs on both; it runs as a child process).  It evaluates the crafted cases the GPU tests use
(tests/outlier_reference.py: holes, step, all valid, none valid, corners; the tie lattice; non-finite and huge coordinates; the Jacobi
lines) over pitched planes whose padding columns are poisoned -- a valid byte of 1 and a point within max_dist of the row's points -- and
every support byte and every rejection is compared with the restatement.

The restatement on the step scene of the issue (37 x 130, two planes 30 mm apart, 2 % speckle, four columns of flying pixels): the planted
pixels go, the others stay."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import outlier_reference as OR

SRC = os.path.join(ROOT, "tests", "native", "outlier_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SHAPES = [(1, 1), (3, 2), (9, 9), (67, 19), (130, 37)]                 # (W, H)


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("outlier_" + request.param) / "outlier_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *FLAGS[request.param], SRC, "-o", exe])
    return exe


def _pitched(xyz, valid, pad):
    """the planes at a pitch of the next multiple of 16 plus 16, the padding poisoned: valid bytes of 1 over the point (pad, pad, pad)"""
    H, W = valid.shape
    pitch = ((W + 15) & ~15) + 16
    pv = np.ones((H, pitch), np.uint8)
    pp = np.full((H, pitch, 3), pad, np.float32)
    pv[:, :W], pp[:, :W] = valid, xyz
    return pitch, pv, pp


def _run(exe, tmp_path, cases):
    """cases: [(xyz, valid, radius, max_dist, min_neighbours, pad)] -> [(support, rejected)] of the C header"""
    blob = [struct.pack("<i", len(cases))]
    for xyz, valid, radius, max_dist, min_n, pad in cases:
        H, W = valid.shape
        pitch, pv, pp = _pitched(xyz, valid, pad)
        blob += [struct.pack("<5if", W, H, pitch, radius, min_n, np.float32(max_dist)), pv.tobytes(), pp.tobytes()]
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(blob))
    subprocess.check_call([exe, str(src), str(out)], timeout=600)
    got, res = np.fromfile(str(out), np.uint8), []
    for _, valid, *_ in cases:
        n = valid.size
        res.append((got[:n].reshape(valid.shape), got[n:2 * n].reshape(valid.shape).astype(bool)))
        got = got[2 * n:]
    assert got.size == 0
    return res


def _check(exe, tmp_path, cases, tags):
    for (xyz, valid, radius, max_dist, min_n, _), (support, rejected), tag in zip(cases, _run(exe, tmp_path, cases), tags):
        want = OR.filter_outliers(xyz, valid, radius, max_dist, min_n)
        assert np.array_equal(support, want["support"]), (tag, int((support != want["support"]).sum()), "support bytes differ")
        assert np.array_equal(rejected, want["rejected"]), (tag, "rejections differ")


def test_crafted_cases_equal_the_restatement(checker, tmp_path):
    cases, tags = [], []
    for W, H in SHAPES:
        for radius in (1, 2, 3, 4):
            for name, xyz, valid in OR.crafted_cases(H, W):
                cases.append((xyz, valid) + OR.PARAMS[radius] + (OR.PAD,))
                tags.append((W, H, radius, name))
    _check(checker, tmp_path, cases, tags)
    # the yardstick's inputs do what they are for: some cases reject some and keep some, the padding would have counted
    counts = [OR.filter_outliers(*c[:5])["counts"] for c in cases[40:]]
    assert sum(0 < rejected < samples for samples, rejected in counts) >= 30
    # ... and a window that ended at the pitch would have counted the padding
    xyz, valid = OR.crafted_cases(19, 67)[2][1:]
    _, pv, pp = _pitched(xyz, valid, OR.PAD)
    assert not np.array_equal(OR.support_plane(pp, pv, 2, 1.5)[:, :67], OR.support_plane(xyz, valid, 2, 1.5))


def test_ties_nonfinite_and_jacobi_lines(checker, tmp_path):
    lx, lv = OR.tie_lattice()
    below = np.nextafter(np.float32(5), np.float32(0))
    nx, nv, special = OR.nonfinite_case()
    row = OR.jacobi_line(19, 130, [(9, c) for c in range(60, 70)])
    col = OR.jacobi_line(19, 67, [(r, 33) for r in range(5, 13)])
    cases = [(lx, lv, 1, 5.0, 8, 0), (lx, lv, 1, below, 8, 0), (lx, lv, 2, np.inf, 24, 0), (lx, lv, 4, np.inf, 80, 0),
             (nx, nv, 2, 1.5, 8, OR.PAD), (nx, nv, 4, np.inf, 1, OR.PAD), (row[0], row[1], 1, 1.0, 2, 0), (col[0], col[1], 2, 1.0, 2, 0)]
    _check(checker, tmp_path, cases, list(range(len(cases))))
    # what the restatement says on them
    s5, sb = OR.support_plane(lx, lv, 1, 5.0), OR.support_plane(lx, lv, 1, below)
    assert (s5[1:-1, 1:-1] == 8).all() and (sb[1:-1, 1:-1] == 4).all() and s5[0, 0] == 3 and sb[0, 0] == 2     # <= counts the tie
    H, W = lv.shape
    si = OR.support_plane(lx, lv, 2, np.inf)
    assert si[3, 4] == 24 and si[0, 0] == 8 and OR.support_plane(lx, lv, 4, np.inf)[3, 4] == min(W, 9) * min(H, 9) - 1
    sn = OR.support_plane(nx, nv, 2, 1.5)
    for name in ("nan", "inf", "ninf", "huge", "nhuge"):
        assert all(sn[r, c] == 0 for r, c in special[name]), name
    assert sn[4, 7] == 1 and sn[4, 8] == 1 and (sn[nv == 0] == OR.NO_SAMPLE).all() and (sn[nv == 1] != OR.NO_SAMPLE).all()
    f = OR.filter_outliers(row[0], row[1], 1, 1.0, 2)
    assert f["counts"] == (10, 2) and f["rejected"][9, 60] and f["rejected"][9, 69]


@pytest.mark.parametrize("params,planted_min,other_max", [((1, 1.0, 3), 245, 0), ((2, 1.5, 8), 249, 1), ((4, 2.5, 20), 246, 0)])
def test_restatement_on_the_step_scene(params, planted_min, other_max):
    xyz, valid, planted = OR.step_scene()
    other = (valid == 1) & ~planted
    assert int(planted.sum()) == 250 and int(other.sum()) == 4432
    f = OR.filter_outliers(xyz, valid, *params)
    hit, lost = int((f["rejected"] & planted).sum()), int((f["rejected"] & other).sum())
    print(f"{params}: {hit} of 250 planted pixels rejected, {lost} of 4432 others")
    assert (hit, lost) == (planted_min, other_max)
    if params == (2, 1.5, 8):
        assert hit >= 0.95 * 250 and lost <= 0.001 * 4432
    assert f["counts"] == (4682, hit + lost) and np.array_equal(f["valid"] == 1, (valid == 1) & ~f["rejected"])
    assert (f["bits"][f["rejected"]] == OR.NAN_BITS).all()
    assert np.array_equal(f["bits"][~f["rejected"]], xyz.view(np.uint32)[~f["rejected"]])
