"""CPU tests of the turntable refinement's arithmetic (3dscan_amd/csrc/sl3d_align.h -- the header k_align_pass compiles, free of HIP)
against the NumPy restatement of the rule (tests/align_reference.py).

The header runs through tests/native/align_check.cpp, built by g++ twice: plainly, and as the same stand-alone program with
-fsanitize=address,undefined (every check runs on both).  The step into the target's frame, the projection, the centre pixel and its
range test over 2^17 hashed float bit patterns (every exponent: denormals, infinities, NaNs among them), hashed points of a scan's size
and the specials -- a camera depth of exactly 0 and negative ones, projections exactly on .5 (ties to even), centres at and beyond 2^30 --
for four cameras: distorted, undistorted, tangential with a skewed and perspective Kc, and the identity camera that makes the specials
exact.  The squared distance over hashed pairs; the acceptance and the quantisation with |e| just below and at 2^18 and d2 exactly
max_dist^2 (accepted) and the next double above (not).  Everything bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import align_reference as AR

SRC = os.path.join(ROOT, "tests", "native", "align_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
CENTRE_OUT = np.dtype([("ph", "<f8", 3), ("cc", "<f8"), ("rr", "<f8"), ("finite", "<i4"), ("ok", "<i4")])
D2_IN = np.dtype([("ph", "<f8", 3), ("q", "<f4", 3), ("pad", "<f4")])
ACCEPT_IN = np.dtype([("d2", "<f8"), ("p", "<f4", 3), ("q", "<f4", 3)])
ACCEPT_OUT = np.dtype([("t", "<i8", 5), ("ok", "<i8")])

REF = dict(Kc=(282.29, 0.0, 158.79, 0.0, 283.64, 118.32, 0.0, 0.0, 1.0), rc=(-0.0199, -0.2865, 0.0038), tc=(-50.78, -39.23, 103.29))
CAMERAS = {
    "distorted": AR.camera_of(REF["Kc"], (0.0813, -0.1102, 0.0, 0.0, 0.0), REF["rc"], REF["tc"]),
    "undistorted": AR.camera_of(REF["Kc"], (0.0, 0.0, 0.0, 0.0, 0.0), REF["rc"], REF["tc"]),
    "skewed": AR.camera_of((282.29, 1.75, 158.79, 0.25, 283.64, 118.32, 1e-4, -2e-4, 1.0), (0.05, -0.02, 0.003, -0.002, 0.01), REF["rc"], REF["tc"]),
    "identity": AR.camera_of((1.0, 0.0, 0.5, 0.0, 1.0, 0.5, 0.0, 0.0, 1.0), (0.0,) * 5, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
}
ESTIMATES = {"step": AR.estimate(20.0, 31.5, -12.25), "identity": np.array([1.0, 0.0, 0.0, 0.0])}


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_" + request.param) / "align_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *FLAGS[request.param], SRC, "-o", exe])
    return exe


def _run(exe, tmp_path, what, data, dtype):
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    subprocess.check_call([exe, what, src, out], timeout=600)
    return np.fromfile(out, dtype=dtype)


def _hash32(t):
    t = t.astype(np.uint64)
    m = np.uint64(0xffffffff)
    t ^= t >> np.uint64(16)
    t = (t * np.uint64(0x7feb352d)) & m
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x846ca68b)) & m
    t ^= t >> np.uint64(16)
    return t


def _scan(n, salt, span=160.0):
    return ((_hash32(np.arange(n) + salt).astype(np.float64) / 2.0**32 - 0.5) * span).astype(np.float32)


def _points():
    n = 1 << 17
    bits = _hash32(np.arange(3 * n)).astype(np.uint32).view(np.float32).reshape(n, 3)          # every kind of float
    scan = np.stack([_scan(n, 1 << 22) + 50, _scan(n, 2 << 22) + 40, _scan(n, 3 << 22, 60.0)], axis=1)
    mixed = scan[:4096].copy()                                                                  # one odd coordinate in a point of the scan
    mixed[np.arange(4096), np.arange(4096) % 3] = bits[:4096, 0]
    tiny = np.array([1, 2, 0x7fffff, 0x800000, 0x80000001, 0x807fffff, 0x7f7fffff, 0xff7fffff], dtype=np.uint32).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0, -1.0], dtype=np.float32)
    odd = np.concatenate([tiny, special])
    grid = np.stack(np.meshgrid(odd, odd[:6], odd, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([bits, scan, mixed, grid]).astype(np.float32)


def _exact_points():
    """for the identity camera and estimate (u = x / z + 0.5, v = y / z + 0.5, p^ = p): depth exactly 0 and negative, u and v exactly on
    .5 for even and odd integers of both signs, centres around 2^30 and beyond every integer"""
    k = np.arange(-9, 10, dtype=np.float32)
    ties = np.stack([k, k[::-1], np.ones_like(k)], axis=1)                                       # u = k + 0.5
    half = np.stack([k + np.float32(0.5), k - np.float32(0.25), np.ones_like(k)], axis=1)        # u = k + 1: no tie
    depth = np.array([[3.0, 4.0, 0.0], [3.0, 4.0, -0.0], [3.0, 4.0, -1.0], [0.0, 0.0, 0.0], [1.0, 1.0, -1e-30], [1.0, 1.0, 1e-30],
                      [1.0, 1.0, 1e-45], [1.0, 1.0, 3e38], [3e38, 1.0, 1e-38]], dtype=np.float32)
    big = np.array([[2.0**30 - 64, 0.0, 1.0], [2.0**30, 0.0, 1.0], [-(2.0**30) + 64, 0.0, 1.0], [-(2.0**30), 0.0, 1.0], [0.0, 2.0**30 - 64, 1.0],
                    [0.0, 2.0**30, 1.0], [2.0**31, 2.0**31, 1.0], [2.0**62, 1.0, 1.0], [1.0, 2.0**64, 1.0]], dtype=np.float32)   # (floats up there are 64 apart)
    return np.concatenate([ties, half, depth, big]).astype(np.float32)


@pytest.mark.parametrize("est", list(ESTIMATES))
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_step_projection_and_centre(checker, tmp_path, camera, est):
    cam, e = CAMERAS[camera], ESTIMATES[est]
    col0, row0 = (37, 5) if camera != "identity" else (0, 0)
    p = np.concatenate([_points(), _exact_points()])
    head = cam.tobytes() + e.tobytes() + np.array([col0, row0], np.int32).tobytes()
    got = _run(checker, tmp_path, "centre", head + p.tobytes(), CENTRE_OUT)
    assert got.shape == (len(p),)
    ph = AR.step(p, e)
    same = (got["ph"].view(np.uint64) == ph.view(np.uint64)) | (np.isnan(got["ph"]) & np.isnan(ph))
    assert same.all()
    finite = np.isfinite(p).all(axis=1)
    assert np.array_equal(got["finite"] != 0, finite)
    cc, rr, ok = AR.centre(ph, cam, col0, row0)
    ok &= finite
    assert np.array_equal(got["ok"] != 0, ok)
    assert np.array_equal(got["cc"][ok], cc[ok]) and np.array_equal(got["rr"][ok], rr[ok])
    assert (got["cc"][~ok] == 0).all() and (got["rr"][~ok] == 0).all()
    assert np.isfinite(ph[finite]).all()                                    # what sl3d_align.h says of a finite source
    assert ok.sum() > 1000 and (finite & ~ok).sum() > 1000                  # both outcomes are exercised
    if camera != "identity":
        inside = ok & (cc >= 0) & (cc < 200) & (rr >= 0) & (rr < 200)
        assert inside.sum() > 1000                                          # ... and centres that land in a frame


def test_the_exact_specials():
    """by the restatement alone, on the identity camera: what each special input is for"""
    cam, e, p = CAMERAS["identity"], ESTIMATES["identity"], _exact_points()
    ph = AR.step(p, e)
    assert np.array_equal(ph, p.astype(np.float64))
    cc, rr, ok = AR.centre(ph, cam, 0, 0)
    k = np.arange(-9, 10)
    assert ok[:19].all() and np.array_equal(cc[:19], 2.0 * np.floor((k + 1) / 2.0))            # k + 0.5 goes to the even neighbour
    assert np.array_equal(cc[19:38], k + 1.0) and ok[19:38].all()
    depth = ok[38:47]
    assert list(depth) == [False, False, False, False, False, False, False, True, False]
    big = ok[47:]
    assert list(big) == [True, False, True, False, True, False, False, False, False]
    assert cc[47] == 2.0**30 - 64 and cc[49] == -(2.0**30) + 64 and rr[51] == 2.0**30 - 64   # ... - 63.5 and + 64.5: ties, to the even side


def test_squared_distance(checker, tmp_path):
    n = 1 << 16
    rec = np.zeros(n + 64, D2_IN)
    rec["ph"][:n] = np.stack([_scan(n, 5 << 22).astype(np.float64) * 1.0000001, _scan(n, 6 << 22) * 0.37, _scan(n, 7 << 22) / 3.0], axis=1)
    rec["q"][:n] = (rec["ph"][:n] + np.stack([_scan(n, 8 << 22, 4.0), _scan(n, 9 << 22, 4.0), _scan(n, 10 << 22, 4.0)], axis=1)).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-45], dtype=np.float32)
    rec["ph"][n:] = [1.0, -2.0, 3.0]
    rec["q"][n:] = np.stack(np.meshgrid(odd, odd[:2], odd[:4], indexing="ij"), -1).reshape(-1, 3)
    got = _run(checker, tmp_path, "d2", rec.tobytes(), np.float64)
    want = AR.dist2(rec["q"], rec["ph"])
    assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)]) and np.isnan(got[np.isnan(want)]).all()
    assert not (want[n:] < np.inf).any()                                   # a q that is not finite, or overflows, is never below +inf
    assert (want[:n] < 50.0).all()


def _accept_reference(rec, ox, oz, rng, max_dist):
    thr2, Q = np.float64(np.float32(max_dist)) ** 2, AR.scale(rng)
    p, q = rec["p"], rec["q"]
    with np.errstate(invalid="ignore"):
        ok = rec["d2"] <= thr2
    oks, ints = zip(*[AR.quant(w, o, Q) for w, o in ((p[:, 0], ox), (p[:, 2], oz), (q[:, 0], ox), (q[:, 2], oz))])
    ok = ok & oks[0] & oks[1] & oks[2] & oks[3]
    t = np.zeros((len(rec), 5), np.int64)
    for k in range(4):
        t[ok, k] = ints[k][ok]
    t[ok, 4] = np.rint((q[ok, 1].astype(np.float64) - p[ok, 1].astype(np.float64)) * Q).astype(np.int64)
    return ok, t


@pytest.mark.parametrize("rng,max_dist", [(256.0, 2.0), (100.0, 0.7), (0.3, 0.3), (4096.0, 64.0)])
def test_acceptance_and_quantisation(checker, tmp_path, rng, max_dist):
    ox, oz = 31.5, -12.25
    n = 1 << 16
    rec = np.zeros(n, ACCEPT_IN)
    span = 2.6 * rng                                                        # a fifth of the coordinates lie out of range
    rec["p"] = np.stack([_scan(n, 11 << 22, span) + np.float32(ox), _scan(n, 12 << 22, span), _scan(n, 13 << 22, span) + np.float32(oz)], axis=1)
    rec["q"] = rec["p"] + np.stack([_scan(n, 14 << 22, 1.6 * max_dist), _scan(n, 15 << 22, 1.6 * max_dist), _scan(n, 16 << 22, 1.6 * max_dist)], axis=1)
    rec["d2"] = AR.dist2(rec["q"], rec["p"].astype(np.float64))            # (the identity estimate: p^ = p)
    # the edges.  |e| at and just below 2^18: (w - o) * Q with w - o = +-range exactly, and the float below it
    r32 = np.float32(rng)
    edge = np.zeros(16, ACCEPT_IN)
    at = [r32, np.nextafter(r32, np.float32(0)), -r32, np.nextafter(-r32, np.float32(0))]
    for i, w in enumerate(at):
        for j in range(4):                                                  # in each of the four quantised coordinates
            e = edge[4 * i + j]
            e["p"], e["q"] = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)
            (e["p"] if j < 2 else e["q"])[(0, 2)[j % 2]] = w
    thr2 = np.float64(np.float32(max_dist)) ** 2
    lim = np.zeros(4, ACCEPT_IN)                                            # d2 exactly max_dist^2, the doubles next to it, NaN
    lim["p"], lim["q"] = (ox, 2.0, oz), (ox, 2.0, oz)                       # (on the centre: in range whatever the range)
    lim["d2"] = [thr2, np.nextafter(thr2, np.inf), np.nextafter(thr2, 0.0), np.nan]
    none = np.zeros(2, ACCEPT_IN)                                           # no candidate at all: the best is still +inf
    none["d2"] = np.inf
    rec = np.concatenate([rec, lim, none])
    for (cx, cz), r in (((ox, oz), rec), ((0.0, 0.0), edge)):
        head = np.array([cx, cz], np.float64).tobytes() + np.array([rng, max_dist], np.float32).tobytes()
        got = _run(checker, tmp_path, "accept", head + r.tobytes(), ACCEPT_OUT)
        ok, t = _accept_reference(r, cx, cz, rng, max_dist)
        assert np.array_equal(got["ok"] != 0, ok) and np.array_equal(got["t"], t)
        assert np.abs(t).max() <= 1 << 18
    assert list(ok) == [False] * 4 + [True] * 4 + [False] * 4 + [True] * 4  # (the edges, about a centre of 0)
    ok, t = _accept_reference(rec, ox, oz, rng, max_dist)
    assert 0.05 < ok[:n].mean() < 0.95
    assert list(ok[n:n + 4]) == [True, False, True, False] and not ok[n + 4:].any()


def test_the_edges_of_the_range():
    """by the restatement alone: about a centre of 0 a coordinate of exactly +-range is out, the float below it is in"""
    for rng in (256.0, 100.0, 0.3, 4096.0):
        r32 = np.float32(rng)
        w = np.array([r32, np.nextafter(r32, np.float32(0)), -r32, np.nextafter(-r32, np.float32(0))], np.float32)
        ok, q = AR.quant(w, 0.0, AR.scale(rng))
        assert list(ok) == [False, True, False, True] and abs(int(q[1])) <= 1 << 18 and abs(int(q[3])) <= 1 << 18
