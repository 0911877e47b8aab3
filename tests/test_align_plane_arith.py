"""CPU tests of the point-to-plane refinement's arithmetic (3dscan_amd/csrc/sl3d_align_plane.h -- the header k_align_normals and
k_align_plane_pass compile, free of HIP) against the NumPy restatement of the rule (tests/align_plane_reference.py).

The header runs through tests/native/align_plane_check.cpp, built by g++ twice: plainly, and as the same stand-alone program with
-fsanitize=address,undefined (every check runs on both; the host program only, nothing that is loaded into Python).  The normal of a pixel
over hashed float bit patterns (every exponent: denormals, infinities, NaNs), over stencils of a scan's size and spacing and over the
specials -- a neighbour exactly at normal_edge and the float beyond, collinear and coincident neighbours, the smallest denormals; the
features, their quantisation and the verdict of a pair with |e| at and just below 2^18, d2 exactly max_dist^2 and the next double above,
NaN normals; the solve on the words of random integer features.  Everything bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import align_plane_reference as PR
import align_reference as AR

SRC = os.path.join(ROOT, "tests", "native", "align_plane_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
NORMAL_IN = np.dtype([("q", "<f4", 3), ("l", "<f4", 3), ("r", "<f4", 3), ("u", "<f4", 3), ("d", "<f4", 3), ("pad", "<f4")])
NORMAL_OUT = np.dtype([("n", "<f4", 3), ("ok", "<i4")])
ACCEPT_IN = np.dtype([("d2", "<f8"), ("p", "<f4", 3), ("q", "<f4", 3), ("n", "<f4", 3), ("pad", "<f4")])
ACCEPT_OUT = np.dtype([("f", "<i8", 5), ("verdict", "<i8")])


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_plane_" + request.param) / "align_plane_check")
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


def _unit(n, salt, span):
    """n hashed floats in [-span / 2, span / 2)"""
    return ((_hash32(np.arange(n) + salt).astype(np.float64) / 2.0**32 - 0.5) * span).astype(np.float32)


def _same_floats(a, b):
    return np.array_equal(a.view(np.uint32)[~np.isnan(b)], b.view(np.uint32)[~np.isnan(b)]) and np.isnan(a[np.isnan(b)]).all()


def _stencils(n, edge):
    """stencils of a scan: a centre, neighbours about 0.4 mm away along two tangents, noise that puts some of them beyond the edge"""
    rec = np.zeros(n, NORMAL_IN)
    q = np.stack([_unit(n, 1 << 22, 160.0), _unit(n, 2 << 22, 120.0), _unit(n, 3 << 22, 60.0) + 100], axis=1)
    t1 = np.stack([np.full(n, 0.4, np.float32), _unit(n, 4 << 22, 0.2), _unit(n, 5 << 22, 0.6)], axis=1)
    t2 = np.stack([_unit(n, 6 << 22, 0.2), np.full(n, 0.4, np.float32), _unit(n, 7 << 22, 0.6)], axis=1)
    noise = lambda k: np.stack([_unit(n, (8 + 3 * k) << 22, 1.6 * edge), _unit(n, (9 + 3 * k) << 22, 1.6 * edge), _unit(n, (10 + 3 * k) << 22, 1.6 * edge)], axis=1)
    rec["q"], rec["l"], rec["r"], rec["u"], rec["d"] = q, q - t1 + noise(0), q + t1 + noise(1), q - t2 + noise(2), q + t2 + noise(3)
    return rec


def _normal_specials(edge):
    f, e = np.float32, np.float32(edge)
    beyond = np.nextafter(e, f(np.inf))
    z = [0.0, 0.0, 0.0]
    rows = [
        dict(l=[-e, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),              # a neighbour exactly at the edge: kept
        dict(l=[-beyond, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),         # ... the float beyond: dropped
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, e, 0]),
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, beyond, 0]),
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[-0.125, 0, 0], d=[0.125, 0, 0]),         # collinear: a zero cross product
        dict(l=z, r=z, u=[0, -0.25, 0], d=[0, 0.25, 0]),                                  # left and right coincide: a = 0
        dict(l=z, r=z, u=z, d=z),
        dict(l=[-1e-45, 0, 0], r=[1e-45, 0, 0], u=[0, -1e-45, 0], d=[0, 1e-45, 0]),       # the smallest denormals still span a plane
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),           # n = (0, 0, 1) exactly
        dict(l=[0.25, 0, 0], r=[-0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),           # the orientation is the cross product's: (0, 0, -1)
        dict(l=[np.nan, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),
        dict(l=[-0.25, 0, 0], r=[0.25, np.inf, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, -np.inf], d=[0, 0.25, 0]),
        dict(l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 3e38]),
        dict(q=[np.nan, 0, 0], l=[-0.25, 0, 0], r=[0.25, 0, 0], u=[0, -0.25, 0], d=[0, 0.25, 0]),
    ]
    rec = np.zeros(len(rows), NORMAL_IN)
    for i, row in enumerate(rows):
        for key, val in row.items():
            rec[key][i] = f(val)
    return rec


@pytest.mark.parametrize("edge", [2.0, 0.7, 3e38])
def test_the_normal_of_a_pixel(checker, tmp_path, edge):
    n = 1 << 16
    bits = np.zeros(n, NORMAL_IN)
    raw = _hash32(np.arange(15 * n)).astype(np.uint32).view(np.float32).reshape(n, 15)            # every kind of float
    for k, key in enumerate(("q", "l", "r", "u", "d")):
        bits[key] = raw[:, 3 * k:3 * k + 3]
    scan = _stencils(n, min(edge, 4.0))
    mixed = scan[:4096].copy()                                                                  # one odd coordinate in a stencil of the scan
    mixed["r"][np.arange(4096), np.arange(4096) % 3] = raw[:4096, 0]
    rec = np.concatenate([bits, scan, mixed, _normal_specials(min(edge, 4.0))])
    head = np.array([edge, 0.0], np.float32).tobytes()
    got = _run(checker, tmp_path, "normal", head + rec.tobytes(), NORMAL_OUT)
    want = PR.normal_of(rec["q"], rec["l"], rec["r"], rec["u"], rec["d"], edge)
    assert got.shape == (len(rec),) and _same_floats(got["n"], want)
    has = ~np.isnan(want[:, 0])
    assert np.array_equal(got["ok"] != 0, has) and np.array_equal(np.isnan(want).all(axis=1), ~has)     # three NaNs or none
    length = np.sqrt((want[has].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() < 1e-6                                                    # a float unit vector
    s = slice(n, 2 * n)
    assert (0.05 < has[s].mean() < 0.95) if edge < 3.0 else has[s].all()                        # both outcomes on the scan's stencils
    sp = list(has[-15:])
    if edge < 3.0:
        assert sp == [True, False, True, False, False, False, False, True, True, True, False, False, False, False, False]
        assert np.array_equal(want[-7], np.float32([0, 0, 1])) and np.array_equal(want[-6], np.float32([0, 0, -1]))


def _accept_reference(rec, ox, oz, rng, max_dist):
    thr2 = np.float64(np.float32(max_dist)) ** 2
    with np.errstate(invalid="ignore"):
        near = rec["d2"] <= thr2
    has = near & ~np.isnan(rec["n"][:, 0])
    ok, f = PR.features(rec["p"], rec["q"], np.where(has[:, None], rec["n"], np.float32(0.0)), ox, oz, PR.scale(rng))
    verdict = np.where(near & ~has, 2, np.where(has & ok, 1, 0))
    f[verdict != 1] = 0
    return verdict, f


@pytest.mark.parametrize("rng,max_dist", [(256.0, 2.0), (100.0, 0.7), (0.25, 0.25), (4096.0, 64.0)])
def test_features_quantisation_and_verdict(checker, tmp_path, rng, max_dist):
    ox, oz = 31.5, -12.25
    n = 1 << 16
    rec = np.zeros(n, ACCEPT_IN)
    span = 7.0 * rng                                                        # some features lie out of range: |A| up to 3.5 * sqrt(2) range
    rec["p"] = np.stack([_unit(n, 11 << 22, span) + np.float32(ox), _unit(n, 12 << 22, span), _unit(n, 13 << 22, span) + np.float32(oz)], axis=1)
    rec["q"] = rec["p"] + np.stack([_unit(n, 14 << 22, 1.6 * max_dist), _unit(n, 15 << 22, 1.6 * max_dist), _unit(n, 16 << 22, 1.6 * max_dist)], axis=1)
    rec["d2"] = AR.dist2(rec["q"], rec["p"].astype(np.float64))            # (the identity estimate: p^ = p)
    v = np.stack([_unit(n, 17 << 22, 2.0), _unit(n, 18 << 22, 2.0), _unit(n, 19 << 22, 2.0)], axis=1).astype(np.float64)
    rec["n"] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    rec["n"][::7] = np.nan                                                  # one best candidate in seven has no normal
    thr2 = np.float64(np.float32(max_dist)) ** 2
    lim = np.zeros(5, ACCEPT_IN)                                            # d2 exactly max_dist^2, the doubles next to it, NaN, no candidate
    lim["p"], lim["q"], lim["n"] = (ox, 2.0, oz), (ox, 2.0, oz), (0.0, 0.0, 1.0)
    lim["d2"] = [thr2, np.nextafter(thr2, np.inf), np.nextafter(thr2, 0.0), np.nan, np.inf]
    rec = np.concatenate([rec, lim])
    head = np.array([ox, oz], np.float64).tobytes() + np.array([rng, max_dist], np.float32).tobytes()
    got = _run(checker, tmp_path, "accept", head + rec.tobytes(), ACCEPT_OUT)
    verdict, f = _accept_reference(rec, ox, oz, rng, max_dist)
    assert np.array_equal(got["verdict"], verdict) and np.array_equal(got["f"], f)
    assert np.abs(f).max() < 1 << 18 and all((verdict[:n] == k).mean() > 0.02 for k in (0, 1, 2))
    assert list(verdict[n:]) == [1, 0, 1, 0, 0]
    # the edges about a centre of 0: A = p.x under n = (1, 0, 0), so |e| is 2^18 at p.x = 4 range exactly (the ranges are exact in float)
    r32 = np.float32(4.0 * rng)
    edge = np.zeros(8, ACCEPT_IN)
    edge["n"] = (1.0, 0.0, 0.0)
    for i, w in enumerate([r32, np.nextafter(r32, np.float32(0)), -r32, np.nextafter(-r32, np.float32(0))]):
        edge["p"][i, 0] = w                                                 # A at the limit, below it
        edge["n"][4 + i] = (0.0, 0.0, 1.0)
        edge["p"][4 + i, 0] = -w                                            # ... and B = n.z * p'x
    head = np.array([0.0, 0.0], np.float64).tobytes() + np.array([rng, max_dist], np.float32).tobytes()
    got = _run(checker, tmp_path, "accept", head + edge.tobytes(), ACCEPT_OUT)
    verdict, f = _accept_reference(edge, 0.0, 0.0, rng, max_dist)
    assert np.array_equal(got["verdict"], verdict) and np.array_equal(got["f"], f)
    if rng != 100.0:                                                        # (2^16 / 100 is not exact: the restatement alone decides there)
        assert list(verdict) == [0, 1, 0, 1] * 2
    assert (f[:, 2] == np.where(verdict[:] == 1, np.where(np.arange(8) < 4, 65536, 0), 0)).all()      # n.x = 1 is 2^16


def test_the_solve_on_random_integer_features(checker, tmp_path):
    """words of random small features through the stand-alone solve and the restatement: bit for bit (one libm, the same operations)"""
    rng = np.random.default_rng(5)
    for trial in range(6):
        m = 400
        th = rng.uniform(0, 2 * np.pi, m)
        el = rng.uniform(-0.6, 0.6, m)
        nrm = np.stack([np.cos(el) * np.cos(th), np.sin(el), np.cos(el) * np.sin(th)], axis=1)
        f = np.stack([rng.integers(-90000, 90000, m), rng.integers(-90000, 90000, m), np.rint(nrm[:, 0] * 65536).astype(np.int64),
                      np.rint(nrm[:, 2] * 65536).astype(np.int64), rng.integers(-9000, 9000, m)], axis=1)
        words = []
        for part in np.array_split(np.arange(m), 3):
            w = [len(part)] + [int((f[part, i] * f[part, j]).sum()) for i in range(5) for j in range(i, 5)] + [len(part) + 5, 2]
            words.append(w)
        words = np.array(words, dtype=np.int64)
        est = AR.estimate(10.0 + 25.0 * trial, 3.0 - trial, -2.0 + 0.5 * trial)
        ox, oz, r = 2.5, -1.5, 128.0
        head = np.array([ox, oz, *est], np.float64).tobytes() + np.array([r], np.float32).tobytes() + np.array([3], np.int32).tobytes()
        got = _run(checker, tmp_path, "solve", head + words.tobytes(), np.float64)
        want_est, stats = PR.solve(words, r, ox, oz, est)
        assert not stats["degenerate"] and stats["n"] == m
        assert np.array_equal(got[:4], want_est) and got[4] == m and got[5] == stats["rms_xz"] and np.isnan(got[6]) and got[7] == 0.0
