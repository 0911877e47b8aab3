"""CPU tests of the TSDF volume's arithmetic (3dscan_amd/csrc/sl3d_tsdf.h -- the header k_tsdf_integrate, k_tsdf_count and k_tsdf_scatter
compile, free of HIP) against the NumPy restatement of the rule (tests/tsdf_reference.py).

The header runs through tests/native/tsdf_check.cpp, built by g++ twice: plainly, and as the same stand-alone program with
-fsanitize=address,undefined (every check runs on both; nothing is loaded into python).  The program fuses views into a volume and
extracts its surface the way the kernels walk the voxels; sum, weight, the counts, xyz, normals and edge are compared word for word, for
the volumes and views of tests/tsdf_cases.py: the five shapes at 1, 2 and 5 views and first_step 0 and 3, the one-voxel special cases of
an integration, and the crafted volumes of an extraction.  The quantisation alone runs over hashed inputs and its edges."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tsdf_cases as TC
import tsdf_reference as TR

SRC = os.path.join(ROOT, "tests", "native", "tsdf_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
HEAD = np.dtype([("cam", "<f8", 26), ("est", "<f8", 4), ("origin", "<f4", 3), ("voxel", "<f4"), ("trunc", "<f4"), ("dims", "<i4", 3), ("W", "<i4"),
                 ("H", "<i4"), ("col0", "<i4"), ("row0", "<i4"), ("V", "<i4"), ("first_step", "<i4"), ("min_weight", "<i8")])
QUANT_IN = np.dtype([("z", "<f8", 4), ("a", "<f8"), ("b", "<f8"), ("zc", "<f8"), ("T", "<f8")])
QUANT_OUT = np.dtype([("ok", "<i4"), ("q", "<i4")])


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tsdf_" + request.param) / "tsdf_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *FLAGS[request.param], SRC, "-o", exe])
    return exe


def _fuse(exe, tmp_path, cam, est, vol, points, valid, first_step=0, min_weight=1):
    """the native program's (words, sum, weight, xyz, normals, edge)"""
    assert HEAD.itemsize == 304
    V, H, W = valid.shape
    h = np.zeros(1, HEAD)
    h["cam"], h["est"], h["origin"], h["voxel"], h["trunc"], h["dims"] = cam, est, vol["origin"], vol["voxel"], vol["trunc"], vol["dims"]
    h["W"], h["H"], h["col0"], h["row0"], h["V"], h["first_step"], h["min_weight"] = W, H, TC.ORIGIN[0], TC.ORIGIN[1], V, first_step, min_weight
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(h.tobytes() + np.ascontiguousarray(points, np.float32).tobytes() + np.ascontiguousarray(valid, np.uint8).tobytes())
    subprocess.check_call([exe, "fuse", src, out], timeout=600)
    raw = open(out, "rb").read()
    words = np.frombuffer(raw, "<i8", 5)
    n, m = int(words[2]), int(words[4])
    at = [40]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype, count, at[0])
        at[0] += a.nbytes
        return a
    got = (words, take("<i4", n), take("<u4", n), take("<f4", 3 * m).reshape(m, 3), take("<f4", 3 * m).reshape(m, 3), take("<i4", m))
    assert at[0] == len(raw)
    return got


def _same(got, want):
    """bit for bit, NaNs included"""
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _check(exe, tmp_path, cam, est, vol, points, valid, first_step=0, min_weight=1):
    words, s, w, xyz, nrm, edge = _fuse(exe, tmp_path, cam, est, vol, points, valid, first_step, min_weight)
    rs, rw = TR.new_volume(vol)
    taken, occupied = TR.integrate(rs, rw, vol, points, valid, cam, *TC.ORIGIN, est, first_step)
    assert np.array_equal(s, rs) and np.array_equal(w, rw) and (int(words[0]), int(words[1])) == (taken, occupied)
    rxyz, rnrm, redge, counts = TR.extract(rs, rw, vol, min_weight)
    assert [int(words[2]), int(words[3]), int(words[4])] == counts
    assert np.array_equal(edge, redge) and _same(xyz, rxyz) and _same(nrm, rnrm)
    return rs, rw, rxyz, rnrm, redge


@pytest.fixture(scope="module")
def rig_cam():
    return TC.camera(TC.rig_calibration())


@pytest.fixture(scope="module")
def exact_cam():
    return TC.camera(TC.exact_calibration())


@pytest.mark.parametrize("dims", TC.SHAPES, ids=["x".join(map(str, d)) for d in TC.SHAPES])
def test_shapes_views_and_steps(checker, tmp_path, rig_cam, dims):
    points, valid, est, _, vol = TC.shape_case(rig_cam, dims, 5, 7 * dims[0] + dims[2])
    est = est + np.array([0.0, 0.0, 0.05, -0.03])
    for V, first_step, mw in ((1, 0, 1), (2, 0, 1), (5, 0, 2), (2, 3, 1)):
        rs, rw, xyz, nrm, edge = _check(checker, tmp_path, rig_cam, est, vol, points[:V], valid[:V], first_step, mw)
        if np.prod(dims) >= 900 and V == 5:                                  # by the restatement alone: the case exercises both outcomes
            assert 0 < (rw > 0).sum() and (rw < V).any() and (rw == V).any() and len(edge) > 0
            assert np.isfinite(nrm).all(axis=1).any()


def test_the_special_cases_of_an_integration(checker, tmp_path, exact_cam):
    xyz, valid, _, cases = TC.special_cases()
    assert np.array_equal(exact_cam[0:9], np.eye(3).ravel()) and not exact_cam[9:12].any()
    for name, vol, weight, q in cases:
        rs, rw, *_ = _check(checker, tmp_path, exact_cam, TC.IDENTITY, vol, xyz[None], valid[None])
        assert int(rw[0]) == weight, name                                   # what the case is for, by the restatement alone
        if q is not None:
            assert int(rs[0]) == q, name


def test_the_crafted_volumes_of_an_extraction(checker, tmp_path, exact_cam):
    for name, (xyz, valid, vol), mw in _extraction_cases():
        _check(checker, tmp_path, exact_cam, TC.IDENTITY, vol, xyz[None], valid[None], 0, mw)


def _extraction_cases():
    """(name, (xyz, valid, vol), min_weight): tests/test_gpu_tsdf_extract.py runs the same on the device"""
    h, N = 0.5, None
    return [
        ("crossings along x and y, one-sided gradients at the border", TC.slab_case([[h, h, -h, -h], [h, -h, -h, -h], [-h, -h, -h, h]]), 1),
        ("a zero gradient: NaN normal", TC.slab_case([[-h, h, -h, h]]), 1),
        ("f0 == 0 and f1 == 0 exactly", TC.slab_case([[0.0, -h, 0.0, h], [-h, 0.0, h, 0.0]]), 1),
        ("unknown voxels between known ones", TC.slab_case([[h, N, -h, h], [-h, -h, N, -h], [h, -h, -h, N]]), 1),
        ("empty: one sign", TC.slab_case([[h, 0.25, 1.0], [0.125, h, 1.0]]), 1),
        ("empty: nothing known at min_weight 2", TC.slab_case([[h, -h], [-h, h]]), 2),
        ("a crossing along z", TC.column_case(9, 64.25), 1),
        ("one voxel", TC.column_case(1, 60.25), 1),
    ]


def test_what_the_extraction_cases_are_for(exact_cam):
    """by the restatement alone"""
    out = {}
    for name, (xyz, valid, vol), mw in _extraction_cases():
        s, w = TR.new_volume(vol)
        TR.integrate(s, w, vol, xyz[None], valid[None], exact_cam, *TC.ORIGIN, TC.IDENTITY)
        out[name] = (s, w) + TR.extract(s, w, vol, mw)
    s, w, xyz, nrm, edge, counts = out["crossings along x and y, one-sided gradients at the border"]
    assert list(s[:4]) == [16384, 16384, -16384, -16384] and (w == 1).all()   # (0.5 * 32767 is a tie: to the even side)
    assert set(edge % 3) == {0, 1} and counts == [12, 12, len(edge)] and np.isfinite(nrm).all()
    assert (nrm[:, 2] == 0).all()                                            # no neighbour along z: that component is 0.0
    s, w, xyz, nrm, edge, counts = out["a zero gradient: NaN normal"]
    assert list(edge) == [0, 3, 6] and np.isnan(nrm[1]).all() and np.isfinite(nrm[0]).all() and np.isfinite(nrm[2]).all()
    s, w, xyz, nrm, edge, counts = out["f0 == 0 and f1 == 0 exactly"]
    vol = _extraction_cases()[2][1][2]
    X, _ = TR.centres(vol)
    assert 0 in edge and np.array_equal(xyz[list(edge).index(0)], X[0].astype(np.float32))      # f0 == 0, f1 < 0: t = 0, the centre itself
    assert 3 in edge and np.array_equal(xyz[list(edge).index(3)], X[2].astype(np.float32))      # f0 < 0, f1 == 0: t = 1, the neighbour's centre
    assert 6 not in edge                                                     # f0 == 0, f1 > 0: no crossing
    s, w, xyz, nrm, edge, counts = out["unknown voxels between known ones"]
    assert counts[1] == 9 and len(edge) > 0 and 0 not in edge                # (voxel 0's + neighbour along x is unknown)
    assert out["empty: one sign"][5] == [6, 6, 0] and out["empty: nothing known at min_weight 2"][5] == [4, 0, 0]
    s, w, xyz, nrm, edge, counts = out["a crossing along z"]
    assert list(edge % 3) == [2] and counts == [9, 7, 1]                     # the voxels more than T behind the surface stay unknown
    assert out["one voxel"][5] == [1, 1, 0]


def _hash32(t):
    t = t.astype(np.uint64)
    m = np.uint64(0xffffffff)
    t ^= t >> np.uint64(16)
    t = (t * np.uint64(0x7feb352d)) & m
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x846ca68b)) & m
    t ^= t >> np.uint64(16)
    return t


def test_quantisation(checker, tmp_path):
    n = 1 << 16
    u = lambda salt: _hash32(np.arange(n) + salt).astype(np.float64) / 2.0**32
    rec = np.zeros(n + 8, QUANT_IN)
    rec["T"][:n] = np.float32(3.0)
    rec["zc"][:n] = 100.0 + 8.0 * (u(1 << 20) - 0.5)
    rec["z"][:n] = rec["zc"][:n, None] + 14.0 * (u(2 << 20)[:, None] - 0.5) + 4.5 * np.stack([u((3 + k) << 20) for k in range(4)], axis=1)
    rec["a"][:n], rec["b"][:n] = u(7 << 20), u(8 << 20)
    odd = rec[n:]
    odd["T"], odd["zc"], odd["a"], odd["b"] = 2.0, 64.0, 0.5, 0.5
    odd["z"] = [[65.0] * 4, [np.nan, 65, 65, 65], [np.inf] * 4, [-np.inf, 65, 65, 65], [62.0] * 4, [61.999] * 4, [66.0] * 4, [1e300] * 4]
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(rec.tobytes())
    subprocess.check_call([checker, "quant", src, out], timeout=600)
    got = np.fromfile(out, QUANT_OUT)
    ok, q = TR.quant(rec["z"], rec["a"], rec["b"], rec["zc"], rec["T"][0])
    ok2, q2 = TR.quant(rec["z"][n:], rec["a"][n:], rec["b"][n:], rec["zc"][n:], 2.0)
    ok[n:], q[n:] = ok2, q2
    assert np.array_equal(got["ok"] != 0, ok) and np.array_equal(got["q"], q)
    assert 0.2 < ok[:n].mean() < 0.8 and (np.abs(q) <= 32767).all() and (q[:n] == 32767).any() and (q[:n] < -30000).any()
    assert list(ok[n:]) == [True, False, False, False, True, False, True, True] and list(q[n:][ok[n:]]) == [16384, -32767, 32767, 32767]
