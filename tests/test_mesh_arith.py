"""CPU test of the mesh arithmetic (3dscan_amd/csrc/sl3d_mesh.h -- the header k_mesh_count / k_mesh_emit compile, free of HIP): whole
frames walked through the header with the kernels' chunk / lane indexing (tests/native/mesh_check.cpp, chunk width a parameter so that
the seams fall everywhere) and compared bit for bit with the NumPy restatement of the definition (tests/mesh_reference.py).  The
restatement itself is pinned to counts and hashes of the real crops that were not derived from the code under test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mesh_reference import check_faces, faces_sha256, np_mesh

SRC = os.path.join(ROOT, "tests", "native", "mesh_check.cpp")
INF = float("inf")

# the golden crops (points cast to float32, the fixture's own valid map): vertices, faces at max_edge 0.25 / 1.0 / +inf, cells that take the
# diagonal a-e / b-d, cells with three valid corners, and the first 16 hex digits of the sha256 of the int32 LE face array at 1.0
GOLDEN = {
    "real_edge": dict(vertices=5234, faces={0.25: 4449, 1.0: 5303, INF: 10006}, diag_ae=2210, diag_bd=2737, three=112, sha="0d55d3880be22811"),
    "real_inside": dict(vertices=8189, faces={0.25: 12962, 1.0: 14309, INF: 15990}, sha="6e152aa5123ca242"),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh") / "mesh_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", exe])
    return exe


def _fmt(max_edge):
    return "inf" if np.isinf(max_edge) else float(np.float32(max_edge)).hex()


def run_checker(exe, tmp_path, xyz, valid, max_edge, chunk):
    H, W = valid.shape
    fx, fv, ov, of = (str(tmp_path / n) for n in ("xyz.bin", "valid.bin", "verts.bin", "faces.bin"))
    np.ascontiguousarray(xyz, dtype=np.float32).tofile(fx)
    np.ascontiguousarray(valid, dtype=np.uint8).tofile(fv)
    subprocess.check_call([exe, fx, fv, str(H), str(W), _fmt(max_edge), str(chunk), ov, of], timeout=600)
    return np.fromfile(ov, dtype=np.float32).reshape(-1, 3), np.fromfile(of, dtype=np.int32).reshape(-1, 3)


def assert_same_mesh(got, want, tag):
    (gv, gf), (wv, wf) = got, want
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), tag
    assert gf.shape == wf.shape and np.array_equal(gf, wf), tag


def _golden_frame(name):
    g = load_golden(name)
    return g["points"].astype(np.float32), g["valid"]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_restatement_has_the_pinned_counts_and_hashes(name):
    xyz, valid = _golden_frame(name)
    G = GOLDEN[name]
    for max_edge, n_faces in G["faces"].items():
        st = {}
        verts, faces = np_mesh(xyz, valid, max_edge, st)
        assert len(verts) == G["vertices"] and len(faces) == n_faces, (name, max_edge)
        check_faces(faces, valid, len(verts))
        assert st["diag_ae"] > 0 and st["diag_bd"] > 0 and st["three"] > 0
        if "diag_ae" in G:
            assert (st["diag_ae"], st["diag_bd"], st["three"]) == (G["diag_ae"], G["diag_bd"], G["three"])
        if max_edge == 1.0:
            assert faces_sha256(faces)[:16] == G["sha"]
            assert 0 < st["rejected"] < st["candidates"]
    # all four 3-corner shapes occur
    v = valid == 1
    va, vb, vd, ve = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    three = (va.astype(int) + vb + vd + ve) == 3
    assert all((three & ~m).any() for m in (va, vb, vd, ve))


@pytest.mark.parametrize("name", sorted(GOLDEN))
@pytest.mark.parametrize("chunk", [64, 1024])
def test_header_equals_restatement_on_the_real_crops(checker, tmp_path, name, chunk):
    xyz, valid = _golden_frame(name)
    for max_edge in (0.25, 1.0, INF):
        assert_same_mesh(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), np_mesh(xyz, valid, max_edge), (name, max_edge, chunk))


SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (9, 3), (9, 4), (9, 5), (5, 1023), (5, 1024), (5, 1025)]
SELECTIONS = [0.0, 0.05, 0.5, 0.95, 1.0]


def _mask(rng, H, W, p):
    if p <= 0.0:
        return np.zeros((H, W), np.uint8)
    if p >= 1.0:
        return np.ones((H, W), np.uint8)
    return (rng.random((H, W)) < p).astype(np.uint8)


def test_integer_points_exact_ties_and_threshold_hits(checker, tmp_path):
    """Small-integer coordinates: len2 is an exact small integer, so exact diagonal ties (len2(a,e) == len2(b,d)) and edges with
    len2 == max_edge^2 exactly both occur -- and are asserted to."""
    rng = np.random.default_rng(7)
    ties = hits = 0
    for H, W in SHAPES:
        xyz = rng.integers(-2, 3, size=(H, W, 3)).astype(np.float32)
        for p in SELECTIONS:
            valid = _mask(rng, H, W, p)
            for max_edge in (2.0, 3.0, INF):             # thr2 = 4, 9: attained by integer len2
                st = {}
                want = np_mesh(xyz, valid, max_edge, st)
                ties += st["ties"]
                hits += st["at_threshold"]
                check_faces(want[1], valid, len(want[0]))
                for chunk in (64, 1024):
                    assert_same_mesh(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), want, (H, W, p, max_edge, chunk))
    assert ties > 100 and hits > 100


def test_float_noise(checker, tmp_path):
    rng = np.random.default_rng(11)
    for H, W in SHAPES:
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        xyz = np.stack([0.2 * cc, 0.2 * rr, 500.0 + 0.0 * cc], axis=-1) + rng.normal(0.0, 0.15, size=(H, W, 3))
        xyz = xyz.astype(np.float32)
        for p in SELECTIONS:
            valid = _mask(rng, H, W, p)
            for max_edge in (0.35, INF):
                st = {}
                want = np_mesh(xyz, valid, max_edge, st)
                check_faces(want[1], valid, len(want[0]))
                if p == 1.0 and H > 1 and W > 4 and max_edge < INF:
                    assert 0 < st["rejected"] < st["candidates"]
                for chunk in (64, 1024):
                    assert_same_mesh(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), want, (H, W, p, max_edge, chunk))


def test_nan_and_inf_coordinates_under_valid_pixels(checker, tmp_path):
    """A NaN len2 is not short and never takes the diagonal a-e; an infinite one is short only at max_edge = +inf."""
    rng = np.random.default_rng(3)
    H, W = 12, 70
    xyz = rng.integers(-1, 2, size=(H, W, 3)).astype(np.float32)
    valid = np.ones((H, W), np.uint8)
    xyz[3, 5, 1] = np.nan
    xyz[7, 64, 0] = np.inf                                  # (next to a chunk seam at chunk width 64)
    xyz[9, 20] = (np.nan, np.inf, -np.inf)
    for max_edge in (1.5, INF):
        want = np_mesh(xyz, valid, max_edge)
        full = np_mesh(np.nan_to_num(xyz, nan=0.0, posinf=0.0, neginf=0.0), valid, max_edge)
        assert len(want[1]) < len(full[1])
        nan_id = 3 * W + 5
        assert not (want[1] == nan_id).any()               # every edge at a NaN point has a NaN length
        inf_id = 7 * W + 64
        assert (want[1] == inf_id).any() == (max_edge == INF)
        check_faces(want[1], valid, len(want[0]))
        for chunk in (64, 1024):
            got = run_checker(checker, tmp_path, xyz, valid, max_edge, chunk)
            assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (max_edge, chunk)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
