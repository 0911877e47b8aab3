"""CPU test of the vertex-normal arithmetic (3dscan_amd/csrc/sl3d_mesh.h: mesh_face_vector, mesh_quad_sums, mesh_normal_from_sum -- the
header k_mesh_normals compiles, free of HIP): whole frames walked through the header with the kernel's chunk / quad indexing
(tests/native/mesh_normals_check.cpp, chunk width a parameter so that the seams fall everywhere) and compared bit for bit with the NumPy
restatement of the definition (tests/mesh_normals_reference.py) over the pinned mesh restatement (tests/mesh_reference.py).  The
restatement itself is pinned to closed-form normals, counts and hashes that were not derived from the code under test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mesh_normals_reference import normals_sha256, np_normals
from mesh_reference import np_mesh

SRC = os.path.join(ROOT, "tests", "native", "mesh_normals_check.cpp")
INF = float("inf")

# the golden crops (points cast to float32, the fixture's own valid map): vertices, vertices in no face at max_edge 0.25 / 1.0 / +inf (counted
# from the pinned np_mesh), and the first 16 hex digits of the sha256 of the float32 LE normals at 1.0 (computed with the restatement)
GOLDEN = {
    "real_edge": dict(vertices=5234, in_no_face={0.25: 2511, 1.0: 1651, INF: 0}, sha="9f831009437a9f04"),
    "real_inside": dict(vertices=8189, in_no_face={0.25: 589, 1.0: 398, INF: 0}, sha="0e1e58a97bd3c1dd"),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_normals") / "mesh_normals_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", exe])
    return exe


def _fmt(max_edge):
    return "inf" if np.isinf(max_edge) else float(np.float32(max_edge)).hex()


def run_checker(exe, tmp_path, xyz, valid, max_edge, chunk):
    H, W = valid.shape
    fx, fv, on = (str(tmp_path / n) for n in ("xyz.bin", "valid.bin", "normals.bin"))
    np.ascontiguousarray(xyz, dtype=np.float32).tofile(fx)
    np.ascontiguousarray(valid, dtype=np.uint8).tofile(fv)
    subprocess.check_call([exe, fx, fv, str(H), str(W), _fmt(max_edge), str(chunk), on], timeout=600)
    return np.fromfile(on, dtype=np.float32).reshape(-1, 3)


def restated(xyz, valid, max_edge, stats=None):
    verts, faces = np_mesh(xyz, valid, max_edge)
    return np_normals(verts, faces, stats)


def assert_same_normals(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape, tag
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag      # bit for bit: +0 is not -0


def _golden_frame(name):
    g = load_golden(name)
    return g["points"].astype(np.float32), g["valid"]


# ---- pins of the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx,sy,g", [(1, 1, (2, 3, -1)), (3, 5, (10, 9, -15))])
def test_restatement_on_a_plane_is_the_closed_form(sx, sy, g):
    """Points (sx*col, sy*row, 2*col + 3*row): every face vector is an exact integer multiple of g, so is every sum, and the normal of
    every vertex with a face is (float)(g / sqrt(g.g)) whatever the number of its faces; a vertex in no face gets +0."""
    H, W = 23, 41
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xyz = np.stack([sx * cc, sy * rr, 2 * cc + 3 * rr], axis=-1).astype(np.float32)
    gg = np.array(g, np.float64)
    want = (gg / np.sqrt((gg * gg).sum())).astype(np.float32)
    rng = np.random.default_rng(1)
    for valid in (np.ones((H, W), np.uint8), (rng.random((H, W)) < 0.8).astype(np.uint8)):
        st = {}
        n = restated(xyz, valid, INF, st)
        has = st["faces_per_vertex"] > 0
        assert has.sum() > 500 and len(np.unique(st["faces_per_vertex"][has])) >= 4
        assert np.array_equal(n[has].view(np.uint32), np.broadcast_to(want, n[has].shape).view(np.uint32))
        assert (n[~has].view(np.uint32) == 0).all()
        if not valid.all():
            assert (~has).sum() > 0


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_restatement_has_the_pinned_counts_and_hashes(name):
    xyz, valid = _golden_frame(name)
    G = GOLDEN[name]
    for max_edge, n_zero in G["in_no_face"].items():
        verts, faces = np_mesh(xyz, valid, max_edge)
        st = {}
        n = np_normals(verts, faces, st)
        assert len(n) == G["vertices"]
        zero = (n.view(np.uint32) == 0).all(axis=1)
        in_no_face = np.ones(len(verts), bool)
        in_no_face[faces.ravel()] = False
        assert np.array_equal(zero, in_no_face) and int(zero.sum()) == n_zero, (name, max_edge)
        assert st["max_faces_per_vertex"] == 8
        length = np.linalg.norm(n[~zero].astype(np.float64), axis=1)
        print(f"{name} max_edge {max_edge}: {n_zero} zero normals, | |n| - 1 | <= {np.abs(length - 1.0).max():.3g}")
        assert np.abs(length - 1.0).max() <= 2e-7
        if max_edge == 1.0:
            assert normals_sha256(n)[:16] == G["sha"]


# ---- the header against the restatement, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN))
@pytest.mark.parametrize("chunk", [64, 1024])
def test_header_equals_restatement_on_the_real_crops(checker, tmp_path, name, chunk):
    xyz, valid = _golden_frame(name)
    for max_edge in (0.25, 1.0, INF):
        assert_same_normals(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), restated(xyz, valid, max_edge), (name, max_edge, chunk))


SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (9, 3), (9, 4), (9, 5), (5, 1023), (5, 1024), (5, 1025)]
SELECTIONS = [0.0, 0.05, 0.5, 0.95, 1.0]


def _mask(rng, H, W, p):
    if p <= 0.0:
        return np.zeros((H, W), np.uint8)
    if p >= 1.0:
        return np.ones((H, W), np.uint8)
    return (rng.random((H, W)) < p).astype(np.uint8)


def test_integer_points_exact_ties_and_threshold_hits(checker, tmp_path):
    """Small-integer coordinates: exact diagonal ties and edges exactly at the threshold decide which faces a vertex sums, and sums that
    cancel to exactly zero (a zero normal at a vertex WITH faces) occur."""
    rng = np.random.default_rng(7)
    cancelled = nonzero = 0
    for H, W in SHAPES:
        xyz = rng.integers(-2, 3, size=(H, W, 3)).astype(np.float32)
        for p in SELECTIONS:
            valid = _mask(rng, H, W, p)
            for max_edge in (2.0, 3.0, INF):
                st = {}
                want = restated(xyz, valid, max_edge, st)
                zero = (want == 0).all(axis=1)
                cancelled += int((zero & (st["faces_per_vertex"] > 0)).sum())
                nonzero += int((~zero).sum())
                for chunk in (64, 1024):
                    assert_same_normals(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), want, (H, W, p, max_edge, chunk))
    assert cancelled > 10 and nonzero > 1000


def test_float_noise(checker, tmp_path):
    rng = np.random.default_rng(11)
    for H, W in SHAPES:
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        xyz = np.stack([0.2 * cc, 0.2 * rr, 500.0 + 0.0 * cc], axis=-1) + rng.normal(0.0, 0.15, size=(H, W, 3))
        xyz = xyz.astype(np.float32)
        for p in SELECTIONS:
            valid = _mask(rng, H, W, p)
            for max_edge in (0.35, INF):
                want = restated(xyz, valid, max_edge)
                if p == 1.0 and H > 1 and W > 4:
                    assert (want != 0).any()
                for chunk in (64, 1024):
                    assert_same_normals(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), want, (H, W, p, max_edge, chunk))


def test_nan_and_inf_coordinates_under_valid_pixels(checker, tmp_path):
    """Every vertex of a face with a non-finite coordinate gets the zero normal (its sum is NaN or infinite); a vertex two pixels or more
    from every such point has the normal of the frame without them."""
    rng = np.random.default_rng(3)
    H, W = 12, 70
    xyz = rng.integers(-1, 2, size=(H, W, 3)).astype(np.float32)
    valid = np.ones((H, W), np.uint8)
    bad = [(3, 5), (7, 64), (9, 20)]
    xyz[3, 5, 1] = np.nan
    xyz[7, 64, 0] = np.inf                                  # (next to a chunk seam at chunk width 64)
    xyz[9, 20] = (np.nan, np.inf, -np.inf)
    clean = np.nan_to_num(xyz, nan=0.0, posinf=0.0, neginf=0.0)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    far = np.ones((H, W), bool)
    for r, c in bad:
        far &= np.maximum(np.abs(rr - r), np.abs(cc - c)) >= 2
    for max_edge in (1.5, INF):
        verts, faces = np_mesh(xyz, valid, max_edge)
        want = np_normals(verts, faces)
        touched = np.zeros(H * W, bool)
        touched[faces[~np.isfinite(verts[faces]).all(axis=(1, 2))].ravel()] = True
        assert touched.any() == (max_edge == INF)           # an infinite edge is short only at +inf, a NaN edge never
        assert (want[touched].view(np.uint32) == 0).all()
        ref = restated(clean, valid, max_edge)
        assert np.array_equal(want[far.ravel()].view(np.uint32), ref[far.ravel()].view(np.uint32)) and (ref[far.ravel()] != 0).any()
        assert np.isfinite(want).all()
        for chunk in (64, 1024):
            assert_same_normals(run_checker(checker, tmp_path, xyz, valid, max_edge, chunk), want, (max_edge, chunk))
