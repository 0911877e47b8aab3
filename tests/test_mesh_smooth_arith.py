"""CPU test of the smoothing arithmetic (3dscan_amd/csrc/sl3d_mesh_smooth.h: smooth_ring, smooth_step, smooth_quad_sums -- the header the
k_smooth_* kernels compile, free of HIP): whole frames walked through the header with the kernels' chunk / quad indexing
(tests/native/mesh_smooth_check.cpp, chunk width a parameter so that the seams fall everywhere) and compared bit for bit with the NumPy
restatement of the definition on (vertices, faces) alone (tests/mesh_smooth_reference.py) over the pinned mesh restatement
(tests/mesh_reference.py).  The restatement itself is pinned to an affine plane, a hand-computed example, and counts of the golden crops
that were computed in advance by a separate restatement -- none of them derived from the code under test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mesh_normals_reference import np_normals
from mesh_reference import np_mesh
from mesh_smooth_reference import FIX_BOUNDARY, NORMALS, np_smooth, np_topology, positions_sha256

SRC = os.path.join(ROOT, "tests", "native", "mesh_smooth_check.cpp")
INF = float("inf")
LAM, MU = np.float32(0.5), np.float32(-0.53)
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]

# the golden crops (points cast to float32, the fixture's own valid map) per max_edge: faces, vertices without a neighbour, boundary
# vertices; and the first 16 hex digits of the sha256 of the float32 LE positions after 10 iterations (0.5, -0.53) at max_edge 1.0, without
# and with SL3D_SMOOTH_FIX_BOUNDARY (computed with the restatement)
GOLDEN = {
    "real_edge": dict(vertices=5234, cases={0.25: (4449, 2511, 898), 1.0: (5303, 1651, 1503), INF: (10006, 0, 481)},
                      sha={0: "9ad915e169f6434e", FIX_BOUNDARY: "317b0c8102928209"}),
    "real_inside": dict(vertices=8189, cases={0.25: (12962, 589, 2388), 1.0: (14309, 398, 1335), INF: (15990, 0, 390)},
                        sha={0: "3207b4934092c569", FIX_BOUNDARY: "d354a5b654eaf03c"}),
}


def _golden_frame(name):
    g = load_golden(name)
    return g["points"].astype(np.float32), g["valid"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unchanged(a, b):
    return (_bits(a) == _bits(b)).all(axis=1)


# ---- pins of the restatement ------------------------------------------------------------------------------------------------------------
def test_affine_plane():
    """Points (col, row, 2*col + 3*row) on 9 x 13: len2(a, e) = 27 > len2(b, d) = 3, so every cell takes b-d, an interior vertex has 6
    neighbours placed symmetrically around it, their sum is exactly 6p and the vertex does not move; every border vertex does."""
    H, W = 9, 13
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xyz = np.stack([cc, rr, 2 * cc + 3 * rr], axis=-1).astype(np.float32)
    verts, faces = np_mesh(xyz, np.ones((H, W), np.uint8), INF)
    assert len(verts) == 117 and len(faces) == 2 * 8 * 12
    interior = ((rr > 0) & (rr < H - 1) & (cc > 0) & (cc < W - 1)).ravel()
    st = {}
    got = np_smooth(verts, faces, 1, 0.5, 0.0, 0, st)
    assert dict(zip(*np.unique(st["degree"], return_counts=True))) == {2: 2, 3: 2, 4: 36, 6: 77}
    same = _unchanged(got, verts)
    assert interior.sum() == 77 and same[interior].all() and not same[~interior].any()
    assert np.array_equal(st["boundary"], ~interior) and st["boundary"].sum() == 40
    for iterations, mu in ((1, 0.0), (3, MU), (10, MU)):
        fixed = np_smooth(verts, faces, iterations, LAM, mu, FIX_BOUNDARY)
        assert np.array_equal(_bits(fixed), _bits(verts))


def test_hand_computed_example():
    """3 x 3, pixel (0, 2) invalid, vertex 3 at pixel (1, 1) raised to z = 2, no edge-length test.  Cells: (0,0) takes b-d (len2 2 < 6):
    (0,2,1) (1,2,3); (0,1) lacks b: (1,3,4); (1,0) takes a-e (2 <= 6): (2,5,6) (2,6,3); (1,1) takes b-d: (3,6,4) (4,6,7)."""
    xyz = np.zeros((3, 3, 3), np.float32)
    xyz[..., 0], xyz[..., 1] = np.arange(3)[None, :], np.arange(3)[:, None]
    xyz[1, 1, 2] = 2.0
    valid = np.ones((3, 3), np.uint8)
    valid[0, 2] = 0
    verts, faces = np_mesh(xyz, valid, INF)
    assert faces.tolist() == [[0, 2, 1], [1, 2, 3], [1, 3, 4], [2, 5, 6], [2, 6, 3], [3, 6, 4], [4, 6, 7]]
    slots, boundary, st = np_topology(len(verts), faces)
    neighbours = [[1, 2], [0, 2, 3, 4], [0, 1, 3, 5, 6], [1, 2, 4, 6], [1, 3, 6, 7], [2, 6], [2, 3, 4, 5, 7], [4, 6]]
    assert [[int(i) for i in row if i >= 0] for row in slots] == neighbours
    # 14 edges; in one face only: 0-1, 0-2, 1-4, 2-5, 5-6, 6-7, 4-7 -- every vertex but the raised one is an endpoint of one of them
    assert st == dict(edges=14, boundary_edges=7, max_faces_per_edge=2)
    assert boundary.tolist() == [True, True, True, False, True, True, True, True]
    # one step with lambda = 1: every vertex goes to the mean of its neighbours
    want = np.array([[0.5, 0.5, 0.0], [0.75, 0.75, 0.5], [0.6, 1.0, 0.4], [1.0, 1.0, 0.0], [1.25, 1.25, 0.5], [0.5, 1.5, 0.0], [1.0, 1.4, 0.4],
                     [1.5, 1.5, 0.0]], np.float64).astype(np.float32)
    got = np_smooth(verts, faces, 1, 1.0, 0.0)
    assert np.array_equal(_bits(got), _bits(want))
    fixed = np_smooth(verts, faces, 1, 1.0, 0.0, FIX_BOUNDARY)
    assert np.array_equal(_bits(fixed[3]), _bits(want[3])) and np.array_equal(_bits(np.delete(fixed, 3, 0)), _bits(np.delete(verts, 3, 0)))


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_restatement_has_the_pinned_counts_and_hashes(name):
    xyz, valid = _golden_frame(name)
    G = GOLDEN[name]
    for max_edge, (n_faces, n_alone, n_boundary) in G["cases"].items():
        verts, faces = np_mesh(xyz, valid, max_edge)
        assert (len(verts), len(faces)) == (G["vertices"], n_faces)
        for flags in (0, FIX_BOUNDARY):
            st = {}
            got = np_smooth(verts, faces, 10, LAM, MU, flags, st)
            alone = st["degree"] == 0
            assert (int(alone.sum()), int(st["boundary"].sum())) == (n_alone, n_boundary), (name, max_edge)
            assert st["degree"].max() == 8 and st["max_faces_per_edge"] == 2
            # bitwise unchanged: exactly the vertices without a neighbour, plus the boundary ones with the flag; all else moves
            stay = alone | st["boundary"] if flags else alone
            assert np.array_equal(_unchanged(got, verts), stay), (name, max_edge, flags)
            assert np.isfinite(got).all()
            if max_edge == 1.0:
                assert positions_sha256(got)[:16] == G["sha"][flags], (name, flags)


def test_taubin_moves_a_noisy_plane_towards_the_plane():
    rng = np.random.default_rng(5)
    H, W = 40, 48
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    clean = np.stack([0.2 * cc, 0.2 * rr, 500.0 + 0.05 * cc + 0.02 * rr], axis=-1)
    noisy = (clean + rng.normal(0.0, 0.05, size=clean.shape)).astype(np.float32)
    verts, faces = np_mesh(noisy, np.ones((H, W), np.uint8), INF)
    got = np_smooth(verts, faces, 10, LAM, MU)
    interior = ((rr > 0) & (rr < H - 1) & (cc > 0) & (cc < W - 1)).ravel()

    def rms(p):
        return np.sqrt(((p.astype(np.float64) - clean.reshape(-1, 3))[interior] ** 2).sum(axis=1).mean())

    print(f"rms distance to the noise-free points: {rms(verts):.4f} before, {rms(got):.4f} after")
    assert rms(got) < rms(verts)


# ---- the header against the restatement, bit for bit --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_smooth") / "mesh_smooth_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    return exe


def _fmt(x):
    return "inf" if np.isinf(x) else float(np.float32(x)).hex()


class Frame:
    """a frame on disk, written once for every run of the checker over it"""

    def __init__(self, tmp_path, xyz, valid):
        self.H, self.W = valid.shape
        self.dir = tmp_path
        self.fx, self.fv = str(tmp_path / "xyz.bin"), str(tmp_path / "valid.bin")
        np.ascontiguousarray(xyz, dtype=np.float32).tofile(self.fx)
        np.ascontiguousarray(valid, dtype=np.uint8).tofile(self.fv)

    def run(self, exe, max_edge, chunk, iterations, lam, mu, flags, env=None):
        ox, on = str(self.dir / "out_xyz.bin"), str(self.dir / "out_normals.bin")
        subprocess.check_call([exe, self.fx, self.fv, str(self.H), str(self.W), _fmt(max_edge), str(chunk), str(iterations), _fmt(lam), _fmt(mu),
                               str(flags), ox, on], timeout=600, env=env)
        return np.fromfile(ox, dtype=np.float32).reshape(-1, 3), np.fromfile(on, dtype=np.float32).reshape(-1, 3)


def assert_header_equals_restatement(exe, frame, verts, faces, max_edge, chunk, iterations, mu, flags, tag):
    want = np_smooth(verts, faces, iterations, LAM, mu, flags & FIX_BOUNDARY)
    got, got_n = frame.run(exe, max_edge, chunk, iterations, LAM, mu, flags)
    tag = (tag, max_edge, chunk, iterations, float(mu), flags)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), tag      # bit for bit: +0 is not -0
    if flags & NORMALS:
        want_n = np_normals(want, faces)
        assert got_n.shape == want_n.shape and np.array_equal(_bits(got_n), _bits(want_n)), tag
    else:
        assert got_n.size == 0, tag


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_header_equals_restatement_on_the_real_crops(checker, tmp_path, name):
    xyz, valid = _golden_frame(name)
    frame = Frame(tmp_path, xyz, valid)
    for max_edge in (0.25, 1.0, INF):
        verts, faces = np_mesh(xyz, valid, max_edge)
        for flags in range(4):
            for mu in (np.float32(0.0), MU):
                for iterations, chunk in ((1, 1024), (3, 64)):
                    assert_header_equals_restatement(checker, frame, verts, faces, max_edge, chunk, iterations, mu, flags, name)


SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (9, 3), (9, 4), (9, 5), (7, 23), (5, 70)]


def test_random_masks_at_chunk_widths_from_4_up(checker, tmp_path):
    rng = np.random.default_rng(11)
    moved = normals = 0
    for n, (H, W) in enumerate(SHAPES):
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        xyz = (np.stack([0.2 * cc, 0.2 * rr, 500.0 + 0.0 * cc], axis=-1) + rng.normal(0.0, 0.08, size=(H, W, 3))).astype(np.float32)
        for p in (0.0, 0.5, 0.8, 1.0):
            valid = np.ones((H, W), np.uint8) if p >= 1.0 else (rng.random((H, W)) < p).astype(np.uint8)
            d = tmp_path / f"{n}_{p}"
            d.mkdir()
            frame = Frame(d, xyz, valid)
            for max_edge in (0.3, INF):
                verts, faces = np_mesh(xyz, valid, max_edge)
                for chunk, iterations, mu, flags in ((4, 1, MU, 2), (8, 2, np.float32(0.0), 3), (12, 3, MU, 1), (64, 2, MU, 3), (1024, 1, np.float32(0.0), 0)):
                    assert_header_equals_restatement(checker, frame, verts, faces, max_edge, chunk, iterations, mu, flags, (H, W, p))
                moved += int((~_unchanged(np_smooth(verts, faces, 1, LAM, 0.0), verts)).sum())
                normals += int((np_normals(verts, faces) != 0).any(axis=1).sum())
    assert moved > 1000 and normals > 1000


def test_nan_and_inf_coordinates_under_valid_pixels(checker, tmp_path):
    """No special case: the arithmetic of the definition is all there is, in the header as in the restatement."""
    rng = np.random.default_rng(3)
    H, W = 12, 70
    xyz = rng.integers(-1, 2, size=(H, W, 3)).astype(np.float32)
    xyz[3, 5, 1] = np.nan
    xyz[7, 64, 0] = np.inf                                  # (next to a chunk seam at chunk width 64)
    xyz[9, 20] = (np.nan, np.inf, -np.inf)
    valid = np.ones((H, W), np.uint8)
    frame = Frame(tmp_path, xyz, valid)
    verts, faces = np_mesh(xyz, valid, INF)
    assert not np.isfinite(np_smooth(verts, faces, 2, LAM, MU)).all()
    for chunk in (8, 64, 1024):
        assert_header_equals_restatement(checker, frame, verts, faces, INF, chunk, 2, MU, 3, "non-finite")


def test_header_walk_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers, over real_edge."""
    exe = str(tmp_path / "mesh_smooth_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    xyz, valid = _golden_frame("real_edge")
    frame = Frame(tmp_path, xyz, valid)
    for max_edge, chunk, flags in ((0.25, 8, 3), (1.0, 64, 2), (INF, 1024, 1)):
        verts, faces = np_mesh(xyz, valid, max_edge)
        want = np_smooth(verts, faces, 2, LAM, MU, flags & FIX_BOUNDARY)
        got, got_n = frame.run(exe, max_edge, chunk, 2, LAM, MU, flags, env=env)
        assert np.array_equal(_bits(got), _bits(want))
        if flags & NORMALS:
            assert np.array_equal(_bits(got_n), _bits(np_normals(want, faces)))
