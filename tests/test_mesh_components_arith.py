"""CPU test of the mesh components (3dscan_amd/csrc/sl3d_mesh_components.h: the cell plane and the union-find the k_cc_* kernels compile,
free of HIP): the NumPy restatement of the definition (tests/mesh_components_reference.py) is pinned to counts, sizes and hashes that were
not derived from the code under test, a hand-built cell fixes what "filtered" means, and whole frames are walked through the header
in the kernels' sequence and indexing (tests/native/mesh_components_check.cpp, built with ASan and UBSan, the tile width a parameter so
that seams fall everywhere; single-threaded in the kernels' order, and with 8 host threads over std::atomic labels) and compared with
the restatement.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mesh_components_reference import component_sizes, labels_sha256, np_filtered, np_labels, serpentine
from mesh_reference import np_mesh

SRC = os.path.join(ROOT, "tests", "native", "mesh_components_check.cpp")
INF = float("inf")

# the golden crops (points cast to float32, the fixture's own valid map): per max_edge (vertices, faces, components, singletons, the six
# largest sizes, first 16 hex digits of the sha256 of the int32 LE labels)
PINS = {
    "real_edge": {
        0.25: (5234, 4449, 2568, 2511, [1165, 828, 317, 193, 13, 10], "f33e477e3ef12419"),
        1.0: (5234, 5303, 1818, 1651, [1206, 851, 335, 195, 50, 48], "d4ef896d95bb1d12"),
        INF: (5234, 10006, 1, 0, [5234], "d39a480247af3d4e"),
    },
    "real_inside": {
        0.25: (8189, 12962, 625, 589, [7420, 20, 14, 9, 9, 7], "cd6eb76552a5397c"),
        1.0: (8189, 14309, 434, 398, [7600, 21, 14, 11, 10, 8], "f31d2f4a353329c5"),
        INF: (8189, 15990, 1, 0, [8189], "7dcd7bcab805eb62"),
    },
}
# (crop, max_edge, min_vertices) -> (vertices', faces', components kept)
FILTERED = {
    ("real_edge", 1.0, 2): (3583, 5303, 167), ("real_edge", 1.0, 4): (3412, 5246, 110), ("real_edge", 1.0, 16): (2821, 4859, 13),
    ("real_edge", 1.0, 100): (2587, 4614, 4), ("real_edge", 1.0, 1000): (1206, 2209, 1), ("real_edge", 0.25, 16): (2503, 4338, 4),
    ("real_inside", 1.0, 2): (7791, 14309, 36), ("real_inside", 1.0, 16): (7621, 14207, 2), ("real_inside", 1.0, 100): (7600, 14186, 1),
}


def _golden_frame(name):
    g = load_golden(name)
    return g["points"].astype(np.float32), g["valid"]


# ---- pins of the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PINS))
def test_restatement_has_the_pinned_counts_sizes_and_hashes(name):
    xyz, valid = _golden_frame(name)
    for max_edge, (n_v, n_f, n_c, n_single, largest, sha) in PINS[name].items():
        verts, faces = np_mesh(xyz, valid, max_edge)
        lab = np_labels(len(verts), faces)
        roots, sizes = component_sizes(lab)
        in_no_face = np.ones(len(verts), bool)
        in_no_face[faces.ravel()] = False
        assert lab.dtype == np.int32 and (len(verts), len(faces), len(roots)) == (n_v, n_f, n_c), (name, max_edge)
        assert int((sizes == 1).sum()) == n_single == int(in_no_face.sum())
        assert sorted(sizes, reverse=True)[:6] == largest
        assert np.array_equal(lab[lab], lab) and (lab <= np.arange(n_v)).all() and np.array_equal(roots, np.flatnonzero(lab == np.arange(n_v)))
        assert (lab[faces] == lab[faces[:, :1]]).all()
        assert labels_sha256(lab)[:16] == sha, (name, max_edge)


@pytest.mark.parametrize("key", sorted(FILTERED))
def test_restatement_has_the_pinned_filtered_counts(key):
    name, max_edge, min_vertices = key
    xyz, valid = _golden_frame(name)
    verts, faces = np_mesh(xyz, valid, max_edge)
    v2, f2, ids = np_filtered(verts, faces, min_vertices)
    assert (len(v2), len(f2), len(np.unique(np_labels(len(v2), f2)))) == FILTERED[key]
    assert np.array_equal(v2.view(np.uint32), verts[ids].view(np.uint32)) and (np.diff(ids) > 0).all()
    assert np.array_equal(ids[f2], faces[np.isin(faces[:, 0], ids)])              # the original faces among the kept, in the original order
    one = np_filtered(verts, faces, 1)
    assert np.array_equal(one[0].view(np.uint32), verts.view(np.uint32)) and np.array_equal(one[1], faces) and np.array_equal(one[2], np.arange(len(verts)))


# ---- the definition: the face list is filtered, never derived again -------------------------------------------------------------------
def _hand_built():
    """5 x 5 pixels around the cell a = (2,2), b = (2,3), d = (3,2), e = (3,3): a between b and d, e near a alone; the pixels right of and
    below e are invalid, everything else is one sheet."""
    H = W = 5
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xyz = np.stack([0.01 * cc, 0.01 * rr, 0.0 * cc], axis=-1).astype(np.float32)
    xyz[2, 3, 2], xyz[3, 2, 2], xyz[3, 3, 0] = 0.5, -0.5, 0.02 + 0.95
    valid = np.ones((H, W), np.uint8)
    valid[2, 4] = valid[3, 4] = valid[4, 2:] = 0
    return xyz, valid, 1.01


def test_filtered_mesh_is_not_the_mesh_of_the_filtered_valid_map():
    xyz, valid, max_edge = _hand_built()
    P = xyz.astype(np.float64)
    a, b, d, e = P[2, 2], P[2, 3], P[3, 2], P[3, 3]
    len2 = lambda p, q: float(((p - q) ** 2).sum())
    thr2 = float(np.float32(max_edge)) ** 2
    assert len2(a, e) <= len2(b, d) <= thr2 and len2(d, e) > thr2 and len2(b, e) > thr2 and len2(a, d) <= thr2 and len2(a, b) <= thr2
    verts, faces = np_mesh(xyz, valid, max_edge)
    vid = (np.cumsum(valid.ravel()) - 1).reshape(valid.shape)
    ia, ib, id_, ie = (int(vid[p]) for p in ((2, 2), (2, 3), (3, 2), (3, 3)))
    lab = np_labels(len(verts), faces)
    size = np.bincount(lab, minlength=len(verts))[lab]
    assert size[ie] == 1 and lab[ia] == lab[ib] == lab[id_] and size[ia] >= 10      # e a fragment; a, b, d in the sheet
    v2, f2, ids = np_filtered(verts, faces, 2)
    assert ie not in ids and {ia, ib, id_} <= set(ids.tolist())
    adb = [ia, id_, ib]
    assert not (ids[f2] == adb).all(axis=1).any() and not (faces == adb).all(axis=1).any()   # the cell has no face, filtered or not
    valid2 = valid.copy()
    valid2[3, 3] = 0
    verts3, faces3 = np_mesh(xyz, valid2, max_edge)
    vid2 = (np.cumsum(valid2.ravel()) - 1).reshape(valid.shape)
    invented = [int(vid2[2, 2]), int(vid2[3, 2]), int(vid2[2, 3])]
    assert (faces3 == invented).all(axis=1).any()                                  # ... the three-corner rule would invent (a, d, b)
    assert np.array_equal(verts3.view(np.uint32), v2.view(np.uint32)) and len(faces3) == len(f2) + 1


# ---- the header against the restatement ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_components") / "mesh_components_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-pthread", SRC, "-o", exe])
    return exe


def _fmt(max_edge):
    return "inf" if np.isinf(max_edge) else float(np.float32(max_edge)).hex()


def run_checker(exe, tmp_path, xyz, valid, max_edge, chunk, threads, min_vertices):
    H, W = valid.shape
    fx, fv, ol, ov, of, oi = (str(tmp_path / n) for n in ("xyz.bin", "valid.bin", "labels.bin", "verts.bin", "faces.bin", "ids.bin"))
    np.ascontiguousarray(xyz, dtype=np.float32).tofile(fx)
    np.ascontiguousarray(valid, dtype=np.uint8).tofile(fv)
    subprocess.check_call([exe, fx, fv, str(H), str(W), _fmt(max_edge), str(chunk), str(threads), str(min_vertices), ol, ov, of, oi], timeout=600)
    return (np.fromfile(ol, dtype=np.int32), np.fromfile(ov, dtype=np.float32).reshape(-1, 3), np.fromfile(of, dtype=np.int32).reshape(-1, 3),
            np.fromfile(oi, dtype=np.int32))


def assert_header_equals_restatement(exe, tmp_path, xyz, valid, max_edge, chunks, mins):
    verts, faces = np_mesh(xyz, valid, max_edge)
    want_lab = np_labels(len(verts), faces)
    for min_vertices in mins:
        want = np_filtered(verts, faces, min_vertices)
        for chunk in chunks:
            for threads in (1, 8):
                tag = (valid.shape, max_edge, chunk, threads, min_vertices)
                lab, v2, f2, ids = run_checker(exe, tmp_path, xyz, valid, max_edge, chunk, threads, min_vertices)
                assert np.array_equal(lab, want_lab), tag
                assert np.array_equal(v2.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(f2, want[1]) and np.array_equal(ids, want[2]), tag
    return want_lab


@pytest.mark.parametrize("name", sorted(PINS))
def test_header_equals_restatement_on_the_real_crops(checker, tmp_path, name):
    xyz, valid = _golden_frame(name)
    for max_edge in (0.25, 1.0, INF):
        assert_header_equals_restatement(checker, tmp_path, xyz, valid, max_edge, (8, 64, 1024), (1, 16) if max_edge == 1.0 else (2,))


def _plane(H, W):
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([0.2 * cc, 0.2 * rr, 500.0 + 0.05 * cc - 0.03 * rr], axis=-1).astype(np.float32)


def test_header_equals_restatement_on_random_masks(checker, tmp_path):
    rng = np.random.default_rng(5)
    for H, W in [(1, 37), (37, 1), (2, 2), (9, 5), (33, 70), (5, 1025)]:
        valid = (rng.random((H, W)) < 0.6).astype(np.uint8)
        xyz = _plane(H, W) + rng.normal(0.0, 0.05, size=(H, W, 3)).astype(np.float32)
        for max_edge in (0.3, INF):
            lab = assert_header_equals_restatement(checker, tmp_path, xyz, valid, max_edge, (4, 16, 1024), (1, 3))
            if H > 8 and W > 8:
                assert 3 < len(np.unique(lab)) < len(lab)
    hand = _hand_built()
    assert_header_equals_restatement(checker, tmp_path, hand[0], hand[1], hand[2], (4, 1024), (1, 2))


def test_header_equals_restatement_on_the_serpentine(checker, tmp_path):
    """One component that winds through the whole frame: the minimum label travels its whole length, across every tile seam."""
    H, W = 41, 257
    valid = serpentine(H, W, 5, 3)
    lab = assert_header_equals_restatement(checker, tmp_path, _plane(H, W), valid, INF, (4, 32), (1, 2))
    assert (lab == 0).all() and len(lab) == int(valid.sum()) > 0.6 * H * W
    valid = serpentine(W, H, 5, 3, vertical=True)
    lab = assert_header_equals_restatement(checker, tmp_path, _plane(W, H), valid, INF, (4, 32), (1,))
    assert (lab == 0).all()
