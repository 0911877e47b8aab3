"""CPU test of the hole-filling arithmetic (3dscan_amd/csrc/sl3d_mesh_holes.h: hole_find / hole_union with the OUTSIDE root, hole_walk_from,
hole_usable, hole_position -- the header the kernels of sl3d_mesh_holes.hip compile, free of HIP): whole frames walked through the header
with the kernels' chunk and lane indexing (tests/native/mesh_holes_check.cpp, chunk width a parameter so that the seams fall everywhere,
one thread and eight) and compared bit for bit with the NumPy restatement of the definition (tests/mesh_holes_reference.py: a flood fill,
no union-find).  The restatement itself is pinned to a hand-computed example, to affine exactness, to the identity at max_hole 0 and to
counts of the golden crops that were computed in advance by a separate restatement -- none of them derived from the code under test."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases
import mesh_holes_cases as HC
from conftest import ROOT, load_golden
from mesh_holes_reference import NORMALS, fill_mesh, filtered_candidates, np_fill, np_holes
from mesh_normals_reference import np_normals
from mesh_reference import np_mesh

SRC = os.path.join(ROOT, "tests", "native", "mesh_holes_check.cpp")
INF = float("inf")
FLAGS_OF_THE_CHECK = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-pthread"]
CHUNK_WIDTHS = (4, 20, 64, 252, 1024)

# (crop, max_edge, min_vertices, max_hole, fill_edge): holes, hole pixels, both / only the row / only the column interpolant usable, none,
# faces of the candidate map's mesh, faces of the filled mesh -- points cast to float32, the fixture's own valid map; computed in advance
# with a separate restatement of the definition
GOLDEN_COUNTS = {
    ("real_edge", INF, 1, 64, 1.0): (13, 169, 41, 25, 50, 53, 10006, 10309),
    ("real_edge", 1.0, 1, 16, 0.5): (10, 30, 1, 1, 2, 26, 5303, 5306),
    ("real_edge", 1.0, 100, 16, 1.0): (12, 42, 42, 0, 0, 0, 4614, 4775),
    ("real_edge", 3.0, 20, 4, 1.0): (60, 92, 36, 11, 23, 22, 6456, 6706),
    ("real_edge", 3.0, 20, 1000, 0.5): (73, 521, 152, 109, 120, 140, 6456, 7451),
    ("real_inside", INF, 1, 4, INF): (2, 3, 3, 0, 0, 0, 15990, 16002),
    ("real_inside", 1.0, 100, 1, 1.0): (72, 72, 72, 0, 0, 0, 14186, 14473),
    ("real_inside", 1.0, 100, 64, 0.5): (112, 267, 255, 9, 2, 1, 14186, 15172),
    ("real_inside", 3.0, 20, 16, 0.5): (98, 188, 151, 17, 9, 11, 14885, 15539),
}


def _golden_frame(name):
    g = load_golden(name)
    return g["points"].astype(np.float32), g["valid"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counts_of(st):
    return tuple(st[k] for k in ("holes", "hole_pixels", "both", "only_h", "only_v", "none"))


def golden_row(xyz, valid, cand, max_edge, max_hole, fill_edge):
    """the eight figures of a GOLDEN_COUNTS row from the restatement (candidate map `cand` given)"""
    st = {}
    _, faces, _, _ = fill_mesh(xyz, valid, cand, max_edge, max_hole, fill_edge, 0, st)
    _, before = np_mesh(np.where(cand[..., None] == 1, xyz, np.float32(0.0)), cand, max_edge)
    return counts_of(st) + (len(before), len(faces))


# ---- pins of the restatement ------------------------------------------------------------------------------------------------------------
def hand_example():
    """5 x 6, points (c, r, c^2), every pixel a candidate but (1,2), (2,2), (2,3): one hole of 3 pixels.
    (1,2): L = (1,1), R = (1,3), dl = dr = 1: h = (2, 1, 5); U = (0,2), D = (3,2), du = 1, dd = 2: v = (2, 1, 4); (3 h + 2 v) / 5
    (2,2): L = (2,1), R = (2,4), dl = 1, dr = 2: h.z = (2*1 + 1*16) / 3 = 6; U = (0,2), D = (3,2), du = 2, dd = 1: v = (2, 2, 4);
           (3 h + 3 v) / 6 = (2, 2, 5)
    (2,3): L = (2,1), R = (2,4), dl = 2, dr = 1: h.z = (1*1 + 2*16) / 3 = 11; U = (1,3), D = (3,3), du = dd = 1: v = (3, 2, 9);
           (2 h + 3 v) / 5 = (3, 2, 9.8)
    fill_edge 2: the row spans have len2 2^2 + 8^2 = 68 > 4^2 at (1,2) and 3^2 + 15^2 = 234 > 6^2 at (2,2), (2,3): unusable; the column
    spans have len2 9 <= 6^2 and 4 <= 4^2: the column interpolants alone"""
    H, W = 5, 6
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xyz = np.stack([cc, rr, cc * cc], axis=-1).astype(np.float32)
    cand = np.ones((H, W), np.uint8)
    cand[1, 2] = cand[2, 2] = cand[2, 3] = 0
    return xyz, cand


def test_hand_computed_example():
    xyz, cand = hand_example()
    at = [(1, 2), (2, 2), (2, 3)]
    st = {}
    got, valid, filled = np_fill(xyz, cand, 3, INF, st)
    assert counts_of(st) == (1, 3, 3, 0, 0, 0) and valid.all() and [tuple(p) for p in np.argwhere(filled)] == at
    want = np.array([(2, 1, 4.6), (2, 2, 5), (3, 2, 9.8)], np.float32)
    assert np.array_equal(_bits(np.array([got[p] for p in at])), _bits(want))
    assert np.array_equal(_bits(got[cand == 1]), _bits(xyz[cand == 1]))
    st = {}
    got, valid, filled = np_fill(xyz, cand, 3, 2.0, st)
    assert counts_of(st) == (1, 3, 0, 0, 3, 0) and valid.all()
    want = np.array([(2, 1, 4), (2, 2, 4), (3, 2, 9)], np.float32)
    assert np.array_equal(_bits(np.array([got[p] for p in at])), _bits(want))
    st = {}
    got, valid, filled = np_fill(xyz, cand, 2, INF, st)
    assert counts_of(st) == (0, 0, 0, 0, 0, 0) and np.array_equal(valid, cand) and not filled.any()
    assert not got[cand == 0].any()
    # the ids: candidates keep their place in the cloud, filled vertices carry -1
    verts, faces, ids, normals = fill_mesh(xyz, cand, cand, INF, 3, INF)
    want_ids = np.arange(27)
    want_ids = np.insert(want_ids, [8, 13, 13], -1)
    assert ids.tolist() == want_ids.tolist() and len(verts) == 30 and len(faces) == 2 * 4 * 5 and normals is None


def test_two_holes_that_meet_at_a_corner_are_judged_separately():
    cand = np.ones((6, 6), np.uint8)
    cand[1:3, 1:3] = 0
    cand[3:5, 3:5] = 0
    hole, n = np_holes(cand, 4)
    assert n == 2 and hole.sum() == 8
    assert np_holes(cand, 3)[1] == 0
    cand[2, 3] = 0                                       # now one component of 9
    assert np_holes(cand, 8)[1] == 0 and np_holes(cand, 9)[1] == 1


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -10, 2.0 ** 20])
def test_affine_exactness(scale):
    """points on (2c - 7r, c + 3r, c + r - 100) s: small integers times a power of two, so every product, sum and quotient of the
    position is exact and a filled pixel carries the plane's own bits"""
    H, W = 40, 90
    rng = np.random.default_rng(5)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xyz = (np.stack([2 * cc - 7 * rr, cc + 3 * rr, cc + rr - 100], axis=-1) * scale).astype(np.float32)
    cand = (rng.random((H, W)) < 0.8).astype(np.uint8)
    st = {}
    got, valid, filled = np_fill(xyz, cand, H * W, INF, st)
    assert st["holes"] > 50 and st["both"] == st["hole_pixels"] == int(filled.sum()) > 100
    assert np.array_equal(_bits(got[filled]), _bits(xyz[filled]))


def test_restatement_has_the_pinned_counts():
    for (name, max_edge, min_vertices, max_hole, fill_edge), want in GOLDEN_COUNTS.items():
        xyz, valid = _golden_frame(name)
        cand = filtered_candidates(xyz, valid, max_edge, min_vertices)
        assert golden_row(xyz, valid, cand, max_edge, max_hole, fill_edge) == want, (name, max_edge, min_vertices, max_hole, fill_edge)


@pytest.mark.parametrize("name", ["real_edge", "real_inside"])
def test_max_hole_0_is_the_mesh(name):
    xyz, valid = _golden_frame(name)
    for max_edge in (0.25, 1.0, INF):
        want_v, want_f = np_mesh(xyz, valid, max_edge)
        for flags in (0, NORMALS):
            verts, faces, ids, normals = fill_mesh(xyz, valid, valid, max_edge, 0, 1.0, flags)
            assert np.array_equal(_bits(verts), _bits(want_v)) and np.array_equal(faces, want_f)
            assert np.array_equal(ids, np.arange(len(want_v)))
            if flags & NORMALS:
                assert np.array_equal(_bits(normals), _bits(np_normals(want_v, want_f)))


# ---- the header against the restatement, bit for bit --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_holes") / "mesh_holes_check")
    subprocess.check_call(["g++", "-O2", *FLAGS_OF_THE_CHECK, SRC, "-o", exe])
    return exe


def _fmt(x):
    return "inf" if np.isinf(x) else float(np.float32(x)).hex()


class Frame:
    """a frame on disk, written once for every run of the checker over it"""

    def __init__(self, tmp_path, xyz, cand):
        self.H, self.W = cand.shape
        self.dir = tmp_path
        self.fx, self.fc = str(tmp_path / "xyz.bin"), str(tmp_path / "cand.bin")
        np.ascontiguousarray(xyz, dtype=np.float32).tofile(self.fx)
        np.ascontiguousarray(cand, dtype=np.uint8).tofile(self.fc)

    def run(self, exe, max_hole, fill_edge, chunk_w, threads, env=None):
        ox, ov, os_ = (str(self.dir / f"out_{k}.bin") for k in ("xyz", "valid", "stats"))
        subprocess.check_call([exe, self.fx, self.fc, str(self.H), str(self.W), str(max_hole), _fmt(fill_edge), str(chunk_w), str(threads), ox, ov, os_],
                              timeout=600, env=env)
        return (np.fromfile(ox, dtype=np.float32).reshape(self.H, self.W, 3), np.fromfile(ov, dtype=np.uint8).reshape(self.H, self.W),
                np.fromfile(os_, dtype=np.int64).tolist())


def assert_header_equals_restatement(exe, frame, xyz, cand, max_hole, fill_edge, chunk_w, threads, tag, stats=None, env=None):
    """-> the restatement's (filled xyz, filled valid)"""
    st = {}
    want, want_valid, filled = np_fill(xyz, cand, max_hole, fill_edge, st)
    got, got_valid, (n_holes, n_filled) = frame.run(exe, max_hole, fill_edge, chunk_w, threads, env=env)
    tag = (tag, max_hole, fill_edge, chunk_w, threads)
    assert np.array_equal(got_valid, want_valid), tag
    assert (n_holes, n_filled) == (st["holes"], int(filled.sum())), tag
    keep = ~filled                                                                # candidates: copies, bit for bit; filled: produced
    assert mesh_cases.bits_differ(got[keep], want[keep]) == 0 and mesh_cases.bits_differ(got[filled], want[filled], produced=True) == 0, tag
    if stats is not None:
        for k, v in st.items():
            stats[k] = stats.get(k, 0) + v
    return want, want_valid


@pytest.mark.parametrize("name", ["real_edge", "real_inside"])
def test_header_equals_restatement_on_the_real_crops(checker, tmp_path, name):
    xyz, valid = _golden_frame(name)
    stats, n = {}, 0
    for (crop, max_edge, min_vertices, max_hole, fill_edge) in GOLDEN_COUNTS:
        if crop != name:
            continue
        cand = filtered_candidates(xyz, valid, max_edge, min_vertices)
        d = tmp_path / str(n)
        d.mkdir()
        frame = Frame(d, xyz, cand)
        for threads in (1, 8):
            for j in range(2):
                n += 1
                assert_header_equals_restatement(checker, frame, xyz, cand, max_hole, fill_edge, CHUNK_WIDTHS[n % len(CHUNK_WIDTHS)], threads, name, stats)
    # what keeps this from passing vacuously
    assert stats["holes"] > 0 and stats["both"] > 0 and stats["only_h"] > 0 and stats["only_v"] > 0 and stats["none"] > 0


@pytest.mark.parametrize("shape", HC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_equals_restatement_on_the_crafted_cases(checker, tmp_path, shape):
    n, stats = 0, {}
    clean = None
    for name, xyz, valid, runs in HC.cases_of(shape):
        d = tmp_path / name
        d.mkdir()
        frame = Frame(d, xyz, valid)
        results = []
        for max_hole, fill_edge in runs:
            for threads in (1, 8):
                n += 1
                results.append(assert_header_equals_restatement(checker, frame, xyz, valid, max_hole, fill_edge, CHUNK_WIDTHS[n % len(CHUNK_WIDTHS)],
                                                                threads, name, stats))
        # garbage under the non-candidates changes nothing: the twin's results are the clean case's
        if name.endswith("clean"):
            clean = results
        elif name.endswith("garbage"):
            assert len(clean) == len(results)
            for (a, av), (b, bv) in zip(clean, results):
                assert np.array_equal(av, bv) and mesh_cases.bits_differ(a, b, produced=True) == 0
    H, W = shape
    if H < 3 or W < 3:
        assert stats["holes"] == 0                                                # no interior
    elif H >= 9:
        assert stats["holes"] > 0 and stats["both"] > 0 and stats["none"] > 0


def test_crafted_features_are_what_they_claim():
    """the restatement over the 9 x 2049 feature map: which features qualify at MAX_HOLE and at MAX_HOLE_LARGE"""
    m = HC.features(9, 2049)
    small, n_small = np_holes(m, HC.MAX_HOLE)
    large, n_large = np_holes(m, HC.MAX_HOLE_LARGE)

    def state(name, hole):
        px = np.zeros_like(m, bool)
        for r0, r1, c0, c1 in HC.FEATURES[name]:
            px[r0:r1, c0:c1] = True
        px &= m == 0
        inside = hole[px]
        assert inside.all() or not inside.any(), name
        return bool(inside.all()), int(px.sum())

    assert state("chunk", small) == (True, HC.MAX_HOLE) and state("too_large", small) == (False, HC.MAX_HOLE + 1)
    assert state("too_large", large)[0] and state("quad", small)[0] and state("wave", small)[0] and state("tiny", small)[0]
    assert state("corner", small) == (True, 18) and state("annulus", small) == (True, 8) and state("u_shape", small) == (True, 11)
    assert not state("borders", large)[0] and not large[4:6, 2047:].any()
    assert not large[0:3, 160:162].any() and small[1:3, 163:165].all()            # the wall: one is outside, its neighbour a hole
    assert n_large == n_small + 1 == 10
    assert HC.MAX_HOLE < 18 < HC.MAX_HOLE_LARGE                                   # the two corner holes together would not qualify at MAX_HOLE


def test_serpentine_hole(checker, tmp_path):
    (name, xyz, valid, runs), size = HC.serpentine_case()
    frame = Frame(tmp_path, xyz, valid)
    for i, (max_hole, fill_edge) in enumerate(runs):
        st = {}
        assert_header_equals_restatement(checker, frame, xyz, valid, max_hole, fill_edge, (1024, 252, 64)[i], (1, 8, 8)[i], name, st)
        assert st["holes"] == (max_hole >= size) and st["hole_pixels"] == (size if max_hole >= size else 0) and size > 20000


def test_random_masks_at_every_chunk_width(checker, tmp_path):
    rng = np.random.default_rng(23)
    for n, (H, W) in enumerate([(9, 2049), (5, 1027), (40, 300), (300, 7), (5, 7)]):
        xyz = (mesh_cases.plane(H, W) + rng.normal(0.0, 0.08, size=(H, W, 3))).astype(np.float32)
        for p in (0.55, 0.8, 0.97):
            cand = (rng.random((H, W)) < p).astype(np.uint8)
            d = tmp_path / f"{n}_{p}"
            d.mkdir()
            frame = Frame(d, xyz, cand)
            for i, chunk_w in enumerate(CHUNK_WIDTHS):
                assert_header_equals_restatement(checker, frame, xyz, cand, (2, 7, 30, 1000, H * W)[i], (0.3, INF)[i % 2], chunk_w, (1, 8)[(i + n) % 2], (H, W, p))


def test_header_walk_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers, over real_edge and a crafted frame."""
    exe = str(tmp_path / "mesh_holes_check_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS_OF_THE_CHECK, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    xyz, valid = _golden_frame("real_edge")
    frame = Frame(tmp_path, xyz, valid)
    for max_hole, fill_edge, chunk_w, threads in ((64, 1.0, 20, 1), (1000, INF, 1024, 8), (0, 0.5, 64, 1), (16, 0.5, 4, 8)):
        assert_header_equals_restatement(exe, frame, xyz, valid, max_hole, fill_edge, chunk_w, threads, "sanitizers", env=env)
    name, xyz, valid, runs = HC.cases_of((9, 1025))[1]
    d = tmp_path / "crafted"
    d.mkdir()
    frame = Frame(d, xyz, valid)
    for max_hole, fill_edge in runs:
        assert_header_equals_restatement(exe, frame, xyz, valid, max_hole, fill_edge, 252, 8, name, env=env)
