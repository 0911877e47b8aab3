"""CPU test of the crafted mesh cases (tests/mesh_cases.py): (1) the cases are what they claim to be -- exact ties, threshold hits,
contraction-sensitive cells, non-finite vertices in or out of the faces, denormals, an overflow in a mu step, the component structure of
the topologies -- stated with the NumPy restatements alone; (2) the host headers (tests/native/*_check.cpp, the code the kernels
compile) stay tied to the restatements on every case, bit for bit, at chunk widths 64 and 1024.  The same cases run on the device in
tests/test_gpu_mesh_crafted.py."""
import subprocess

import numpy as np
import pytest

import mesh_cases as MC
import test_mesh_arith as TM
import test_mesh_components_arith as TC
import test_mesh_normals_arith as TN
import test_mesh_smooth_arith as TS
from mesh_components_reference import np_filtered, np_labels
from mesh_normals_reference import np_normals
from mesh_reference import check_faces, np_mesh
from mesh_smooth_reference import FIX_BOUNDARY, np_smooth

INF = float("inf")
CHUNKS = (64, 1024)


def _cases(prefix, shapes=MC.ALL_SHAPES):
    return [c for s in shapes for c in MC.cases_of(s) if c[0].startswith(prefix)]


def _in_a_face(n, faces):
    used = np.zeros(n, bool)
    used[np.asarray(faces).ravel()] = True
    return used


# ---- 1. what the cases contain ----------------------------------------------------------------------------------------------------------
def test_integer_cases_hit_ties_thresholds_and_zero_normals():
    ties = hits = coincident = zero_normal_in_a_face = 0
    for name, xyz, valid, edges in _cases("integers"):
        for max_edge in edges:
            st = {}
            verts, faces = np_mesh(xyz, valid, max_edge, st)
            ties += st["ties"]
            hits += st["at_threshold"]
            n = np_normals(verts, faces)
            zero_normal_in_a_face += int((_in_a_face(len(verts), faces) & ~n.any(axis=1)).sum())
            if len(faces):
                p = verts[faces]
                coincident += int(((p[:, 0] == p[:, 1]).all(axis=1) | (p[:, 1] == p[:, 2]).all(axis=1) | (p[:, 0] == p[:, 2]).all(axis=1)).sum())
    print(f"integer cases: {ties} ties, {hits} threshold hits, {coincident} faces with coincident corners, "
          f"{zero_normal_in_a_face} vertices in a face with the zero normal")
    assert ties > 100 and hits > 100 and coincident > 100 and zero_normal_in_a_face > 100


def test_swapped_cells_tie_only_without_contraction():
    cells = took_bd_x = took_bd_y = 0
    for name, xyz, valid, edges in _cases("swapped"):
        shape = valid.shape
        sw = MC.swapped_cells(shape)
        tie, fused_x, fused_y = MC.swapped_diagonals(xyz, sw)
        assert tie.all(), name
        st = {}
        verts, faces = np_mesh(xyz, valid, INF, st)
        # the swapped cells are the only candidates; all of them tie, take a-e and give two faces
        assert st["ties"] == st["diag_ae"] == len(sw) and st["diag_bd"] == st["three"] == 0 and len(faces) == 2 * len(sw), name
        assert MC.swapped_took_bd(faces, valid, sw) == 0
        cells += len(sw)
        took_bd_x += int(fused_x.sum())
        took_bd_y += int(fused_y.sum())
        if shape[1] >= 1023:                         # every wide shape alone would notice either form (one flipped cell fails the test)
            assert fused_x.sum() >= 16 and fused_y.sum() >= 16, (name, fused_x.sum(), fused_y.sum())
    print(f"swapped cells: {cells}; b-d under fma(dx, dx, dy*dy): {took_bd_x}, under fma(dy, dy, dx*dx): {took_bd_y}")
    assert cells > 1000 and took_bd_x >= 32 and took_bd_y >= 32


def test_nonfinite_vertices_and_their_faces():
    seen = {k: 0 for k in MC.KINDS}
    for name, xyz, valid, edges in _cases("nonfinite"):
        H, W = valid.shape
        vid = (np.cumsum(valid.ravel()) - 1).reshape(H, W)
        spots = MC.special_positions(H, W)
        assert (~np.isfinite(xyz)).any(axis=-1).sum() == len(spots) >= 2
        if name.endswith("garbage"):
            assert (xyz[valid == 0] == MC.GARBAGE).all() and (valid == 0).any() == (H * W > 30)
        for max_edge in edges:
            verts, faces = np_mesh(xyz, valid, max_edge)
            used = _in_a_face(len(verts), faces)
            check_faces(faces, valid, len(verts))
            for r, c, kind in spots:
                assert valid[r, c] == 1
                if kind in ("nan", "mixed"):
                    assert not used[vid[r, c]], (name, r, c, kind, max_edge)          # every edge at a NaN point has a NaN length
                elif H > 1 and W > 1:
                    assert used[vid[r, c]] == (max_edge == INF), (name, r, c, kind, max_edge)   # an infinite one is short only without a test
                seen[kind] += 1
    assert min(seen.values()) >= 8, seen


def test_range_cases_reach_the_ends_of_the_float_range():
    tiny = np.finfo(np.float32).tiny
    overflowed = 0
    for name, xyz, valid, edges in _cases("range"):
        H, W = valid.shape
        assert np.isfinite(xyz).all()
        if name.endswith("denormal"):
            a = np.abs(xyz[valid == 1])
            assert ((a > 0) & (a < tiny)).mean() > 0.9 and a.max() < 1e-36
            if H > 1 and W > 4:
                st = {}
                _, faces = np_mesh(xyz, valid, edges[0], st)
                assert 0 < st["rejected"] < st["candidates"] and len(faces) > 0      # max_edge, a denormal itself, splits the edges
        elif name.endswith("huge"):
            assert np.abs(xyz[..., 0]).max() > 3.4e38
            verts, faces = np_mesh(xyz, valid, INF)
            lam_only = np_smooth(verts, faces, 1, MC.LAMBDA, 0.0, FIX_BOUNDARY)
            both = np_smooth(verts, faces, 1, MC.LAMBDA, -0.53, FIX_BOUNDARY)
            assert np.isfinite(lam_only).all(), name                                  # a step towards the mean stays inside the range
            if (H, W) == MC.HUGE_SHAPE:                                                # crests with moving neighbours all around
                assert np.isinf(both).any() and not np.isnan(both).any(), name        # the mu step left it
                assert np.isnan(np_smooth(verts, faces, 2, MC.LAMBDA, -0.53, FIX_BOUNDARY)).any(), name    # and the step after makes NaNs of it
                overflowed += int(np.isinf(both).any(axis=1).sum())
        else:
            assert name.endswith("1e5") and xyz.min() > 9e4
    print(f"huge cases: {overflowed} vertices leave the float range in the first mu step")
    assert overflowed > 100


def test_topologies_have_the_components_they_are_built_for():
    for name, xyz, valid, edges in _cases(("checkerboard", "comb", "spiral", "blocks", "lone_face", "percolation")):
        verts, faces = np_mesh(xyz, valid, edges[0])
        check_faces(faces, valid, len(verts))
        lab = np_labels(len(verts), faces)
        sizes = np.bincount(lab)[np.unique(lab)]
        H, W = valid.shape
        if name.startswith("checkerboard"):
            assert len(faces) == 0 and np.array_equal(lab, np.arange(len(verts))) and len(verts) == (H * W + 1) // 2
        elif name.startswith(("comb", "spiral")):
            assert len(sizes) == 1 and (lab == 0).all() and len(verts) > 2000, (name, len(sizes))
        if name.startswith("spiral"):
            # a spiral, not rings with shortcuts: closing any one door cuts it in two
            doors = MC.spiral_doors(H, W)
            assert len(doors) >= 10
            for k in range(0, len(doors), 2):
                closed = valid.copy()
                closed[doors[k]] = closed[doors[k + 1]] = 0
                v2, f2 = np_mesh(xyz, closed, INF)
                assert len(np.unique(np_labels(len(v2), f2))) == 2, k
        if name.startswith("blocks"):
            assert len(sizes) == 1
            vid = (np.cumsum(valid.ravel()) - 1).reshape(H, W)
            bridge = [vid[H - 2, 1023], vid[H - 1, 1023], vid[H - 1, 1024]]             # (a, d, e) of the cell at column 1023, last cell row
            k = np.flatnonzero((faces == bridge).all(axis=1))
            assert len(k) == 1
            left = np.delete(faces, k[0], axis=0)
            parts = np.unique(np_labels(len(verts), left), return_counts=True)[1]
            assert len(parts) == 2 and parts.min() > 0.45 * len(verts)                 # without that face: two blocks
        if name.startswith("lone_face"):
            vid = (np.cumsum(valid.ravel()) - 1).reshape(H, W)
            assert valid[0, :1024].sum() == 0
            assert (faces == [vid[0, 1024], vid[1, 1023], vid[1, 1024]]).all(axis=1).sum() == 1   # (b, d, e): chunk (row 0, 0) has 1 face, 0 vertices
            # row 0 and row 1 from column 1023 on are one sheet; row 1 left of it has no second row: singletons, like 3 of the islands' pixels
            assert sorted(sizes)[-4:] == [3, 4, 4, 1025 + 1026] and (sizes == 1).sum() == 1023 + 3
            assert MC.second_largest(lab) == 4
        if name.startswith("percolation"):
            print(f"{name}: max_edge {edges[0]:.6g}, {len(faces)} faces, {len(sizes)} components, the largest {sizes.max()} of {len(verts)} vertices")
            assert len(sizes) > 50 and sizes.max() > 0.2 * len(verts)


# ---- 2. the host headers on every case --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_cases")
    flags = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-pthread"]
    exes = {}
    for key, mod in (("mesh", TM), ("normals", TN), ("components", TC), ("smooth", TS)):
        exes[key] = str(d / key)
        subprocess.check_call(flags + [mod.SRC, "-o", exes[key]])
    return exes


def _differ(got, want):
    return MC.bits_differ(got, want)            # bit for bit: host header and restatement are both x86 code, a produced NaN is the same NaN


@pytest.mark.parametrize("shape", MC.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_headers_equal_the_restatements_on_every_case(checkers, tmp_path, shape):
    n = 0
    for name, xyz, valid, edges in MC.cases_of(shape):
        frame = TS.Frame(tmp_path, xyz, valid)
        for max_edge in edges:
            verts, faces = np_mesh(xyz, valid, max_edge)
            normals = np_normals(verts, faces)
            lab = np_labels(len(verts), faces)
            s = MC.second_largest(lab)
            smooth = {(it, mu, fl): np_smooth(verts, faces, it, MC.LAMBDA, mu, fl) for it, mu, fl in MC.SMOOTH_RUNS}
            for chunk in CHUNKS:
                tag = (name, max_edge, chunk)
                gv, gf = TM.run_checker(checkers["mesh"], tmp_path, xyz, valid, max_edge, chunk)
                assert _differ(gv, verts) == 0 and gf.shape == faces.shape and np.array_equal(gf, faces), tag
                assert _differ(TN.run_checker(checkers["normals"], tmp_path, xyz, valid, max_edge, chunk), normals) == 0, tag
                for min_vertices in ((1, s) if chunk == 64 else (2, s + 1)):
                    want = np_filtered(verts, faces, min_vertices)
                    gl, v2, f2, ids = TC.run_checker(checkers["components"], tmp_path, xyz, valid, max_edge, chunk, 1 if chunk == 64 else 8, min_vertices)
                    assert np.array_equal(gl, lab), tag
                    assert _differ(v2, want[0]) == 0 and np.array_equal(f2, want[1]) and np.array_equal(ids, want[2]), (tag, min_vertices)
                for (it, mu, fl), want in smooth.items():
                    got, got_n = frame.run(checkers["smooth"], max_edge, chunk, it, np.float32(MC.LAMBDA), np.float32(mu), fl)
                    if fl & 2:
                        assert _differ(got, want[0]) == 0 and _differ(got_n, want[1]) == 0, (tag, it, mu, fl)
                    else:
                        assert _differ(got, want) == 0 and got_n.size == 0, (tag, it, mu, fl)
                n += 1
    assert n > 0
