"""GPU tests (-m gpu) of the mesh, normal, component and smoothing kernels on crafted dense planes (tests/mesh_cases.py, written into a
context by tests/dense_planes.py): the inputs on which the definitions have special cases -- exact ties, threshold hits, NaN and infinite
lengths, zero / overflowing / NaN face-vector sums, rings of 0, steps that leave the float range -- next to every seam of the kernels'
indexing, and topologies a decode does not produce.  tests/test_mesh_cases.py asserts, on the CPU, that the cases contain what they are
built for.

The reference of every comparison is a NumPy restatement applied to the CRAFTED arrays, never to a download.  Everything is compared bit for
bit (+0 is not -0).  The one exception: where the restatement holds a NaN that the arithmetic PRODUCED (a normal, a smoothed position),
the device must hold a NaN; its sign and payload are not compared -- x86 makes 0xFFC00000, the GPU 0x7FC00000, and the definitions do not
say.  A NaN that is merely copied (the vertices of a mesh, a cloud) keeps its bits and is compared exactly."""
import numpy as np
import pytest

import mesh_cases as MC
from conftest import pkg
from dense_planes import check_put, dense_layout, put_dense
from mesh_components_reference import np_filtered, np_labels
from mesh_normals_reference import np_normals
from mesh_reference import check_faces, np_mesh
from mesh_smooth_reference import np_smooth
from test_gpu_mesh import _synth_scanner

pytestmark = pytest.mark.gpu

INF = float("inf")


def _context(shape, V=1):
    """a context of the shape behind one run over a small synthetic view: every buffer exists, nothing is pending"""
    S, syn = pkg("scanner"), pkg("synth")
    H, W = shape
    full = (max(W, 300), max(H, 300))
    sc = _synth_scanner(S, syn, W, H, 10, 2, V=V, PW=2048, PH=2048, full=full)
    sc.set_masks(np.ones((full[1], full[0]), np.uint8))
    for v in range(V):
        sc.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
    sc.run(0, V)
    sc.synchronize()
    return sc


def _smoothed(sc, max_edge, view, run):
    it, mu, flags = run
    return sc.mesh_smoothed(max_edge, view, iterations=it, lam=MC.LAMBDA, mu=mu, fix_boundary=bool(flags & 1), normals=bool(flags & 2))


def _same_ints(got, want, tag):
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), tag


def _same_floats(got, want, tag, produced=False):
    n = MC.bits_differ(got, want, produced)
    assert n == 0, (tag, f"{n} of {want.size} values differ")


def check_view(sc, view, name, xyz, valid, max_edge, count):
    """every device result of one view at one max_edge against the restatements of the crafted arrays; returns the device results"""
    tag = (name, max_edge)
    verts, faces = np_mesh(xyz, valid, max_edge)
    out = {}
    gv, gf = out["mesh"] = sc.mesh(max_edge, view)
    _same_floats(gv, verts, tag + ("vertices",))
    _same_ints(gf, faces, tag + ("faces",))
    check_faces(gf, valid, len(gv))
    out["normals"] = sc.mesh_normals(max_edge, view)
    _same_floats(out["normals"], np_normals(verts, faces), tag + ("normals",), produced=True)
    lab = np_labels(len(verts), faces)
    out["labels"] = sc.mesh_components(max_edge, view)
    _same_ints(out["labels"], lab, tag + ("labels",))
    _, _, nv, nc = sc.mesh_components_device(max_edge, view, 1)
    assert (nv[0], nc[0]) == (len(verts), len(np.unique(lab))), tag + ("component count",)
    s = MC.second_largest(lab)
    for min_vertices in (1, 2, s, s + 1):
        want = np_filtered(verts, faces, min_vertices)
        got = out["filtered", min_vertices] = sc.mesh_filtered(max_edge, min_vertices, view)
        _same_floats(got[0], want[0], tag + ("filtered vertices", min_vertices))
        _same_ints(got[1], want[1], tag + ("filtered faces", min_vertices))
        _same_ints(got[2], want[2], tag + ("filtered ids", min_vertices))
    for run in MC.SMOOTH_RUNS:
        want = np_smooth(verts, faces, run[0], MC.LAMBDA, run[1], run[2])
        got = out["smoothed", run] = _smoothed(sc, max_edge, view, run)
        if run[2] & 2:
            _same_floats(got[0], want[0], tag + ("smoothed", run), produced=True)
            _same_floats(got[1], want[1], tag + ("normals of the smoothed", run), produced=True)
        else:
            _same_floats(got, want, tag + ("smoothed", run), produced=True)
    count[0] += 1
    count[1] += 5 + 3 * 4 + len(MC.SMOOTH_RUNS) + 1
    return out


def _flat(results):
    """the arrays of check_view's results, in a fixed order"""
    for key in sorted(results, key=repr):
        r = results[key]
        yield from ((key, a) for a in (r if isinstance(r, tuple) else (r,)))


def _identical(a, b, tag):
    for (ka, x), (kb, y) in zip(_flat(a), _flat(b)):
        assert ka == kb and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, ka)


@pytest.mark.parametrize("shape", MC.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crafted_cases(shape):
    count = [0, 0]
    results = {}
    with _context(shape) as sc:
        for name, xyz, valid, edges in MC.cases_of(shape):
            put_dense(sc, 0, xyz, valid, **MC.padding_of(name))
            check_put(sc, 0, xyz, valid)
            for max_edge in edges:
                if name.startswith("swapped"):                 # (before the restatement, which would only say that the faces differ)
                    cells = MC.swapped_cells(shape)
                    took_bd = MC.swapped_took_bd(sc.mesh(max_edge)[1], valid, cells)
                    print(f"{name}: {took_bd} of {len(cells)} swapped cells took the diagonal b-d")
                    assert took_bd == 0, f"{took_bd} of {len(cells)} swapped cells took the diagonal b-d: a product was fused into the add"
                r = results[name, max_edge] = check_view(sc, 0, name, xyz, valid, max_edge, count)
                # ---- properties beside the restatement ----
                if name.startswith("checkerboard"):
                    verts = xyz[valid == 1]
                    assert np.array_equal(r["labels"], np.arange(len(verts), dtype=np.int32)) and len(r["mesh"][1]) == 0
                    assert not r["normals"].view(np.uint32).any()                            # all +0
                    for run in MC.SMOOTH_RUNS:
                        got = r["smoothed", run]
                        pos, nrm = got if run[2] & 2 else (got, None)
                        assert np.array_equal(pos.view(np.uint32), verts.view(np.uint32))     # a ring of 0: bitwise the input
                        assert nrm is None or not nrm.view(np.uint32).any()
            if name.endswith("garbage"):                                                       # what the kernels must not look at changed nothing
                clean = name[:-len("garbage")] + "clean"
                for max_edge in edges:
                    _identical(results[name, max_edge], results[clean, max_edge], (name, max_edge))
    print(f"{shape[0]}x{shape[1]}: {len(MC.cases_of(shape))} cases, {count[0]} (case, max_edge) pairs, {count[1]} comparisons with a restatement")
    assert count[0] > 0


def test_put_dense_leaves_the_padding_alone_unless_asked():
    """the helper itself: a put without a fill keeps the padding columns, one with a fill sets exactly them"""
    shape = (3, 5)
    name, xyz, valid, _ = MC.nonfinite_cases(shape)[1]
    with _context(shape) as sc:
        p_addr, p_pitch, v_addr, v_pitch, pitch = dense_layout(sc, 0)
        rows = np.empty((shape[0], pitch), np.uint8)

        def padding():
            for r in range(shape[0]):
                sc._d2h(rows[r], v_addr + r * v_pitch)
            return rows[:, shape[1]:].copy()

        assert pitch == 16 and not padding().any()                                          # as the context leaves it
        put_dense(sc, 0, xyz, valid, **MC.PADDING)
        check_put(sc, 0, xyz, valid)
        assert (padding() == 1).all()
        put_dense(sc, 0, xyz, 1 - valid)
        check_put(sc, 0, xyz, 1 - valid)
        assert (padding() == 1).all()
        put_dense(sc, 0, xyz, valid, pad_valid=0)
        assert not padding().any()


def test_batches_over_injected_views():
    """Three different cases in views 0..2 of one context: the batched calls over (0, 3) and (1, 2) give the per-view results, which are
    the restatements' -- the view strides of the injected planes and of every output."""
    shape = (3, 1025)
    cases = [MC.integer_cases(shape)[1], MC.nonfinite_cases(shape)[1], MC.swapped_cases(shape)[0]]
    assert [c[0].split("-")[0] for c in cases] == ["integers", "nonfinite", "swapped"] and cases[1][0].endswith("garbage")
    count = [0, 0]
    with _context(shape, V=3) as sc:
        for v, (name, xyz, valid, _) in enumerate(cases):
            put_dense(sc, v, xyz, valid, **MC.padding_of(name))
        for v, (name, xyz, valid, _) in enumerate(cases):                                      # (behind all three puts: no put touched a neighbour)
            check_put(sc, v, xyz, valid)
        for max_edge in (2.0, INF):
            single = [check_view(sc, v, name, xyz, valid, max_edge, count) for v, (name, xyz, valid, _) in enumerate(cases)]
            assert len({len(r["mesh"][1]) for r in single}) == 3                               # the views differ
            s = 4
            for first, n in ((0, 3), (1, 2)):
                tag = (max_edge, first, n)
                want = single[first:first + n]
                got = sc.meshes(max_edge, first, n)
                nrm = sc.meshes_normals(max_edge, first, n)
                lab = sc.meshes_components(max_edge, first, n)
                fil = sc.meshes_filtered(max_edge, s, first, n)
                assert len(got) == len(nrm) == len(lab) == len(fil) == n
                for k in range(n):
                    _identical({"mesh": got[k], "normals": nrm[k], "labels": lab[k]},
                               {key: want[k][key] for key in ("mesh", "normals", "labels")}, tag + (k,))
                    w = sc.mesh_filtered(max_edge, s, first + k)
                    _identical({"filtered": fil[k]}, {"filtered": w}, tag + (k, "filtered"))
                    ref = np_filtered(*np_mesh(cases[first + k][1], cases[first + k][2], max_edge), s)
                    _same_floats(w[0], ref[0], tag + (k,))
                    _same_ints(w[1], ref[1], tag + (k,))
                    _same_ints(w[2], ref[2], tag + (k,))
                for run in MC.SMOOTH_RUNS:
                    it, mu, flags = run
                    sm = sc.meshes_smoothed(max_edge, first, n, iterations=it, lam=MC.LAMBDA, mu=mu, fix_boundary=bool(flags & 1), normals=bool(flags & 2))
                    assert len(sm) == n
                    for k in range(n):
                        _identical({"smoothed": sm[k]}, {"smoothed": want[k]["smoothed", run]}, tag + (k, run))
    assert count[0] == 6
