"""GPU tests (-m gpu) of the mesh components and the filtered mesh (sl3d_mesh_components / sl3d_mesh_views_filtered and their host forms;
3dscan_amd/csrc/sl3d_mesh_components.h, sl3d_mesh_components.hip).  The reference is the NumPy restatement of the definition
(tests/mesh_components_reference.py over tests/mesh_reference.py; both pinned to constants by their arith tests) applied to what
Scanner.points() returned for that very context: every comparison is exact -- labels id for id, vertices bit for bit, faces id for id,
in order."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_calibration, load_golden, pkg
from mesh_components_reference import component_sizes, np_filtered, np_labels, serpentine
from mesh_reference import np_mesh
from test_gpu_mesh import _edge_from_percentile, _lasso, _synth_scanner
from test_meshio_normals import read_ply

pytestmark = pytest.mark.gpu

INF = float("inf")
SL3D_E_INVALID_ARG = -1


def _same_filtered(got, want, tag):
    (gv, gf, gi), (wv, wf, wi) = got, want
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gi.dtype == np.int32, tag
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), tag
    assert gf.shape == wf.shape and np.array_equal(gf, wf), tag
    assert gi.shape == wi.shape and np.array_equal(gi, wi), tag


def _check_view(sc, max_edge, mins, view=0, tag=None):
    """labels, n_components and the filtered meshes of one view == the restatement on the device's own dense result; returns
    (labels, (roots, sizes), verts, faces)"""
    xyz, valid = sc.points(view)
    verts, faces = np_mesh(xyz, valid, max_edge)
    want = np_labels(len(verts), faces)
    got = sc.mesh_components(max_edge, view)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (tag, view, max_edge)
    assert np.array_equal(got[got], got) and (got <= np.arange(len(got))).all()
    _, _, nv, nc = sc.mesh_components_device(max_edge, view, 1)
    assert nv == [len(verts)] and nc == [int((want == np.arange(len(want))).sum())], (tag, view, max_edge)
    for m in mins:
        _same_filtered(sc.mesh_filtered(max_edge, m, view), np_filtered(verts, faces, m), (tag, view, max_edge, m))
    return got, component_sizes(want), verts, faces


# ---- 1. the real crops, as windows of the 1600x1200 frame ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real_edge", "real_inside"])
@pytest.mark.parametrize("keep", [False, True])
def test_real_crops(name, keep):
    S = pkg("scanner")
    g = load_golden(name)
    cal, dims = golden_calibration()
    H, W = g["mask"].shape
    x0, y0 = [int(v) for v in g["origin"]]
    N_v, N_h, fw_v, fw_h, nc_v, nc_h = [int(v) for v in g["params"]]
    full = np.zeros((dims["H"], dims["W"]), np.uint8)
    full[y0 - 2:y0 + H + 2, x0 - 2:x0 + W + 2] = g["mask_halo2"]
    with S.Scanner(W, H, dims["PW"], dims["PH"], N_v, N_h, fw_v, fw_h, n_codes_v=nc_v, n_codes_h=nc_h, keep_stages=keep,
                   full_size=(dims["W"], dims["H"]), origin=(x0, y0)) as sc:
        sc.set_calibration(*cal)
        sc.set_mask(full)
        sc.set_frames(0, list(g["fringe_v"]) + list(g["gray_v"]) + list(g["inv_v"]))
        sc.set_frames(1, list(g["fringe_h"]) + list(g["gray_h"]) + list(g["inv_h"]))
        sc.run()
        assert np.array_equal(sc.points()[1], g["valid"])
        for max_edge in (0.25, 1.0, INF):
            lab, (roots, sizes), verts, faces = _check_view(sc, max_edge, (1, 2, 16, 100, 10 ** 6), tag=name)
            assert len(lab) == int((g["valid"] == 1).sum())
            assert (len(roots) == 1) == (max_edge == INF)
            one = sc.mesh_filtered(max_edge, 1)
            mesh = sc.mesh(max_edge)
            assert np.array_equal(one[0].view(np.uint32), mesh[0].view(np.uint32)) and np.array_equal(one[1], mesh[1])
            assert np.array_equal(one[2], np.arange(len(lab)))
            none = sc.mesh_filtered(max_edge, 10 ** 6)
            assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2].shape == (0,)


# ---- 2. islands: every size in turn --------------------------------------------------------------------------------------------------
ISLANDS = [(10, 10, 6, 6), (10, 30, 9, 12), (10, 60, 20, 17), (40, 20, 33, 25), (10, 100, 50, 40), (90, 10, 80, 60), (10, 160, 70, 130),
           (150, 320, 200, 300)]  # (row, column, rows, columns)


def test_islands():
    S, syn = pkg("scanner"), pkg("synth")
    W, H = 640, 360
    mask = np.zeros((H, W), np.uint8)
    for y, x, h, w in ISLANDS:
        mask[y:y + h, x:x + w] = 1
    with _synth_scanner(S, syn, W, H, 9, 2, PW=1024, PH=1024) as sc:
        sc.set_mask(mask)
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        lab, (roots, sizes), verts, faces = _check_view(sc, INF, (), tag="islands")
        big = np.sort(sizes[sizes >= 2])
        assert len(big) == 8 and len(set(big.tolist())) == 8                  # the restatement: eight islands of distinct sizes
        for i, s in enumerate(big.tolist()):
            for m, kept in ((s, 8 - i), (s + 1, 7 - i)):
                got = sc.mesh_filtered(INF, m)
                _same_filtered(got, np_filtered(verts, faces, m), ("islands", m))
                assert len(np.unique(lab[got[2]])) == kept


# ---- 3. serpentines: the minimum label travels the whole length of one component ---------------------------------------------------
@pytest.mark.parametrize("vertical", [False, True])
def test_serpentine(vertical):
    S, syn = pkg("scanner"), pkg("synth")
    if vertical:
        W, H, full, origin, PW = 70, 1500, (640, 1500), (200, 0), 1024
    else:
        W, H, full, origin, PW = 2049, 33, (2049, 576), (0, 300), 2048
    mask = np.zeros((full[1], full[0]), np.uint8)
    mask[origin[1]:origin[1] + H, origin[0]:origin[0] + W] = serpentine(H, W, 5, 3, vertical=vertical)
    with _synth_scanner(S, syn, W, H, 10, 2, PW=PW, PH=2048, full=full, origin=origin) as sc:
        sc.set_mask(mask)
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        lab, (roots, sizes), verts, faces = _check_view(sc, INF, (2,), tag=("serpentine", vertical))
        print(f"serpentine {W} x {H}: {len(lab)} vertices, {len(roots)} components, the largest {sizes.max()}")
        assert len(lab) > 0.3 * W * H and sizes.max() >= 0.9 * len(lab)           # one snake through the whole window
        pix = np.flatnonzero(sc.points()[1].ravel() == 1)[lab == roots[np.argmax(sizes)]]
        assert (pix // W).max() - (pix // W).min() >= 0.7 * H and (pix % W).max() - (pix % W).min() >= 0.7 * W


# ---- 4. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1021, 9), (1025, 9), (2049, 9), (1027, 2)])
def test_widths_off_the_quad_the_pitch_and_the_chunk(W, H):
    S, syn = pkg("scanner"), pkg("synth")
    rng = np.random.default_rng(W)
    FH, y0 = 576, 300                                                   # a thin window of a frame of ordinary proportions
    with _synth_scanner(S, syn, W, H, 10, 2, PW=2048, PH=2048, full=(W, FH), origin=(0, y0)) as sc:
        for p in (1.0, 0.6):
            sc.set_mask((rng.random((FH, W)) < p).astype(np.uint8))
            sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
            sc.run()
            for max_edge in (_edge_from_percentile(sc, 0, 80), INF):
                lab, (roots, sizes), verts, faces = _check_view(sc, max_edge, (2, 5), tag=(W, H, p))
                if max_edge < INF:
                    assert len(roots) > 20 and sizes.max() > 1                # many small components
            if W > 1025 and p == 1.0:                                        # a component across the chunk seam at column 1024
                pix = np.flatnonzero(sc.points()[1].ravel() == 1)
                cols = pix[faces] % W
                assert ((cols.min(axis=1) == 1023) & (cols.max(axis=1) == 1024)).any()


@pytest.mark.parametrize("W,H", [(300, 1), (1, 300)])
def test_one_row_and_one_column(W, H):
    S, syn = pkg("scanner"), pkg("synth")
    with _synth_scanner(S, syn, W, H, 8, 2, PW=512, PH=512, full=(300, 300), origin=(0 if W > 1 else 150, 0 if H > 1 else 150)) as sc:
        sc.set_mask(np.ones((300, 300), np.uint8))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=0)
        sc.run()
        lab, (roots, sizes), verts, faces = _check_view(sc, INF, (1, 2), tag=(W, H))
        assert len(lab) == int(sc.points()[1].sum()) > 0 and np.array_equal(lab, np.arange(len(lab)))   # every vertex a singleton
        assert sc.mesh_components_device(INF)[3] == [len(lab)]
        assert sc.mesh_filtered(INF, 2)[0].shape == (0, 3)


def test_window_with_an_origin_and_an_empty_selection():
    S, syn = pkg("scanner"), pkg("synth")
    FW, FH, W, H, x0, y0 = 640, 480, 333, 211, 101, 57
    with _synth_scanner(S, syn, W, H, 8, 4, PW=1024, PH=768, full=(FW, FH), origin=(x0, y0)) as sc:
        mask = syn.default_mask(FW, FH)
        mask[y0 + 40:y0 + 60, x0 + 100:x0 + 180] = 0
        sc.set_mask(mask)
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        assert sc.points()[1].mean() > 0.5
        for max_edge in (_edge_from_percentile(sc, 0, 80), INF):
            _check_view(sc, max_edge, (1, 3, 50), tag="window")
        sc.set_mask(np.zeros((FH, FW), np.uint8))
        sc.run()
        assert sc.points()[1].sum() == 0
        lab, _, _, _ = _check_view(sc, INF, (1, 2), tag="empty")
        assert lab.shape == (0,) and sc.mesh_components_device(INF)[2:] == ([0], [0])


# ---- 5. 1920x1080 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", ["default", "lasso"])
def test_1080p(selection):
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw = 1920, 1080, 10, 2
    mask = syn.default_mask(W, H) if selection == "default" else _lasso(W, H)
    with _synth_scanner(S, syn, W, H, N, fw) as sc:
        sc.set_mask(mask)
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        max_edge = _edge_from_percentile(sc, 0, 80)
        lab, (roots, sizes), verts, faces = _check_view(sc, max_edge, (), tag=selection)
        order = np.sort(sizes)[::-1]
        assert len(order) >= 2 and order[0] > order[1]
        m = int(order[1]) + 1
        got = sc.mesh_filtered(max_edge, m)
        _same_filtered(got, np_filtered(verts, faces, m), (selection, m))
        assert len(np.unique(lab[got[2]])) == 1 and len(got[0]) == order[0]    # exactly one component is kept
        print(f"{selection}: max_edge {max_edge:.6g} mm, {len(verts)} vertices, {len(faces)} faces, {len(roots)} components, "
              f"{int((sizes == 1).sum())} singletons, largest {order[:4].tolist()}; min_vertices {m} keeps {len(got[0])} vertices, {len(got[1])} faces")


# ---- 6. batches -----------------------------------------------------------------------------------------------------------------------
def test_batches_equal_one_view_calls():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 16
    rng = np.random.default_rng(16)
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
        for v in range(V):
            m = syn.default_mask(W, H) if v % 3 == 0 else _lasso(W, H, dx=7 * v - 50, dy=3 * v - 20) if v % 3 == 1 else (rng.random((H, W)) < 0.7).astype(np.uint8)
            sc.set_mask(m, view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=2)
        sc.run(0, V)
        max_edge, min_v = _edge_from_percentile(sc, 0, 80), 4
        labels = [sc.mesh_components(max_edge, v) for v in range(V)]
        filtered = [sc.mesh_filtered(max_edge, min_v, v) for v in range(V)]
        assert len({len(np.unique(l)) for l in labels}) > 3                      # the views differ
        for v in (0, 1, 2, V - 1):
            verts, faces = np_mesh(*sc.points(v), max_edge)
            assert np.array_equal(labels[v], np_labels(len(verts), faces))
            _same_filtered(filtered[v], np_filtered(verts, faces, min_v), v)
        for first, n in ((0, 1), (5, 3), (0, 16), (13, 3)):
            got_l, got_f = sc.meshes_components(max_edge, first, n), sc.meshes_filtered(max_edge, min_v, first, n)
            assert len(got_l) == len(got_f) == n
            for k in range(n):
                assert np.array_equal(got_l[k], labels[first + k]), (first, n, k)
                _same_filtered(got_f[k], filtered[first + k], (first, n, k))
        # the device-resident forms: addresses, strides and counts describe the same arrays
        dev, stride, nv, nc = sc.mesh_components_device(max_edge, 2, 3)
        assert stride >= W * H
        m, fv, ff = sc.mesh_filtered_device(max_edge, min_v, 2, 3)
        assert m.view_stride_faces == 2 * (W - 1) * (H - 1) and m.view_stride_points >= W * H
        for k in range(3):
            lab = np.empty(nv[k], np.int32)
            sc._d2h(lab, dev + 4 * k * stride)
            assert np.array_equal(lab, labels[2 + k]) and nc[k] == len(np.unique(lab))
            xyz, faces, ids = np.empty((fv[k], 3), np.float32), np.empty((ff[k], 3), np.int32), np.empty(fv[k], np.int32)
            sc._d2h(xyz, m.xyz + 12 * k * m.view_stride_points)
            sc._d2h(faces, m.faces + 12 * k * m.view_stride_faces)
            sc._d2h(ids, m.vertex_ids + 4 * k * m.view_stride_points)
            _same_filtered((xyz, faces, ids), filtered[2 + k], ("device", k))


# ---- 7. repeatability, no side effects, launch lanes ------------------------------------------------------------------------------------
def test_repeatable_and_without_side_effects():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 2
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
        for v in range(V):
            sc.set_mask(syn.default_mask(W, H), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        before = [sc.points(v) for v in range(V)]
        cloud0 = sc.cloud(0)
        counts = sc.compact_views(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        m, nv, nf = sc.mesh_device(max_edge, 0, V)
        ndev, nstride, _ = sc.mesh_normals_device(max_edge, 0, V)

        def device_state():
            out = []
            for k in range(V):
                xyz, faces, nrm = np.empty((nv[k], 3), np.float32), np.empty((nf[k], 3), np.int32), np.empty((nv[k], 3), np.float32)
                sc._d2h(xyz, m.xyz + 12 * k * m.view_stride_points)
                sc._d2h(faces, m.faces + 12 * k * m.view_stride_faces)
                sc._d2h(nrm, ndev + 12 * k * nstride)
                out.append(xyz.tobytes() + faces.tobytes() + nrm.tobytes())
            return out

        state = device_state()
        a = (sc.meshes_components(max_edge, 0, V), sc.meshes_filtered(max_edge, 5, 0, V))
        b = (sc.meshes_components(max_edge, 0, V), sc.meshes_filtered(max_edge, 5, 0, V))
        for v in range(V):
            assert a[0][v].tobytes() == b[0][v].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1][v], b[1][v]))
            assert 0 < len(a[1][v][0]) < len(a[0][v])
            xyz, valid = sc.points(v)
            assert np.array_equal(valid, before[v][1]) and np.array_equal(xyz.view(np.uint32), before[v][0].view(np.uint32))
        assert np.array_equal(sc.cloud(0), cloud0) and sc.compact_views(0, V) == counts
        assert [len(x) for x in a[0]] == counts
        assert device_state() == state


def test_after_a_series_of_one_view_launches():
    """30 one-view launches over three views put the launch lanes to use; the call joins them and sees the LAST launches' results."""
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 3
    for filtered in (False, True):
        with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
            for v in range(V):
                sc.set_mask(syn.default_mask(W, H), view=v)
                sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
            sc.run(0, V)
            max_edge = _edge_from_percentile(sc, 0, 80)
            old = sc.meshes_components(max_edge, 0, V)
            lassos = [_lasso(W, H, dx=40 * v - 40, dy=10 * v) for v in range(V)]
            sc.set_masks(np.stack(lassos))
            sc.synchronize()
            for i in range(30):
                sc.run(i % V, 1)
            assert sc.launch_counts()[1] > 0
            got = sc.meshes_filtered(max_edge, 3, 0, V) if filtered else sc.meshes_components(max_edge, 0, V)   # (has to join the lanes)
            for v in range(V):
                xyz, valid = sc.points(v)
                assert valid.sum() > 0 and not valid[lassos[v] == 0].any()     # the launches behind the new masks, not the run before them
                verts, faces = np_mesh(xyz, valid, max_edge)
                if filtered:
                    _same_filtered(got[v], np_filtered(verts, faces, 3), ("lanes", v))
                else:
                    assert np.array_equal(got[v], np_labels(len(verts), faces)) and len(got[v]) < len(old[v])


# ---- 8. the host forms' capacities, the error contract ---------------------------------------------------------------------------------
def _get_components(sc, first, n, max_edge, vcap, want_labels=True, counts=(True, True)):
    nv, nc = (C.c_int64 * n)(*([-7] * n)), (C.c_int64 * n)(*([-7] * n))
    labels = np.full(max(vcap, 0) + 1, -1, np.int32)                     # one guard row
    rc = sc.L.sl3d_get_mesh_components(sc._h, first, n, C.c_float(max_edge), labels.ctypes.data if want_labels else None, vcap,
                                       nv if counts[0] else None, nc if counts[1] else None)
    return rc, labels, list(nv), list(nc)


def _get_filtered(sc, first, n, max_edge, min_v, vcap, fcap, want=(True, True, True), counts=(True, True)):
    nv, nf = (C.c_int64 * n)(*([-7] * n)), (C.c_int64 * n)(*([-7] * n))
    xyz = np.full((max(vcap, 0) + 1, 3), -1.0, np.float32)              # one guard row each
    ids = np.full(max(vcap, 0) + 1, -1, np.int32)
    faces = np.full((max(fcap, 0) + 1, 3), -1, np.int32)
    rc = sc.L.sl3d_get_meshes_filtered(sc._h, first, n, C.c_float(max_edge), C.c_int64(min_v), xyz.ctypes.data if want[0] else None,
                                       ids.ctypes.data if want[1] else None, vcap, faces.ctypes.data if want[2] else None, fcap,
                                       nv if counts[0] else None, nf if counts[1] else None)
    return rc, xyz, ids, faces, list(nv), list(nf)


def test_capacities_and_errors():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V, min_v = 322, 181, 8, 2, 3, 3
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=512, PH=512) as sc:
        for v in range(V):
            sc.set_mask(_lasso(W, H, share=0.5, dx=5 * v), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        labels, want = sc.meshes_components(max_edge, 0, V), sc.meshes_filtered(max_edge, min_v, 0, V)
        for v in range(V):
            verts, faces = np_mesh(*sc.points(v), max_edge)
            assert np.array_equal(labels[v], np_labels(len(verts), faces))
            _same_filtered(want[v], np_filtered(verts, faces, min_v), v)
        alll = np.concatenate(labels)
        allv, allf, alli = (np.concatenate([w[j] for w in want]) for j in range(3))
        tl, tv, tf = len(alll), len(allv), len(allf)
        assert 0 < tv < tl and tf > 0
        n_comp = [len(np.unique(l)) for l in labels]
        for cap in (0, tl // 2, len(labels[0]) + 1, tl, tl + 100):
            rc, lab, nv, nc = _get_components(sc, 0, V, max_edge, cap)
            assert rc == 0 and nv == [len(l) for l in labels] and nc == n_comp
            k = min(cap, tl)
            assert np.array_equal(lab[:k], alll[:k]) and (lab[k:] == -1).all()           # nothing beyond the capacity / the total
        rc, lab, nv, nc = _get_components(sc, 0, V, max_edge, tl, want_labels=False)
        assert rc == 0 and sum(nv) == tl and (lab == -1).all()
        for vcap, fcap in ((0, 0), (tv // 2, tf // 3), (len(want[0][0]) + 1, len(want[0][1]) + 1), (tv, tf), (tv + 100, tf + 100)):
            rc, xyz, ids, faces, nv, nf = _get_filtered(sc, 0, V, max_edge, min_v, vcap, fcap)
            assert rc == 0 and nv == [len(w[0]) for w in want] and nf == [len(w[1]) for w in want]
            kv, kf = min(vcap, tv), min(fcap, tf)
            assert np.array_equal(xyz[:kv], allv[:kv]) and (xyz[kv:] == -1.0).all()
            assert np.array_equal(ids[:kv], alli[:kv]) and (ids[kv:] == -1).all()
            assert np.array_equal(faces[:kf], allf[:kf]) and (faces[kf:] == -1).all()
        for w in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            rc, xyz, ids, faces, nv, nf = _get_filtered(sc, 0, V, max_edge, min_v, tv, tf, want=w)
            assert rc == 0 and sum(nv) == tv and sum(nf) == tf
            assert (np.array_equal(xyz[:tv], allv), np.array_equal(ids[:tv], alli), np.array_equal(faces[:tf], allf)) == w
        # refused calls: SL3D_E_INVALID_ARG, a text in last_error, and the device results of the calls before them intact
        dev, stride, nv0, nc0 = sc.mesh_components_device(max_edge, 0, V)
        m, fv0, ff0 = sc.mesh_filtered_device(max_edge, min_v, 0, V)

        def device_results_intact(tag):
            for k in range(V):
                lab = np.empty(nv0[k], np.int32)
                sc._d2h(lab, dev + 4 * k * stride)
                assert np.array_equal(lab, labels[k]), tag
                xyz, faces, ids = np.empty((fv0[k], 3), np.float32), np.empty((ff0[k], 3), np.int32), np.empty(fv0[k], np.int32)
                sc._d2h(xyz, m.xyz + 12 * k * m.view_stride_points)
                sc._d2h(faces, m.faces + 12 * k * m.view_stride_faces)
                sc._d2h(ids, m.vertex_ids + 4 * k * m.view_stride_points)
                _same_filtered((xyz, faces, ids), want[k], tag)

        device_results_intact("before")
        nv, nn = (C.c_int64 * V)(), (C.c_int64 * V)()
        dl, ds, dm = C.c_void_p(), C.c_size_t(), S.MeshFiltered()
        comp = lambda first, n, e, a=nv, b=nn: sc.L.sl3d_mesh_components(sc._h, first, n, C.c_float(e), C.byref(dl), C.byref(ds), a, b)
        filt = lambda first, n, e, mv, a=nv, b=nn: sc.L.sl3d_mesh_views_filtered(sc._h, first, n, C.c_float(e), C.c_int64(mv), C.byref(dm), a, b)
        refused = [lambda e=e: comp(0, V, e) for e in (float("nan"), 0.0, -0.0, -1.0, -INF)]
        refused += [lambda e=e: filt(0, V, e, min_v) for e in (float("nan"), 0.0, -1.0)]
        refused += [lambda mv=mv: filt(0, V, 1.0, mv) for mv in (0, -1)]
        refused += [lambda: comp(-1, 1, 1.0), lambda: comp(0, V + 1, 1.0), lambda: comp(1, 0, 1.0), lambda: comp(V, 1, 1.0),
                    lambda: comp(0, V, 1.0, a=None), lambda: comp(0, V, 1.0, b=None),
                    lambda: filt(-1, 1, 1.0, 2), lambda: filt(0, V + 1, 1.0, 2), lambda: filt(0, V, 1.0, 2, a=None), lambda: filt(0, V, 1.0, 2, b=None),
                    lambda: _get_components(sc, 0, V, float("nan"), tl)[0], lambda: _get_components(sc, 2, V, 1.0, tl)[0],
                    lambda: _get_components(sc, 0, V, 1.0, tl, counts=(False, True))[0], lambda: _get_components(sc, 0, V, 1.0, tl, counts=(True, False))[0],
                    lambda: _get_filtered(sc, 0, V, -2.0, min_v, tv, tf)[0], lambda: _get_filtered(sc, 0, V, 1.0, 0, tv, tf)[0],
                    lambda: _get_filtered(sc, 0, V, 1.0, -1, tv, tf)[0], lambda: _get_filtered(sc, 2, V, 1.0, min_v, tv, tf)[0],
                    lambda: _get_filtered(sc, 0, V, 1.0, min_v, tv, tf, counts=(False, True))[0]]
        for i, call in enumerate(refused):
            sc.synchronize()                                                # (a successful call in between: the text below is the refusal's)
            assert call() == SL3D_E_INVALID_ARG, i
            assert len(sc.L.sl3d_last_error(sc._h)) > 0, i
            device_results_intact(i)
        with pytest.raises(S.Sl3dError):
            sc.mesh_components(0.0)
        with pytest.raises(S.Sl3dError):
            sc.mesh_filtered(1.0, 0)


# ---- 9. a filtered mesh with normals and colours as a PLY file ------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_of_a_filtered_mesh_with_normals_and_colours(tmp_path, binary):
    S, syn, io = pkg("scanner"), pkg("synth"), pkg("meshio")
    W, H, N, fw = 322, 181, 8, 2
    rng = np.random.default_rng(1)
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.4))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        sc.set_texture(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
        max_edge = _edge_from_percentile(sc, 0, 80)
        verts, faces, ids = sc.mesh_filtered(max_edge, 10)
        full_verts, full_faces = sc.mesh(max_edge)
        assert 0 < len(verts) < len(full_verts) and len(faces) > 0
        n, rgb = sc.mesh_normals(max_edge)[ids], sc.cloud_rgb()[1][ids]
        # the gathers are exact: the filtered mesh's own normals (every face of a kept vertex is kept) and its vertices
        assert np.array_equal(verts.view(np.uint32), full_verts[ids].view(np.uint32))
        assert np.array_equal(ids[faces], full_faces[np.isin(full_faces[:, 0], ids)])
        path = str(tmp_path / "filtered.ply")
        io.write_ply(path, verts, faces=faces, rgb=rgb, binary=binary, normals=n)
        fmt, gx, gn, gc, gf, _ = read_ply(path)
        assert np.array_equal(gx.view(np.uint32), verts.view(np.uint32)) and np.array_equal(gn.view(np.uint32), n.view(np.uint32))
        assert np.array_equal(gc, rgb) and np.array_equal(gf, faces)
