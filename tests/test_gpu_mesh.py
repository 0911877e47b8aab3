"""GPU tests (-m gpu) of the mesh stage (sl3d_mesh_views / sl3d_get_meshes; 3dscan_amd/csrc/sl3d_mesh.h, sl3d_mesh.hip).  The reference is
the NumPy restatement of the definition (tests/mesh_reference.py; pinned to constants by tests/test_mesh_arith.py) applied to what
Scanner.points() returned for that very context: every comparison is exact -- vertices bit for bit, faces id for id, in order."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_calibration, load_golden, pkg
from mesh_reference import check_faces, np_mesh
from test_meshio import read_ply

pytestmark = pytest.mark.gpu

INF = float("inf")
SL3D_E_INVALID_ARG = -1


def _same_mesh(got, want, tag):
    (gv, gf), (wv, wf) = got, want
    assert gv.dtype == np.float32 and gf.dtype == np.int32, tag
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), tag
    assert gf.shape == wf.shape and np.array_equal(gf, wf), tag


def _check_view(sc, max_edge, view=0, stats=None, tag=None):
    """the device's mesh of one view == the restatement on the device's own dense result; returns the mesh"""
    xyz, valid = sc.points(view)
    want = np_mesh(xyz, valid, max_edge, stats)
    got = sc.mesh(max_edge, view)
    _same_mesh(got, want, (tag, view, max_edge))
    check_faces(got[1], valid, len(got[0]))
    return got


def _edge_from_percentile(sc, view, pct):
    """a max_edge from the restatement's own edge lengths: the pct-th percentile of len2 over the candidates' edges"""
    st = {}
    xyz, valid = sc.points(view)
    np_mesh(xyz, valid, INF, st)
    l2 = st["len2"][np.isfinite(st["len2"])]
    assert len(l2) > 0
    return float(np.float32(np.sqrt(np.percentile(l2, pct))))


def _synth_scanner(S, syn, W, H, N, fw, V=1, PW=None, PH=None, keep=False, full=None, origin=(0, 0)):
    PW, PH = PW or W, PH or H
    FW, FH = full if full else (W, H)
    sc = S.Scanner(W, H, PW, PH, N, N, fw, fw, max_views=V, keep_stages=keep, full_size=full, origin=origin)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(FW, FH, PW, PH)))
    return sc


def _lasso(W, H, share=358580.0 / 1920000.0, dx=0, dy=0):
    """a rectangle of about a fifth of the frame (the share the reference's real captures select)"""
    mh, mw = int(round(H * share ** 0.5)), int(round(W * share ** 0.5))
    m = np.zeros((H, W), np.uint8)
    y0, x0 = (H - mh) // 2 + dy, (W - mw) // 2 + dx
    m[y0:y0 + mh, x0:x0 + mw] = 1
    return m


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
            st = {}
            verts, faces = _check_view(sc, max_edge, stats=st, tag=name)
            assert len(verts) == int((g["valid"] == 1).sum()) and len(faces) > 0
            assert st["diag_ae"] > 0 and st["diag_bd"] > 0 and st["three"] > 0
            if max_edge < INF:
                assert 0 < st["rejected"] < st["candidates"]
            else:
                assert len(faces) == st["candidates"]


# ---- 2. 1920x1080 synthetic views ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", ["default", "lasso"])
def test_1080p(selection):
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw = 1920, 1080, 10, 2
    mask = syn.default_mask(W, H) if selection == "default" else _lasso(W, H)
    with _synth_scanner(S, syn, W, H, N, fw) as sc:
        sc.set_mask(mask)
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        if selection == "lasso":
            assert 0.15 < sc.points()[1].mean() < 0.25
        max_edge = _edge_from_percentile(sc, 0, 80)
        st = {}
        verts, faces = _check_view(sc, max_edge, stats=st, tag=selection)
        rejected = st["rejected"] / st["candidates"]
        print(f"{selection}: max_edge {max_edge:.6g} mm, {len(verts)} vertices, {len(faces)} faces, {100 * rejected:.1f} % of the candidates rejected")
        assert 0.05 < rejected < 0.95
        assert np.array_equal(verts, sc.cloud())
        verts, faces = _check_view(sc, INF, stats=st, tag=selection)
        assert len(faces) == st["candidates"] and np.array_equal(verts, sc.cloud())


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------------
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
                verts, faces = _check_view(sc, max_edge, tag=(W, H, p))
                assert len(faces) > 0
            # a face across the chunk seam: a vertex left and one right of column 1024 (the frame's last column is never valid, so only
            # where column 1024 is not the last; a full selection, so that the pixels at the seam are valid)
            if W > 1025 and p == 1.0:
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
        verts, faces = _check_view(sc, INF, tag=(W, H))
        assert faces.shape == (0, 3) and len(verts) == int(sc.points()[1].sum())


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
            assert len(_check_view(sc, max_edge, tag="window")[1]) > 0
        sc.set_mask(np.zeros((FH, FW), np.uint8))
        sc.run()
        assert sc.points()[1].sum() == 0
        verts, faces = _check_view(sc, INF, tag="empty")
        assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------
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
        max_edge = _edge_from_percentile(sc, 0, 80)
        single = [sc.mesh(max_edge, v) for v in range(V)]
        assert len({len(f) for _, f in single}) > 3                       # the views differ
        for v in (0, 1, 2, V - 1):
            _same_mesh(single[v], np_mesh(*sc.points(v), max_edge), v)
        for first, n in ((0, 1), (5, 3), (0, 16), (13, 3)):
            got = sc.meshes(max_edge, first, n)
            assert len(got) == n
            for k in range(n):
                _same_mesh(got[k], single[first + k], (first, n, k))
        # the device-resident form: addresses, strides and counts describe the same meshes
        m, nv, nf = sc.mesh_device(max_edge, 2, 3)
        assert m.view_stride_faces == 2 * (W - 1) * (H - 1) and m.view_stride_points >= W * H
        for k in range(3):
            xyz, faces = np.empty((nv[k], 3), np.float32), np.empty((nf[k], 3), np.int32)
            sc._d2h(xyz, m.xyz + 12 * k * m.view_stride_points)
            sc._d2h(faces, m.faces + 12 * k * m.view_stride_faces)
            _same_mesh((xyz, faces), single[2 + k], ("device", k))


# ---- 5. repeatability, no side effects, launch lanes ------------------------------------------------------------------------------------
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
        a = sc.meshes(max_edge, 0, V)
        b = sc.meshes(max_edge, 0, V)
        for v in range(V):
            assert a[v][0].tobytes() == b[v][0].tobytes() and a[v][1].tobytes() == b[v][1].tobytes()
            xyz, valid = sc.points(v)
            assert np.array_equal(valid, before[v][1]) and np.array_equal(xyz.view(np.uint32), before[v][0].view(np.uint32))
        assert np.array_equal(sc.cloud(0), cloud0) and sc.compact_views(0, V) == counts
        assert [len(x) for x, _ in a] == counts


def test_after_a_series_of_one_view_launches():
    """30 one-view launches over three views put the launch lanes to use; the mesh call joins them and sees the LAST launches' results."""
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 3
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
        for v in range(V):
            sc.set_mask(syn.default_mask(W, H), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        old = sc.meshes(max_edge, 0, V)
        lassos = [_lasso(W, H, dx=40 * v - 40, dy=10 * v) for v in range(V)]
        sc.set_masks(np.stack(lassos))
        sc.synchronize()
        for i in range(30):
            sc.run(i % V, 1)
        assert sc.launch_counts()[1] > 0
        got = sc.meshes(max_edge, 0, V)                                    # (the first call behind the series: it has to join the lanes)
        for v in range(V):
            xyz, valid = sc.points(v)
            assert valid.sum() > 0 and not valid[lassos[v] == 0].any()     # the launches behind the new masks, not the run before them
            _same_mesh(got[v], np_mesh(xyz, valid, max_edge), ("lanes", v))
            assert len(got[v][1]) < len(old[v][1])


# ---- 6. sl3d_get_meshes' capacities, the error contract ---------------------------------------------------------------------------------
def _get_meshes(sc, first, n, max_edge, vcap, fcap, want_xyz=True, want_faces=True, counts=True):
    nv, nf = (C.c_int64 * n)(*([-7] * n)), (C.c_int64 * n)(*([-7] * n))
    xyz = np.full((max(vcap, 0) + 1, 3), -1.0, np.float32)              # one guard row each
    faces = np.full((max(fcap, 0) + 1, 3), -1, np.int32)
    rc = sc.L.sl3d_get_meshes(sc._h, first, n, C.c_float(max_edge), xyz.ctypes.data if want_xyz else None, vcap,
                              faces.ctypes.data if want_faces else None, fcap, nv if counts else None, nf if counts else None)
    return rc, xyz, faces, list(nv), list(nf)


def test_capacities_and_errors():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 322, 181, 8, 2, 3
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=512, PH=512) as sc:
        for v in range(V):
            sc.set_mask(_lasso(W, H, share=0.5, dx=5 * v), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        want = sc.meshes(max_edge, 0, V)
        for v in range(V):
            _same_mesh(want[v], np_mesh(*sc.points(v), max_edge), v)
        allv, allf = np.concatenate([x for x, _ in want]), np.concatenate([f for _, f in want])
        tv, tf = len(allv), len(allf)
        assert tv > 0 and tf > 0
        for vcap, fcap in ((0, 0), (tv // 2, tf // 3), (len(want[0][0]) + 1, len(want[0][1]) + 1), (tv, tf), (tv + 100, tf + 100)):
            rc, xyz, faces, nv, nf = _get_meshes(sc, 0, V, max_edge, vcap, fcap)
            assert rc == 0 and nv == [len(x) for x, _ in want] and nf == [len(f) for _, f in want]
            kv, kf = min(vcap, tv), min(fcap, tf)
            assert np.array_equal(xyz[:kv], allv[:kv]) and (xyz[kv:] == -1.0).all()       # nothing beyond the capacity / the total
            assert np.array_equal(faces[:kf], allf[:kf]) and (faces[kf:] == -1).all()
        for wx, wf in ((False, True), (True, False), (False, False)):
            rc, xyz, faces, nv, nf = _get_meshes(sc, 0, V, max_edge, tv, tf, want_xyz=wx, want_faces=wf)
            assert rc == 0 and sum(nv) == tv and sum(nf) == tf
            assert np.array_equal(xyz[:tv], allv) == wx and np.array_equal(faces[:tf], allf) == wf
        # refused calls: SL3D_E_INVALID_ARG, a text in last_error, and the device mesh of the call before them intact
        m, nv0, nf0 = sc.mesh_device(max_edge, 0, V)

        def device_mesh():
            out = []
            for k in range(V):
                xyz, faces = np.empty((nv0[k], 3), np.float32), np.empty((nf0[k], 3), np.int32)
                sc._d2h(xyz, m.xyz + 12 * k * m.view_stride_points)
                sc._d2h(faces, m.faces + 12 * k * m.view_stride_faces)
                out.append((xyz, faces))
            return out

        for k in range(V):
            _same_mesh(device_mesh()[k], want[k], k)
        nv, nf = (C.c_int64 * V)(), (C.c_int64 * V)()
        dm = S.Mesh()
        refused = [lambda e=e: sc.L.sl3d_mesh_views(sc._h, 0, V, C.c_float(e), C.byref(dm), nv, nf) for e in (float("nan"), 0.0, -0.0, -1.0, -INF)]
        refused += [lambda: sc.L.sl3d_mesh_views(sc._h, -1, 1, C.c_float(1.0), C.byref(dm), nv, nf),
                    lambda: sc.L.sl3d_mesh_views(sc._h, 0, V + 1, C.c_float(1.0), C.byref(dm), nv, nf),
                    lambda: sc.L.sl3d_mesh_views(sc._h, 1, 0, C.c_float(1.0), C.byref(dm), nv, nf),
                    lambda: sc.L.sl3d_mesh_views(sc._h, V, 1, C.c_float(1.0), C.byref(dm), nv, nf),
                    lambda: sc.L.sl3d_mesh_views(sc._h, 0, V, C.c_float(1.0), C.byref(dm), None, nf),
                    lambda: sc.L.sl3d_mesh_views(sc._h, 0, V, C.c_float(1.0), C.byref(dm), nv, None),
                    lambda: _get_meshes(sc, 0, V, float("nan"), tv, tf)[0],
                    lambda: _get_meshes(sc, 0, V, -2.0, tv, tf)[0],
                    lambda: _get_meshes(sc, 2, V, 1.0, tv, tf)[0],
                    lambda: _get_meshes(sc, 0, V, 1.0, tv, tf, counts=False)[0]]
        for i, call in enumerate(refused):
            sc.synchronize()                                                # (a successful call in between: the text below is the refusal's)
            assert call() == SL3D_E_INVALID_ARG, i
            assert len(sc.L.sl3d_last_error(sc._h)) > 0, i
            for k in range(V):
                _same_mesh(device_mesh()[k], want[k], (i, k))
        with pytest.raises(S.Sl3dError):
            sc.mesh(0.0)


# ---- 7. a textured mesh as a PLY file -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_of_a_gpu_mesh_with_colours(tmp_path, binary):
    S, syn, io = pkg("scanner"), pkg("synth"), pkg("meshio")
    W, H, N, fw = 322, 181, 8, 2
    rng = np.random.default_rng(1)
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.4))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        bgr = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
        sc.set_texture(bgr)
        cloud, rgb = sc.cloud_rgb()
        verts, faces = sc.mesh(_edge_from_percentile(sc, 0, 80))
        assert len(faces) > 0 and np.array_equal(verts.view(np.uint32), cloud.view(np.uint32))   # same order: the colours belong to the vertices
        assert np.array_equal(rgb, bgr[sc.points()[1] == 1][:, ::-1])
        path = str(tmp_path / "mesh.ply")
        io.write_ply(path, verts, faces=faces, rgb=rgb, binary=binary)
        fmt, gx, gc, gf, _ = read_ply(path)
        assert np.array_equal(gx.view(np.uint32), verts.view(np.uint32)) and np.array_equal(gc, rgb) and np.array_equal(gf, faces)
