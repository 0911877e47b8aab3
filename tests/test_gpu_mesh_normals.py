"""GPU tests (-m gpu) of the vertex normals (sl3d_mesh_normals / sl3d_get_mesh_normals; 3dscan_amd/csrc/sl3d_mesh.h,
sl3d_mesh_normals.hip).  The reference is the NumPy restatement of the definition (tests/mesh_normals_reference.py; pinned to constants by
tests/test_mesh_normals_arith.py) applied to the (vertices, faces) Scanner.mesh returned for that very context and max_edge: every
comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_calibration, load_golden, pkg
from mesh_normals_reference import np_normals
from test_gpu_mesh import _edge_from_percentile, _lasso, _synth_scanner
from test_meshio_normals import read_ply

pytestmark = pytest.mark.gpu

INF = float("inf")
SL3D_E_INVALID_ARG = -1


def _same(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape, tag
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag


def _check_view(sc, max_edge, view=0, tag=None):
    """the device's normals of one view == the restatement on the device's own mesh; returns (normals, vertices, faces)"""
    verts, faces = sc.mesh(max_edge, view)
    got = sc.mesh_normals(max_edge, view)
    _same(got, np_normals(verts, faces), (tag, view, max_edge))
    return got, verts, faces


def _zero(n):
    return (n.view(np.uint32) == 0).all(axis=1)


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
        for max_edge in (0.25, 1.0, INF):
            n, verts, faces = _check_view(sc, max_edge, tag=name)
            assert len(n) == int((g["valid"] == 1).sum()) and len(faces) > 0
            z = _zero(n)
            assert (~z).any()
            if max_edge < INF:
                assert z.any()
            length = np.linalg.norm(n[~z].astype(np.float64), axis=1)
            assert np.abs(length - 1.0).max() <= 2e-7


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------
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
                n, verts, faces = _check_view(sc, max_edge, tag=(W, H, p))
                assert len(faces) > 0 and (~_zero(n)).any()
            # across the chunk seam: a vertex at column 1023 and one at 1024 share a face, and both carry a normal
            if W > 1025 and p == 1.0:
                pix = np.flatnonzero(sc.points()[1].ravel() == 1)
                cols = pix[faces] % W
                seam = faces[(cols.min(axis=1) == 1023) & (cols.max(axis=1) == 1024)]
                assert len(seam) > 0
                ids = seam.ravel()
                assert set(pix[ids] % W) == {1023, 1024} and not _zero(n[ids]).any()


@pytest.mark.parametrize("W,H", [(300, 1), (1, 300)])
def test_one_row_and_one_column(W, H):
    S, syn = pkg("scanner"), pkg("synth")
    with _synth_scanner(S, syn, W, H, 8, 2, PW=512, PH=512, full=(300, 300), origin=(0 if W > 1 else 150, 0 if H > 1 else 150)) as sc:
        sc.set_mask(np.ones((300, 300), np.uint8))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=0)
        sc.run()
        n, verts, faces = _check_view(sc, INF, tag=(W, H))
        assert len(n) == len(sc.cloud()) == int(sc.points()[1].sum()) > 0 and _zero(n).all()


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
            n, _, _ = _check_view(sc, max_edge, tag="window")
            assert (~_zero(n)).any()
        sc.set_mask(np.zeros((FH, FW), np.uint8))
        sc.run()
        assert sc.points()[1].sum() == 0
        n, _, _ = _check_view(sc, INF, tag="empty")
        assert n.shape == (0, 3)


# ---- 3. batches -----------------------------------------------------------------------------------------------------------------------
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
        single = [sc.mesh_normals(max_edge, v) for v in range(V)]
        assert len({len(n) for n in single}) > 3                          # the views differ
        for v in (0, 1, 2, V - 1):
            _same(single[v], np_normals(*sc.mesh(max_edge, v)), v)
        for first, n in ((0, 1), (5, 3), (0, 16), (13, 3)):
            got = sc.meshes_normals(max_edge, first, n)
            assert len(got) == n
            for k in range(n):
                _same(got[k], single[first + k], (first, n, k))
        # the device-resident form: address, stride and counts describe the same arrays
        dev, stride, nv = sc.mesh_normals_device(max_edge, 2, 3)
        assert stride >= W * H and nv == [len(single[2 + k]) for k in range(3)]
        for k in range(3):
            out = np.empty((nv[k], 3), np.float32)
            sc._d2h(out, dev + 12 * k * stride)
            _same(out, single[2 + k], ("device", k))


# ---- 4. repeatability, no side effects, launch lanes ------------------------------------------------------------------------------------
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
        want = sc.meshes(max_edge, 0, V)
        m, nv, nf = sc.mesh_device(max_edge, 0, V)                        # the device mesh a caller holds while it asks for the normals
        a = sc.meshes_normals(max_edge, 0, V)
        b = sc.meshes_normals(max_edge, 0, V)
        for v in range(V):
            assert a[v].tobytes() == b[v].tobytes() and len(a[v]) == counts[v]
            _same(a[v], np_normals(*want[v]), v)
            xyz, valid = sc.points(v)
            assert np.array_equal(valid, before[v][1]) and np.array_equal(xyz.view(np.uint32), before[v][0].view(np.uint32))
            dx, df = np.empty((nv[v], 3), np.float32), np.empty((nf[v], 3), np.int32)
            sc._d2h(dx, m.xyz + 12 * v * m.view_stride_points)
            sc._d2h(df, m.faces + 12 * v * m.view_stride_faces)
            assert np.array_equal(dx.view(np.uint32), want[v][0].view(np.uint32)) and np.array_equal(df, want[v][1])
        assert np.array_equal(sc.cloud(0), cloud0) and sc.compact_views(0, V) == counts


def test_after_a_series_of_one_view_launches():
    """30 one-view launches over three views put the launch lanes to use; the normals call joins them and sees the LAST launches' results."""
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 3
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
        for v in range(V):
            sc.set_mask(syn.default_mask(W, H), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        old = sc.meshes_normals(max_edge, 0, V)
        lassos = [_lasso(W, H, dx=40 * v - 40, dy=10 * v) for v in range(V)]
        sc.set_masks(np.stack(lassos))
        sc.synchronize()
        for i in range(30):
            sc.run(i % V, 1)
        assert sc.launch_counts()[1] > 0
        got = sc.meshes_normals(max_edge, 0, V)                            # (the first call behind the series: it has to join the lanes)
        for v in range(V):
            valid = sc.points(v)[1]
            assert valid.sum() > 0 and not valid[lassos[v] == 0].any()     # the launches behind the new masks, not the run before them
            _same(got[v], np_normals(*sc.mesh(max_edge, v)), ("lanes", v))
            assert len(got[v]) == int(valid.sum()) < len(old[v])


# ---- 5. sl3d_get_mesh_normals' capacities, the error contract -----------------------------------------------------------------------------
def _get_normals(sc, first, n, max_edge, cap, want=True, counts=True):
    nv = (C.c_int64 * n)(*([-7] * n))
    out = np.full((max(cap, 0) + 1, 3), -1.0, np.float32)               # one guard row
    rc = sc.L.sl3d_get_mesh_normals(sc._h, first, n, C.c_float(max_edge), out.ctypes.data if want else None, cap, nv if counts else None)
    return rc, out, list(nv)


def test_capacities_and_errors():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 322, 181, 8, 2, 3
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=512, PH=512) as sc:
        for v in range(V):
            sc.set_mask(_lasso(W, H, share=0.5, dx=5 * v), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        meshes = sc.meshes(max_edge, 0, V)
        want = [np_normals(x, f) for x, f in meshes]
        alln = np.concatenate(want)
        tv = len(alln)
        assert tv > 0 and (~_zero(alln)).any()
        for cap in (0, tv // 2, len(want[0]) + 1, tv, tv + 100):
            rc, out, nv = _get_normals(sc, 0, V, max_edge, cap)
            assert rc == 0 and nv == [len(x) for x in want]
            k = min(cap, tv)
            assert np.array_equal(out[:k].view(np.uint32), alln[:k].view(np.uint32)) and (out[k:] == -1.0).all()   # nothing beyond the capacity / the total
        rc, out, nv = _get_normals(sc, 0, V, max_edge, tv, want=False)
        assert rc == 0 and sum(nv) == tv and (out == -1.0).all()
        # refused calls: SL3D_E_INVALID_ARG, a text in last_error, and the device normals of the call before them intact
        dev, stride, nv0 = sc.mesh_normals_device(max_edge, 0, V)

        def device_normals():
            out = []
            for k in range(V):
                a = np.empty((nv0[k], 3), np.float32)
                sc._d2h(a, dev + 12 * k * stride)
                out.append(a)
            return out

        for k in range(V):
            _same(device_normals()[k], want[k], k)
        nv, dp, ds = (C.c_int64 * V)(), C.c_void_p(), C.c_size_t()
        refused = [lambda e=e: sc.L.sl3d_mesh_normals(sc._h, 0, V, C.c_float(e), C.byref(dp), C.byref(ds), nv) for e in (float("nan"), 0.0, -0.0, -1.0, -INF)]
        refused += [lambda: sc.L.sl3d_mesh_normals(sc._h, -1, 1, C.c_float(1.0), C.byref(dp), C.byref(ds), nv),
                    lambda: sc.L.sl3d_mesh_normals(sc._h, 0, V + 1, C.c_float(1.0), C.byref(dp), C.byref(ds), nv),
                    lambda: sc.L.sl3d_mesh_normals(sc._h, 1, 0, C.c_float(1.0), C.byref(dp), C.byref(ds), nv),
                    lambda: sc.L.sl3d_mesh_normals(sc._h, V, 1, C.c_float(1.0), C.byref(dp), C.byref(ds), nv),
                    lambda: sc.L.sl3d_mesh_normals(sc._h, 0, V, C.c_float(1.0), C.byref(dp), C.byref(ds), None),
                    lambda: _get_normals(sc, 0, V, float("nan"), tv)[0],
                    lambda: _get_normals(sc, 0, V, -2.0, tv)[0],
                    lambda: _get_normals(sc, 2, V, 1.0, tv)[0],
                    lambda: _get_normals(sc, 0, V, 1.0, tv, counts=False)[0]]
        for i, call in enumerate(refused):
            sc.synchronize()                                                # (a successful call in between: the text below is the refusal's)
            assert call() == SL3D_E_INVALID_ARG, i
            assert len(sc.L.sl3d_last_error(sc._h)) > 0, i
            for k in range(V):
                _same(device_normals()[k], want[k], (i, k))
        with pytest.raises(S.Sl3dError):
            sc.mesh_normals(0.0)


# ---- 6. a textured mesh with normals as a PLY file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_of_a_gpu_mesh_with_normals_and_colours(tmp_path, binary):
    S, syn, io = pkg("scanner"), pkg("synth"), pkg("meshio")
    W, H, N, fw = 322, 181, 8, 2
    rng = np.random.default_rng(1)
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.4))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        sc.set_texture(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
        cloud, rgb = sc.cloud_rgb()
        max_edge = _edge_from_percentile(sc, 0, 80)
        verts, faces = sc.mesh(max_edge)
        n = sc.mesh_normals(max_edge)
        assert len(faces) > 0 and np.array_equal(verts.view(np.uint32), cloud.view(np.uint32)) and (~_zero(n)).any()
        path = str(tmp_path / "mesh.ply")
        io.write_ply(path, verts, faces=faces, rgb=rgb, binary=binary, normals=n)
        fmt, gx, gn, gc, gf, _ = read_ply(path)
        assert np.array_equal(gx.view(np.uint32), verts.view(np.uint32)) and np.array_equal(gn.view(np.uint32), n.view(np.uint32))
        assert np.array_equal(gc, rgb) and np.array_equal(gf, faces)
