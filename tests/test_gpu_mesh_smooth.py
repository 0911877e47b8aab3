"""GPU tests (-m gpu) of the smoothing stage (sl3d_mesh_smooth / sl3d_get_mesh_smoothed; 3dscan_amd/csrc/sl3d_mesh_smooth.h,
sl3d_mesh_smooth.hip).  The reference is the NumPy restatement of the definition (tests/mesh_smooth_reference.py; pinned to constants by
tests/test_mesh_smooth_arith.py) applied to the (vertices, faces) Scanner.mesh returned for that very context and max_edge; the normals
are np_normals(smoothed, faces) of tests/mesh_normals_reference.py.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_calibration, load_golden, pkg
from mesh_normals_reference import np_normals
from mesh_smooth_reference import FIX_BOUNDARY, NORMALS, np_smooth
from test_gpu_mesh import _edge_from_percentile, _lasso, _synth_scanner
from test_meshio_normals import read_ply

pytestmark = pytest.mark.gpu

INF = float("inf")
SL3D_E_INVALID_ARG = -1
LAM, MU = 0.5, -0.53
# tests/test_mesh_smooth_arith.py: GOLDEN -- vertices without a neighbour and boundary vertices of the crops per max_edge
CROP_COUNTS = {"real_edge": {0.25: (2511, 898), 1.0: (1651, 1503), INF: (0, 481)}, "real_inside": {0.25: (589, 2388), 1.0: (398, 1335), INF: (0, 390)}}


def _same(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape, tag
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag


def _unchanged(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)


def _check(sc, max_edge, view=0, iterations=10, lam=LAM, mu=MU, flags=0, tag=None, mesh=None, stats=None):
    """the device's smoothed vertices (and normals) of one view == the restatement on the device's own mesh; returns (smoothed, vertices,
    faces)"""
    verts, faces = mesh if mesh is not None else sc.mesh(max_edge, view)
    want = np_smooth(verts, faces, iterations, lam, mu, flags & FIX_BOUNDARY, stats)
    got = sc.mesh_smoothed(max_edge, view, iterations, lam, mu, bool(flags & FIX_BOUNDARY), bool(flags & NORMALS))
    tag = (tag, view, max_edge, iterations, mu, flags)
    if flags & NORMALS:
        got, got_n = got
        _same(got_n, np_normals(want, faces), tag + ("normals",))
    _same(got, want, tag)
    return got, verts, faces


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
            mesh = sc.mesh(max_edge)
            for flags in range(4):
                st = {}
                got, verts, faces = _check(sc, max_edge, flags=flags, tag=name, mesh=mesh, stats=st)          # Taubin: 10 x (0.5, -0.53)
                _check(sc, max_edge, iterations=3, mu=0.0, flags=flags, tag=name, mesh=mesh)                   # Laplacian
                # bitwise unchanged: exactly the vertices without a neighbour, plus the boundary ones with the flag
                alone, boundary = st["degree"] == 0, st["boundary"]
                print(f"{name} keep {keep} max_edge {max_edge} flags {flags}: {int(alone.sum())} without a neighbour, {int(boundary.sum())} boundary")
                assert (int(alone.sum()), int(boundary.sum())) == CROP_COUNTS[name][max_edge]
                assert np.array_equal(_unchanged(got, verts), alone | boundary if flags & FIX_BOUNDARY else alone)
                assert st["degree"].max() == 8 and np.isfinite(got).all()


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
                mesh = sc.mesh(max_edge)
                got, verts, faces = _check(sc, max_edge, iterations=3, flags=NORMALS, tag=(W, H, p), mesh=mesh)
                _check(sc, max_edge, iterations=2, mu=0.0, flags=FIX_BOUNDARY | NORMALS, tag=(W, H, p), mesh=mesh)
                assert len(faces) > 0 and not _unchanged(got, verts).all()
            # across the chunk seam: a vertex at column 1023 and one at 1024 share a face -- they are neighbours -- and both move
            if W > 1025 and p == 1.0:
                pix = np.flatnonzero(sc.points()[1].ravel() == 1)
                cols = pix[faces] % W
                seam = faces[(cols.min(axis=1) == 1023) & (cols.max(axis=1) == 1024)]
                assert len(seam) > 0
                ids = seam.ravel()
                assert set(pix[ids] % W) == {1023, 1024} and not _unchanged(got[ids], verts[ids]).any()


@pytest.mark.parametrize("W,H", [(300, 1), (1, 300)])
def test_one_row_and_one_column(W, H):
    S, syn = pkg("scanner"), pkg("synth")
    with _synth_scanner(S, syn, W, H, 8, 2, PW=512, PH=512, full=(300, 300), origin=(0 if W > 1 else 150, 0 if H > 1 else 150)) as sc:
        sc.set_mask(np.ones((300, 300), np.uint8))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=0)
        sc.run()
        for flags in (0, FIX_BOUNDARY | NORMALS):
            got, verts, faces = _check(sc, INF, iterations=2, flags=flags, tag=(W, H))
            assert len(faces) == 0 and len(got) == int(sc.points()[1].sum()) > 0
            _same(got, sc.cloud(), (W, H))                               # no faces: the cloud, bitwise


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
            got, verts, _ = _check(sc, max_edge, iterations=3, flags=FIX_BOUNDARY | NORMALS, tag="window")
            assert not _unchanged(got, verts).all()
        sc.set_mask(np.zeros((FH, FW), np.uint8))
        sc.run()
        assert sc.points()[1].sum() == 0
        got, _, _ = _check(sc, INF, flags=NORMALS, tag="empty")
        assert got.shape == (0, 3)
        assert sc.mesh_smoothed(INF).shape == (0, 3)


# ---- 3. iteration counts: the result lands in the right plane for odd and even step counts ------------------------------------------------
def test_iteration_counts_and_plane_parity():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw = 322, 181, 8, 2
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.5))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        max_edge = _edge_from_percentile(sc, 0, 80)
        mesh = sc.mesh(max_edge)
        seen = []
        for iterations in (1, 2, 7):
            for mu in (MU, 0.0):                                          # 2, 4, 14 and 1, 2, 7 steps
                for flags in (0, NORMALS):
                    got, verts, faces = _check(sc, max_edge, iterations=iterations, mu=mu, flags=flags, tag="parity", mesh=mesh)
                # the device-resident form describes the same arrays
                m, nv = sc.mesh_smoothed_device(max_edge, 0, 1, iterations, LAM, mu, False, True)
                assert nv == [len(got)] and m.view_stride_points >= W * H and m.normals
                dx, dn = np.empty((nv[0], 3), np.float32), np.empty((nv[0], 3), np.float32)
                sc._d2h(dx, m.xyz)
                sc._d2h(dn, m.normals)
                _same(dx, got, ("device", iterations, mu))
                _same(dn, np_normals(got, faces), ("device normals", iterations, mu))
                seen.append(got.tobytes())
        assert len(set(seen)) == len(seen)
        m, _ = sc.mesh_smoothed_device(max_edge)
        assert m.normals is None                                          # NULL without SL3D_SMOOTH_NORMALS


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------
def test_batches_equal_one_view_calls():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 640, 360, 9, 2, 4
    rng = np.random.default_rng(16)
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=1024, PH=1024) as sc:
        for v in range(V):
            m = syn.default_mask(W, H) if v % 3 == 0 else _lasso(W, H, dx=7 * v - 50, dy=3 * v - 20) if v % 3 == 1 else (rng.random((H, W)) < 0.7).astype(np.uint8)
            sc.set_mask(m, view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        single = [sc.mesh_smoothed(max_edge, v, 3, normals=True) for v in range(V)]
        assert len({len(x) for x, _ in single}) > 2                       # the views differ
        for v in (1, 2):
            _check(sc, max_edge, v, iterations=3, flags=NORMALS, tag="single")
        for first, n in ((1, 3), (0, 4)):
            got = sc.meshes_smoothed(max_edge, first, n, 3, normals=True)
            assert len(got) == n
            for k in range(n):
                _same(got[k][0], single[first + k][0], (first, n, k))
                _same(got[k][1], single[first + k][1], (first, n, k, "normals"))
            m, nv = sc.mesh_smoothed_device(max_edge, first, n, 3, normals=True)
            for k in range(n):
                out = np.empty((nv[k], 3), np.float32)
                sc._d2h(out, m.xyz + 12 * k * m.view_stride_points)
                _same(out, single[first + k][0], ("device", first, k))


# ---- 5. repeatability, no side effects ------------------------------------------------------------------------------------------------------
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
        max_edge = _edge_from_percentile(sc, 0, 80)
        want = sc.meshes(max_edge, 0, V)
        want_n = sc.meshes_normals(max_edge, 0, V)
        want_l = sc.meshes_components(max_edge, 0, V)
        # what a caller holds on the device while it asks for the smoothed mesh
        m, nv, nf = sc.mesh_device(max_edge, 0, V)
        dn, sn, _ = sc.mesh_normals_device(max_edge, 0, V)
        dl, sl, _, _ = sc.mesh_components_device(max_edge, 0, V)
        a = sc.meshes_smoothed(max_edge, 0, V, 4, normals=True)
        other = sc.meshes_smoothed(INF, 0, V, 3, lam=0.25, mu=0.0, fix_boundary=True)
        b = sc.meshes_smoothed(max_edge, 0, V, 4, normals=True)
        for v in range(V):
            assert a[v][0].tobytes() == b[v][0].tobytes() and a[v][1].tobytes() == b[v][1].tobytes() and len(a[v][0]) == nv[v]
            assert other[v].tobytes() != a[v][0].tobytes()
            s = np_smooth(*want[v], 4, LAM, MU)
            _same(a[v][0], s, v)
            _same(a[v][1], np_normals(s, want[v][1]), v)
            xyz, valid = sc.points(v)
            assert np.array_equal(valid, before[v][1]) and np.array_equal(xyz.view(np.uint32), before[v][0].view(np.uint32))
            dx, df = np.empty((nv[v], 3), np.float32), np.empty((nf[v], 3), np.int32)
            sc._d2h(dx, m.xyz + 12 * v * m.view_stride_points)
            sc._d2h(df, m.faces + 12 * v * m.view_stride_faces)
            assert np.array_equal(dx.view(np.uint32), want[v][0].view(np.uint32)) and np.array_equal(df, want[v][1])
            on, ol = np.empty((nv[v], 3), np.float32), np.empty(nv[v], np.int32)
            sc._d2h(on, dn + 12 * v * sn)
            sc._d2h(ol, dl + 4 * v * sl)
            assert np.array_equal(on.view(np.uint32), want_n[v].view(np.uint32)) and np.array_equal(ol, want_l[v])
        assert np.array_equal(sc.cloud(0), cloud0)


# ---- 6. the filtered mesh: gathers through vertex_ids ------------------------------------------------------------------------------------
def test_gather_through_the_filtered_mesh():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw = 322, 181, 8, 2
    rng = np.random.default_rng(2)
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.3) | (rng.random((H, W)) < 0.45).astype(np.uint8))       # one object among many fragments
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        max_edge = _edge_from_percentile(sc, 0, 80)
        verts, faces = sc.mesh(max_edge)
        fx, ff, ids = sc.mesh_filtered(max_edge, 20)
        assert 0 < len(ids) < len(verts) and len(ff) > 0
        for fix in (False, True):
            s, n = sc.mesh_smoothed(max_edge, 0, 3, fix_boundary=fix, normals=True)
            # the filtered mesh smoothed on its own (its faces, its ids) == the gather: a kept vertex keeps all its faces
            own = np_smooth(fx, ff, 3, LAM, MU, FIX_BOUNDARY if fix else 0)
            _same(s[ids], own, ("gather", fix))
            _same(n[ids], np_normals(own, ff), ("gather normals", fix))
            assert np.array_equal(ids[ff], faces[np.isin(faces, ids).all(axis=1)])


# ---- 7. the error contract -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments():
    S, syn = pkg("scanner"), pkg("synth")
    W, H, N, fw, V = 322, 181, 8, 2, 2
    with _synth_scanner(S, syn, W, H, N, fw, V=V, PW=512, PH=512) as sc:
        for v in range(V):
            sc.set_mask(_lasso(W, H, share=0.5, dx=5 * v), view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=2)
        sc.run(0, V)
        max_edge = _edge_from_percentile(sc, 0, 80)
        meshes = sc.meshes(max_edge, 0, V)
        want = [np_smooth(x, f, 2, LAM, MU) for x, f in meshes]
        dev, nv0 = sc.mesh_smoothed_device(max_edge, 0, V, 2, normals=True)

        def device_result():
            out = []
            for k in range(V):
                a, n = np.empty((nv0[k], 3), np.float32), np.empty((nv0[k], 3), np.float32)
                sc._d2h(a, dev.xyz + 12 * k * dev.view_stride_points)
                sc._d2h(n, dev.normals + 12 * k * dev.view_stride_points)
                out.append((a, n))
            return out

        for k in range(V):
            _same(device_result()[k][0], want[k], k)
            _same(device_result()[k][1], np_normals(want[k], meshes[k][1]), k)
        m, nv = S.MeshSmoothed(), (C.c_int64 * V)()

        def smooth(first=0, n=V, e=max_edge, it=2, lam=LAM, mu=MU, flags=0, counts=nv):
            return sc.L.sl3d_mesh_smooth(sc._h, first, n, e, it, lam, mu, flags, C.byref(m), counts)

        def get(first=0, n=V, e=max_edge, it=2, lam=LAM, mu=MU, flags=0, counts=nv):
            return sc.L.sl3d_get_mesh_smoothed(sc._h, first, n, e, it, lam, mu, flags, None, None, 0, counts)

        nan = float("nan")
        bad = [dict(e=nan), dict(e=0.0), dict(e=-0.0), dict(e=-1.0), dict(e=-INF),
               dict(it=0), dict(it=-3), dict(it=1025),
               dict(lam=nan), dict(lam=INF), dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5),
               dict(mu=nan), dict(mu=-INF), dict(mu=INF), dict(mu=0.5), dict(mu=-1.5),
               dict(flags=4), dict(flags=0x80000001),
               dict(first=-1, n=1), dict(n=V + 1), dict(first=1, n=0), dict(first=V, n=1),
               dict(counts=None)]
        for i, kw in enumerate(bad):
            for call in (smooth, get):
                sc.synchronize()                                            # (a successful call in between: the text below is the refusal's)
                assert call(**kw) == SL3D_E_INVALID_ARG, (i, kw)
                assert len(sc.L.sl3d_last_error(sc._h)) > 0, (i, kw)
            for k in range(V):                                              # nothing on the device changed
                _same(device_result()[k][0], want[k], (i, k))
        assert smooth(it=1024, lam=1.0, mu=-1.0, n=1) == 0 and smooth(it=1, lam=1e-3, mu=0.0) == 0      # the ends of the ranges are inside
        with pytest.raises(S.Sl3dError):
            sc.mesh_smoothed(max_edge, iterations=0)
        for k in range(V):
            _check(sc, max_edge, k, iterations=2, flags=FIX_BOUNDARY | NORMALS, tag="after refusals", mesh=meshes[k])


# ---- 8. a smoothed mesh with normals as a PLY file -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_of_a_smoothed_mesh_with_normals(tmp_path, binary):
    S, syn, io = pkg("scanner"), pkg("synth"), pkg("meshio")
    W, H, N, fw = 322, 181, 8, 2
    with _synth_scanner(S, syn, W, H, N, fw, PW=512, PH=512) as sc:
        sc.set_mask(_lasso(W, H, share=0.4))
        sc.synth_view(0, plane=(0.0, 0.05, 0.05), view_id=0, noise=2)
        sc.run()
        max_edge = _edge_from_percentile(sc, 0, 80)
        verts, faces = sc.mesh(max_edge)
        s, n = sc.mesh_smoothed(max_edge, fix_boundary=True, normals=True)
        assert len(faces) > 0 and not _unchanged(s, verts).all() and (n != 0).any()
        path = str(tmp_path / "smoothed.ply")
        io.write_ply(path, s, faces=faces, binary=binary, normals=n)
        got = read_ply(path)
        gx, gn, gf = got[1], got[2], got[4]
        assert np.array_equal(gx.view(np.uint32), s.view(np.uint32)) and np.array_equal(gn.view(np.uint32), n.view(np.uint32))
        assert np.array_equal(gf, faces)
