"""GPU tests (-m gpu): the fringe-modulation test (sl3d_set_masks_modulated / sl3d_get_modulation; 3dscan_amd/csrc/sl3d_modulation.h,
the reference's check_I_mod_criteria, 3/wrapped_phase.cpp:63-104).  gamma of the device equals a NumPy float32 restatement bit for bit;
a selection made on the device gives exactly what the same selection handed over through sl3d_set_masks gives, through every route a
mask takes (deferred MASKIN launch, eager preparation, several views per call, more than 4 views, the parity mode, no mask, pageable /
pinned / device-resident masks, segmented clouds, launch lanes); the oracle agrees on the valid map and the points; the call's
contracts (unsupported shapes, bad arguments, refused calls, frames replaced afterwards)."""
import numpy as np
import pytest

from conftest import assert_points_close, golden_calibration, load_golden, pkg
from instantiation_plan import Key

pytestmark = pytest.mark.gpu

SL3D_E_INVALID_ARG, SL3D_E_UNSUPPORTED = -1, -5


def np_gamma(f0, f1, f2):
    """3/wrapped_phase.cpp:92-94 in float32: sqrtf((float)(3d^2 + e^2)) / (float)(I0 + I1 + I2)"""
    i0, i1, i2 = (np.asarray(f, dtype=np.int64) for f in (f0, f1, f2))
    d, e = i0 - i2, 2 * i1 - i0 - i2
    t1 = np.sqrt((3 * d * d + e * e).astype(np.float32))
    t2 = (i0 + i1 + i2).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t1 / t2


def np_selection(fringe_v, fringe_h, thr, mask=None):
    """(mask == NULL || byte == 1) && (double)gamma_v > thr && (double)gamma_h > thr, as 0/1 bytes"""
    sel = (np_gamma(*fringe_v[:3]).astype(np.float64) > thr) & (np_gamma(*fringe_h[:3]).astype(np.float64) > thr)
    if mask is not None:
        sel &= np.asarray(mask) == 1
    return sel.astype(np.uint8)


def _same_float(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def _painted_capture(syn, W, H, PW, PH, N, fw, seed, view=0, plane=(0.0, 0.05, 0.05)):
    """A synthetic view with shadow rectangles (every plane dark and nearly flat), saturated pixels (255 on every fringe) and black
    pixels (0 on every fringe: gamma = 0/0)."""
    cap = syn.make_capture(W, H, PW, PH, N, N, fw, fw, plane=plane, view=view, noise=2)
    rng = np.random.default_rng(seed)
    pv, ph = [p.copy() for p in cap["planes_v"]], [p.copy() for p in cap["planes_h"]]
    for _ in range(4):
        y, x = int(rng.integers(0, max(1, H - 4))), int(rng.integers(0, max(1, W - 4)))
        h, w = int(rng.integers(1, max(2, H // 3))), int(rng.integers(1, max(2, W // 3)))
        _shadow(pv, ph, rng, y, x, h, w)
    sat = rng.random((H, W)) < 0.01
    black = rng.random((H, W)) < 0.01
    for p in pv[:3] + ph[:3]:
        p[sat] = 255
        p[black] = 0
    black[:2, :7] = True                                  # (the frame's first quads too)
    for p in pv[:3] + ph[:3]:
        p[:2, :7] = 0
    cap["planes_v"], cap["planes_h"] = pv, ph
    return cap


def _shadow(pv, ph, rng, y, x, h, w, F=3):
    """a dark patch: every plane dark; the fringes of an axis the same level plus a little noise (gamma 0 .. ~0.15)"""
    for planes in (pv, ph):
        base = rng.integers(6, 14, size=planes[0][y:y + h, x:x + w].shape)
        noisy = rng.random(base.shape) < 0.3
        for i, p in enumerate(planes):
            p[y:y + h, x:x + w] = (base + (noisy * rng.integers(0, 2, size=base.shape) if i < F else rng.integers(-4, 5, size=base.shape))).astype(np.uint8)


def _mixed_mask(rng, W, H):
    """bytes 0, 1 and 7 (selected iff == 1)"""
    return rng.choice(np.array([0, 1, 1, 1, 7], np.uint8), size=(H, W))


# ---- 1. gamma, bit exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(322, 181), (64, 7), (1920, 24)])
def test_modulation_equals_numpy_synthetic(W, H):
    S, syn = pkg("scanner"), pkg("synth")
    N, fw, V = 7, 4, 2
    PW, PH = fw << N, fw << N
    caps = [_painted_capture(syn, W, H, PW, PH, N, fw, seed=W + v, view=v, plane=(0.7 * v, 0.05, 0.04)) for v in range(V)]
    with S.Scanner(W, H, PW, PH, N, N, fw, fw, max_views=V) as sc:
        for v in range(V):
            sc.set_frames(0, caps[v]["planes_v"], view=v)
            sc.set_frames(1, caps[v]["planes_h"], view=v)
        for v in range(V):
            for axis, planes in ((0, caps[v]["planes_v"]), (1, caps[v]["planes_h"])):
                got, want = sc.modulation(axis, view=v), np_gamma(*planes[:3])
                assert got.dtype == np.float32 and got.shape == (H, W)
                assert np.isnan(want).any() and (want == 0).any()
                assert _same_float(got, want), (v, axis)


@pytest.mark.parametrize("name", ["real_edge", "real_inside"])
def test_modulation_equals_numpy_real_crops(name):
    """The reference's real captures, as windows of the 1600x1200 frame at the crop's origin (gamma needs no halo)."""
    S = pkg("scanner")
    g = load_golden(name)
    _, dims = golden_calibration()
    H, W = g["mask"].shape
    x0, y0 = [int(v) for v in g["origin"]]
    N_v, N_h, fw_v, fw_h, nc_v, nc_h = [int(v) for v in g["params"]]
    with S.Scanner(W, H, dims["PW"], dims["PH"], N_v, N_h, fw_v, fw_h, n_codes_v=nc_v, n_codes_h=nc_h, full_size=(dims["W"], dims["H"]),
                   origin=(x0, y0)) as sc:
        sc.set_frames(0, list(g["fringe_v"]) + list(g["gray_v"]) + list(g["inv_v"]))
        sc.set_frames(1, list(g["fringe_h"]) + list(g["gray_h"]) + list(g["inv_h"]))
        for axis, key in ((0, "fringe_v"), (1, "fringe_h")):
            assert _same_float(sc.modulation(axis), np_gamma(*g[key])), axis


# ---- 2. the device's selection == the same selection handed over -------------------------------------------------------------------
W2, H2, N2, FW2 = 322, 181, 7, 4
PW2 = PH2 = FW2 << N2
THR = 0.05


def _outputs(sc, n, clouds=None):
    """per view (xyz, valid) of the last dense launch -- or, behind a clouds launch, (None, valid) and the clouds"""
    out = [sc.points(v) for v in range(n)]
    if clouds is not None:
        return [(None, valid) for _, valid in out], clouds
    return out, None


def _assert_same(a, b, tag):
    (pa, ca), (pb, cb) = a, b
    for v, ((xa, va), (xb, vb)) in enumerate(zip(pa, pb)):
        assert np.array_equal(va, vb), (tag, v)
        if xa is not None:
            assert np.array_equal(xa, xb, equal_nan=True), (tag, v)
    if ca is not None:
        assert len(ca) == len(cb) and all(np.array_equal(x, y) for x, y in zip(ca, cb)), tag
        assert [len(x) for x in ca] == [int(valid.sum()) for _, valid in pa], tag


def _pair_run(V, caps, masks, how, clouds=False, thr=THR, **kw):
    """Context A: set_masks_modulated(thr, masks) over [0, V) in one call; context B: set_masks(NumPy selection).  Same frames, same
    launch.  Returns both contexts' outputs and A's kernel name."""
    torch = pytest.importorskip("torch") if how == "device" else None
    S, syn = pkg("scanner"), pkg("synth")
    cal = syn.cal_tuple(syn.synth_rig(W2, H2, PW2, PH2))
    sels = np.stack([np_selection(c["planes_v"], c["planes_h"], thr, None if masks is None else masks[v]) for v, c in enumerate(caps)])
    with S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=V, **kw) as a, S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=V, **kw) as b:
        for c in (a, b):
            c.set_calibration(*cal)
            c.set_masks(np.ones((H2, W2), np.uint8))       # (densely selected history: the dense MASKIN form)
            for v in range(V):
                c.set_frames(0, caps[v]["planes_v"], view=v)
                c.set_frames(1, caps[v]["planes_h"], view=v)
            c.run(0, V)
            c.synchronize()
        if how == "none":
            a.set_masks_modulated(thr, None, 0, V)
        elif how == "pinned":
            pm = a.pinned(masks.shape, np.uint8)
            pm[:] = masks
            a.set_masks_modulated(thr, pm)
        elif how == "device":
            d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
            torch.cuda.synchronize()
            a.set_masks_modulated_device(thr, d.data_ptr(), W2, H2 * W2, 0, V)
        elif how == "shared":                                # one mask for every view (view_stride 0)
            a.set_masks_modulated(thr, masks[0], 0, V)
        else:
            a.set_masks_modulated(thr, masks)
        b.set_masks(sels)
        res = []
        for c in (a, b):
            cl = c.fused_clouds(0, V) if clouds else c.run(0, V)
            if c is a:
                name = a.last_fused_kernel_name()
            res.append(_outputs(c, V, cl))
        if how == "device":
            a.synchronize()
            del d
    return res, name, sels


def _caps(V, seed=0):
    syn = pkg("synth")
    return [_painted_capture(syn, W2, H2, PW2, PH2, N2, FW2, seed=seed + v, view=v, plane=(1.1 * v, 0.05, 0.04)) for v in range(V)]


def test_single_timed_view_takes_the_maskin_route():
    caps = _caps(1)
    masks = _mixed_mask(np.random.default_rng(1), W2, H2)[None]
    (ra, rb), name, sels = _pair_run(1, caps, masks, "pageable")
    assert Key.parse(name).cmode & 4, name                    # the deferred selection was evaluated inside the fused launch
    _assert_same(ra, rb, "single timed view")
    assert 0 < int(ra[0][0][1].sum()) < int((masks[0] == 1).sum())


def test_eager_mask_context():
    caps = _caps(1, seed=10)
    masks = _mixed_mask(np.random.default_rng(2), W2, H2)[None]
    (ra, rb), name, _ = _pair_run(1, caps, masks, "pageable", eager_mask=True)
    assert not Key.parse(name).cmode & 4, name
    _assert_same(ra, rb, "eager")


@pytest.mark.parametrize("how", ["pageable", "pinned", "device", "none", "shared"])
def test_three_views_distinct_selections(how):
    caps = _caps(3, seed=20)
    rng = np.random.default_rng(3)
    masks = np.stack([_mixed_mask(rng, W2, H2) for _ in range(3)])
    (ra, rb), name, sels = _pair_run(3, caps, None if how == "none" else (np.stack([masks[0]] * 3) if how == "shared" else masks), how)
    assert Key.parse(name).cmode & 4, name
    assert not np.array_equal(sels[0], sels[1]) and not np.array_equal(sels[1], sels[2])
    _assert_same(ra, rb, how)


@pytest.mark.parametrize("clouds", [False, True])
def test_six_views_prepared_at_once(clouds):
    caps = _caps(6, seed=30)
    rng = np.random.default_rng(4)
    masks = np.stack([_mixed_mask(rng, W2, H2) for _ in range(6)])
    (ra, rb), name, _ = _pair_run(6, caps, masks, "pageable", clouds=clouds)
    assert not Key.parse(name).cmode & 4, name
    _assert_same(ra, rb, ("six views", clouds))


@pytest.mark.parametrize("how", ["pageable", "device"])
def test_run_clouds(how):
    caps = _caps(2, seed=40)
    rng = np.random.default_rng(5)
    masks = np.stack([_mixed_mask(rng, W2, H2) for _ in range(2)])
    (ra, rb), name, _ = _pair_run(2, caps, masks, how, clouds=True)
    assert Key.parse(name).cmode & 4, name
    _assert_same(ra, rb, ("clouds", how))


def test_keep_stages():
    caps = _caps(2, seed=50)
    rng = np.random.default_rng(6)
    masks = np.stack([_mixed_mask(rng, W2, H2) for _ in range(2)])
    (ra, rb), _, sels = _pair_run(2, caps, masks, "pageable", keep_stages=True)
    _assert_same(ra, rb, "keep_stages")


# ---- 3. the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_parity_full_frame_synthetic():
    """A whole 1600x1200 view with the reference's capture set (6 / 5 Gray planes, fringe width 32)."""
    from oracle.oracle import Oracle
    S, syn = pkg("scanner"), pkg("synth")
    W, H, PW, PH, Nv, Nh, fw = 1600, 1200, 1280, 720, 6, 5, 32
    cap = syn.make_capture(W, H, PW, PH, Nv, Nh, fw, fw, noise=2)
    rng = np.random.default_rng(7)
    pv, ph = [p.copy() for p in cap["planes_v"]], [p.copy() for p in cap["planes_h"]]
    for (y, x, h, w) in ((100, 200, 300, 250), (700, 900, 200, 500)):
        _shadow(pv, ph, rng, y, x, h, w)
    for p in pv[:3] + ph[:3]:
        p[150, 300] = 9                                      # (gamma 0 on both axes)
    cal = syn.cal_tuple(cap["cal"])
    sel = np_selection(pv, ph, 0.01, cap["mask"])
    o = Oracle(W, H, PW, PH, Nv, Nh, fw, fw)
    o.set_mask(sel)
    o.set_calibration(*cal)
    o.run_scan(pv, ph)
    v = o.valid_map(2) == 1
    with S.Scanner(W, H, PW, PH, Nv, Nh, fw, fw) as sc:
        sc.set_calibration(*cal)
        sc.set_frames(0, pv)
        sc.set_frames(1, ph)
        sc.set_masks_modulated(0.01, cap["mask"])
        sc.run()
        xyz, valid = sc.points()
    assert np.array_equal(valid == 1, v)
    assert v.sum() > 0.5 * W * H and not v[150, 300]
    assert_points_close(xyz, o.intersection_points(), v)


@pytest.mark.parametrize("thr", [0.01, 0.05])
def test_oracle_parity_real_edge(thr):
    """The real_edge crop (a capture at the lasso's edge) taken as a whole frame, with its own lasso."""
    from oracle.oracle import Oracle
    S = pkg("scanner")
    g = load_golden("real_edge")
    cal, dims = golden_calibration()
    H, W = g["mask"].shape
    N_v, N_h, fw_v, fw_h, nc_v, nc_h = [int(v) for v in g["params"]]
    pv = list(g["fringe_v"]) + list(g["gray_v"]) + list(g["inv_v"])
    ph = list(g["fringe_h"]) + list(g["gray_h"]) + list(g["inv_h"])
    counts = {}
    for label, sel in (("lasso", g["mask"]), ("lasso + modulation", np_selection(g["fringe_v"], g["fringe_h"], thr, g["mask"]))):
        o = Oracle(W, H, dims["PW"], dims["PH"], N_v, N_h, fw_v, fw_h, ncodes_v=nc_v, ncodes_h=nc_h)
        o.set_mask(sel)
        o.set_calibration(*cal)
        o.run_scan(pv, ph)
        v = o.valid_map(2) == 1
        with S.Scanner(W, H, dims["PW"], dims["PH"], N_v, N_h, fw_v, fw_h, n_codes_v=nc_v, n_codes_h=nc_h) as sc:
            sc.set_calibration(*cal)
            sc.set_frames(0, pv)
            sc.set_frames(1, ph)
            if label == "lasso":
                sc.set_mask(g["mask"])
            else:
                sc.set_masks_modulated(thr, g["mask"])
            sc.run()
            xyz, valid = sc.points()
        assert np.array_equal(valid == 1, v), label
        assert_points_close(xyz, o.intersection_points(), v)
        counts[label] = int(v.sum())
    print(f"real_edge, threshold {thr}: valid pixels {counts}")
    assert 0 < counts["lasso + modulation"] <= counts["lasso"]
    if thr == 0.05:
        assert counts["lasso + modulation"] < counts["lasso"]


# ---- 4. contracts -------------------------------------------------------------------------------------------------------------------
def _rc(sc, first, n, thr, mask=None, stride=None, view_stride=0):
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    return sc.L.sl3d_set_masks_modulated(sc._h, first, n, thr, None if m is None else m.ctypes.data,
                                          (m.strides[0] if stride is None else stride) if m is not None else 0, view_stride)


def test_unsupported_shapes_and_bad_arguments():
    S, syn = pkg("scanner"), pkg("synth")
    N, fw = 6, 4
    PW, PH = fw << N, fw << N
    mask = np.ones((40, 64), np.uint8)
    with S.Scanner(64, 40, PW, PH, N, N, fw, fw, n_fringe=4) as sc:
        assert _rc(sc, 0, 1, 0.01, mask) == SL3D_E_UNSUPPORTED
        out = np.empty((40, 64), np.float32)
        assert sc.L.sl3d_get_modulation(sc._h, 0, 0, out.ctypes.data, 64) == SL3D_E_UNSUPPORTED
    with S.Scanner(32, 20, PW, PH, N, N, fw, fw, full_size=(64, 40), origin=(16, 8)) as sc:   # a window
        assert _rc(sc, 0, 1, 0.01, mask) == SL3D_E_UNSUPPORTED
        assert _rc(sc, 0, 1, 0.01) == SL3D_E_UNSUPPORTED
        assert sc.modulation(1).shape == (20, 32)            # gamma itself works on any window
    with S.Scanner(64, 40, PW, PH, N, N, fw, fw, max_views=2) as sc:
        assert _rc(sc, 0, 1, float("nan"), mask) == SL3D_E_INVALID_ARG
        assert _rc(sc, 0, 1, float("nan")) == SL3D_E_INVALID_ARG
        assert _rc(sc, -1, 1, 0.01, mask) == SL3D_E_INVALID_ARG
        assert _rc(sc, 1, 2, 0.01, mask) == SL3D_E_INVALID_ARG
        assert _rc(sc, 0, 0, 0.01, mask) == SL3D_E_INVALID_ARG
        assert _rc(sc, 0, 1, 0.01, mask, stride=63) == SL3D_E_INVALID_ARG
        assert _rc(sc, 0, 2, 0.01, mask, view_stride=64) == SL3D_E_INVALID_ARG
        out = np.empty((40, 64), np.float32)
        assert sc.L.sl3d_get_modulation(sc._h, 0, 2, out.ctypes.data, 64) == SL3D_E_INVALID_ARG
        assert sc.L.sl3d_get_modulation(sc._h, 0, 0, out.ctypes.data, 63) == SL3D_E_INVALID_ARG
        assert sc.L.sl3d_get_modulation(sc._h, 2, 0, out.ctypes.data, 64) == SL3D_E_INVALID_ARG


@pytest.mark.parametrize("eager", [False, True])
def test_refused_call_keeps_the_previous_selection(eager):
    S, syn = pkg("scanner"), pkg("synth")
    caps = _caps(2, seed=60)
    cal = syn.cal_tuple(syn.synth_rig(W2, H2, PW2, PH2))
    lasso = _mixed_mask(np.random.default_rng(8), W2, H2)
    with S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=2, eager_mask=eager) as sc, \
            S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=2, eager_mask=eager) as ref:
        for c in (sc, ref):
            c.set_calibration(*cal)
            for v in range(2):
                c.set_frames(0, caps[v]["planes_v"], view=v)
                c.set_frames(1, caps[v]["planes_h"], view=v)
        # a selection that is still deferred (timed context) or already prepared (eager), then refused calls over the same views
        for c in (sc, ref):
            c.set_masks(lasso)
        assert _rc(sc, 0, 2, float("nan"), lasso) == SL3D_E_INVALID_ARG
        assert _rc(sc, 0, 2, 0.01, lasso, stride=W2 - 1) == SL3D_E_INVALID_ARG
        assert _rc(sc, 1, 2, 0.01) == SL3D_E_INVALID_ARG
        for c in (sc, ref):
            c.run(0, 2)
        _assert_same(_outputs(sc, 2), _outputs(ref, 2), "refused")
        # a modulated selection, then a refused call: the modulated selection stays
        sc.set_masks_modulated(THR, lasso)
        assert _rc(sc, 0, 2, float("nan")) == SL3D_E_INVALID_ARG
        ref.set_masks(np.stack([np_selection(c["planes_v"], c["planes_h"], THR, lasso) for c in caps]))
        for c in (sc, ref):
            c.run(0, 2)
        _assert_same(_outputs(sc, 2), _outputs(ref, 2), "refused after a modulated selection")


@pytest.mark.parametrize("eager", [False, True])
def test_frames_replaced_afterwards_do_not_change_the_selection(eager):
    S, syn = pkg("scanner"), pkg("synth")
    first, second = _caps(1, seed=70)[0], _caps(1, seed=71)[0]
    cal = syn.cal_tuple(syn.synth_rig(W2, H2, PW2, PH2))
    sel_first = np_selection(first["planes_v"], first["planes_h"], THR)
    assert not np.array_equal(sel_first, np_selection(second["planes_v"], second["planes_h"], THR))
    with S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, eager_mask=eager) as sc, S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, eager_mask=eager) as ref:
        for c in (sc, ref):
            c.set_calibration(*cal)
            c.set_frames(0, first["planes_v"])
            c.set_frames(1, first["planes_h"])
        sc.set_masks_modulated(THR)
        ref.set_mask(sel_first)
        for c in (sc, ref):
            c.set_frames(0, second["planes_v"])
            c.set_frames(1, second["planes_h"])
            c.run()
        _assert_same(_outputs(sc, 1), _outputs(ref, 1), "frames replaced")


# ---- 5. launch lanes ----------------------------------------------------------------------------------------------------------------
def test_one_view_scans_on_lanes_equal_serial_ones():
    S, syn = pkg("scanner"), pkg("synth")
    V = 4
    caps = _caps(V, seed=80)
    cal = syn.cal_tuple(syn.synth_rig(W2, H2, PW2, PH2))
    rng = np.random.default_rng(9)
    lassos = np.stack([_mixed_mask(rng, W2, H2) for _ in range(V)])
    lanes = S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=V)
    serial = S.Scanner(W2, H2, PW2, PH2, N2, N2, FW2, FW2, max_views=V, serial_launches=True)
    with lanes, serial:
        for c in (lanes, serial):
            c.set_calibration(*cal)
            for v in range(V):
                c.set_frames(0, caps[v]["planes_v"], view=v)
                c.set_frames(1, caps[v]["planes_h"], view=v)
        for i in range(24):
            v, k = i % V, (3 * i + 1) % V
            thr = (0.01, 0.05, 0.1)[i % 3]
            for c in (lanes, serial):
                c.set_masks_modulated(thr, lassos[k], v, 1)
                c.run(v, 1)
            if i >= 24 - V:
                want = np_selection(caps[v]["planes_v"], caps[v]["planes_h"], thr, lassos[k])
                _assert_same(_outputs_view(lanes, v), _outputs_view(serial, v), ("scan", i))
                assert not (lanes.points(v)[1] & ~want).any()
        assert sum(lanes.launch_counts()) == 24 and serial.launch_counts() == (24, 0)


def _outputs_view(sc, v):
    return [sc.points(v)], None
