"""CPU tests of the inputs of tests/edge_frames.py, before any GPU time is spent: with the oracle and the NumPy restatements alone
(one_axis_reference fed the oracle's planes of one axis, subpixel_reference / anchor_reference fed both) they prove that the frames do what
tests/test_gpu_subpixel_edges.py relies on.  For `random` and `noise3` on the base shape, per coded axis and for the two-axis scan:

(a) the valid share is strictly between 0 and 1 with at least 500 valid pixels; (b) a selected pixel fails `correspond`; (c) at least 10
    valid pixels have an anchored coordinate more than half a fringe width from the plain one; (d) every border line of the frame holds a
    valid pixel, and on the lines where stage 4's loop does not run the anchored coordinate IS the plain one (anchor_applies is false);
(e) the float64 restatements are well conditioned on exactly these inputs: against the same formulas evaluated in np.longdouble, points
    within 1e-9 relative (four orders below the device tests' 1e-5 bar), two-axis residuals within a hundredth of the residual bar of
    tests/test_gpu_subpixel.py (1e-8 * ref + 1e-9 px), no pixel left out.  The measured maxima are printed.
These are conditions on the inputs: if a seed fails one, the seed or the shape changes, never the condition.

(f) view_masks(): the structure the per-view-mask test needs, asserted on the arrays; selected() against the oracle's boundary removal."""
import numpy as np
import pytest

from oracle.oracle import Oracle

import anchor_reference as AR
import edge_frames as EF
import one_axis_reference as OR

CONDITIONED = [(name, shape, p) for name, shape, p in EF.BASE_CASES if name in ("random", "noise3")]


# ---- the formulas of the restatements with the number type as a parameter --------------------------------------------------------------------
def _undistort_reproject(T, px, py, K, d):
    K = np.asarray(K, np.float64).reshape(3, 3).astype(T)
    k1, k2, p1, p2, k3 = (T(v) for v in np.asarray(d, np.float64).ravel())
    one, two = T(1), T(2)
    ifx, ify = one / K[0, 0], one / K[1, 1]
    x0, y0 = (px.astype(T) - K[0, 2]) * ifx, (py.astype(T) - K[1, 2]) * ify
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = one / (one + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = two * p1 * x * y + p2 * (r2 + two * x * x)
        dy = p1 * (r2 + two * y * y) + two * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    h = [K[i, 0] * x + K[i, 1] * y + K[i, 2] for i in range(3)]
    return h[0] / h[2], h[1] / h[2]


def _one_axis_points(T, cal, A_cam, A_proj, axis, cols, rows, s):
    """Steps 5 and 6 of tests/one_axis_reference.py in the number type T."""
    Kc, dc, _, _, Kp, _, _, _ = cal
    u, v = _undistort_reproject(T, cols, rows, Kc, dc)
    K = np.asarray(Kp, np.float64).reshape(3, 3).astype(T)
    f, c = (K[0, 0], K[0, 2]) if axis == 0 else (K[1, 1], K[1, 2])
    t = f * ((s.astype(T) - c) * (T(1) / f)) + c
    Ac, Ap = np.asarray(A_cam, np.float64).reshape(3, 4).astype(T), np.asarray(A_proj, np.float64).reshape(3, 4).astype(T)
    spec = [(Ac, 0, u), (Ac, 1, v), (Ap, axis, t)]
    r = [np.stack([A[k, j] - x * A[2, j] for j in range(3)], axis=-1) for A, k, x in spec]
    F = [A[2, 3] * x - A[k, 3] for A, k, x in spec]
    cross = lambda p, q: np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=-1)
    c0, c1, c2 = cross(r[1], r[2]), cross(r[2], r[0]), cross(r[0], r[1])
    det = r[0][:, 0] * c0[:, 0] + (r[0][:, 1] * c0[:, 1] + r[0][:, 2] * c0[:, 2])
    assert (det != 0).all()
    n = F[0][:, None] * c0 + (F[1][:, None] * c1 + F[2][:, None] * c2)
    return n * (T(1) / det)[:, None]


def _two_axis(T, cal, A_cam, A_proj, cols, rows, xy):
    """The solve and the residual (before its float cast) of tests/subpixel_reference.py in the number type T."""
    Kc, dc, _, _, Kp, dp, _, _ = cal
    u, v = _undistort_reproject(T, cols, rows, Kc, dc)
    up, vp = _undistort_reproject(T, xy[:, 0], xy[:, 1], Kp, dp)
    Ac, Ap = np.asarray(A_cam, np.float64).reshape(3, 4).astype(T), np.asarray(A_proj, np.float64).reshape(3, 4).astype(T)
    spec = [(Ac, 0, u), (Ac, 1, v), (Ap, 0, up), (Ap, 1, vp)]
    P = np.stack([np.stack([A[k, q] - t * A[2, q] for q in range(3)], axis=-1) for A, k, t in spec], axis=-2)
    F = np.stack([A[2, 3] * t - A[k, 3] for A, k, t in spec], axis=-1)
    I1 = np.stack([np.stack([sum(P[:, a, i] * P[:, a, j] for a in range(4)) for j in range(3)], axis=-1) for i in range(3)], axis=-2)
    m = lambda i, j: I1[:, i, j]
    det = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) + m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0))
    assert (det != 0).all()
    adj = [m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2), m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1),
           m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0), m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2),
           m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0), m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1), m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)]
    inv = np.stack([a * (T(1) / det) for a in adj], axis=-1).reshape(I1.shape)
    I2 = np.stack([np.stack([sum(inv[:, i, k] * P[:, a, k] for k in range(3)) for a in range(4)], axis=-1) for i in range(3)], axis=-2)
    X = np.stack([sum(I2[:, i, a] * F[:, a] for a in range(4)) for i in range(3)], axis=-1)

    def err2(A, x, y):
        h = [A[i, 0] * X[:, 0] + A[i, 1] * X[:, 1] + A[i, 2] * X[:, 2] + A[i, 3] for i in range(3)]
        eu, ev = h[0] / h[2] - x, h[1] / h[2] - y
        return eu * eu + ev * ev

    return X, np.sqrt(err2(Ac, u, v) + err2(Ap, up, vp))


def _rel(X, ref):
    ref = ref.astype(np.longdouble)
    return float((np.linalg.norm((X.astype(np.longdouble) - ref).astype(np.float64), axis=-1) / np.linalg.norm(ref.astype(np.float64), axis=-1)).max())


def _border_lines(v):
    return dict(top=v[0], bottom=v[-1], left=v[:, 0], right=v[:, -1])


# ---- (a)-(e) per coded axis --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name,shape,p", CONDITIONED)
def test_one_axis_inputs_take_every_branch(name, shape, p, axis):
    c, o = EF.case(name, shape, p, axis), EF.oracle_scan(name, shape, p, axis)
    plain, anch = EF.restated_one_axis(name, shape, p, axis, False), EF.restated_one_axis(name, shape, p, axis, True)
    sel, v = o["valid_axis"][axis] == 1, plain["valid"] == 1
    assert np.array_equal(plain["valid"], anch["valid"])
    assert 0.0 < v.mean() < 1.0 and v.sum() >= 500, (int(v.sum()), v.size)                                        # (a)
    assert (sel & ~v).any(), "a selected pixel must fail correspond"                                                # (b)
    far = v & (np.abs(anch["s"] - plain["s"]) > 0.5 * EF.FW[axis])
    assert far.sum() >= 10, int(far.sum())                                                                          # (c)
    applies = AR.applies(axis, v.shape, c["origin"], c["full"], EF.N[axis])
    off = ("left", "right") if axis == 0 else ("top", "bottom")
    for line, on in _border_lines(v).items():                                                                       # (d)
        assert on.any(), (line, "holds no valid pixel")
        assert (not _border_lines(applies)[line].any()) == (line in off)
    skipped = v & ~applies
    assert skipped.sum() >= 2 and np.array_equal(anch["s"][skipped], plain["s"][skipped]) and (anch["s"][v & applies] != plain["s"][v & applies]).any()
    rows, cols = np.nonzero(v)                                                                                      # (e)
    worst = 0.0
    for r in (plain, anch):
        args = (c["cal"], o["A_cam"], o["A_proj"], axis, cols + c["origin"][0], rows + c["origin"][1], r["s"][v])
        assert np.array_equal(_one_axis_points(np.float64, *args), r["ipoints"][v]), "the same formulas"
        worst = max(worst, _rel(_one_axis_points(np.longdouble, *args), r["ipoints"][v]))
    det = np.abs(plain["det"][v])
    print(f"{name}, axis {axis}: {int(v.sum())} of {v.size} valid, {int((sel & ~v).sum())} selected pixels fail correspond, {int(far.sum())} anchored by more than "
          f"fw / 2, {int(skipped.sum())} valid where the formula does not apply, |det| min {det.min():.3g}; float64 against longdouble: points {worst:.2e} rel")
    assert worst <= 1e-9


# ---- (a)-(e) of the two-axis scan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,p", CONDITIONED)
def test_two_axis_inputs_take_every_branch(name, shape, p):
    c, o = EF.case(name, shape, p), EF.oracle_scan(name, shape, p)
    plain, anch = EF.restated_two_axis(name, shape, p, False), EF.restated_two_axis(name, shape, p, True)
    sel, v = (o["valid_axis"][0] == 1) & (o["valid_axis"][1] == 1), o["valid"] == 1
    assert 0.0 < v.mean() < 1.0 and v.sum() >= 500, (int(v.sum()), v.size)
    assert (sel & ~v).any()
    d = np.abs(anch["xy"] - plain["xy"])
    far = v & ((d[..., 0] > 0.5 * EF.FW[0]) | (d[..., 1] > 0.5 * EF.FW[1]))
    assert far.sum() >= 10, int(far.sum())
    for line, on in _border_lines(v).items():
        assert on.any(), (line, "holds no valid pixel")
        a = 0 if line in ("left", "right") else 1                # the axis whose formula does not apply on this line
        assert np.array_equal(_border_lines(anch["xy"][..., a])[line][on], _border_lines(plain["xy"][..., a])[line][on])
    rows, cols = np.nonzero(v)
    worst_p = worst_r = 0.0
    for r in (plain, anch):
        args = (c["cal"], o["A_cam"], o["A_proj"], cols + c["origin"][0], rows + c["origin"][1], r["xy"][v])
        X, res = _two_axis(np.float64, *args)
        assert np.array_equal(X, r["ipoints"][v]) and np.array_equal(res.astype(np.float32), r["residual"][v]), "the same formulas"
        XL, resL = _two_axis(np.longdouble, *args)
        worst_p = max(worst_p, _rel(XL, X))
        err = np.abs(res.astype(np.longdouble) - resL).astype(np.float64)
        assert (err <= 1e-8 * res + 1e-9).all(), (float(err.max()), float(res[np.argmax(err)]))
        worst_r = max(worst_r, float(err.max()))
    print(f"{name}, two axes: {int(v.sum())} of {v.size} valid, {int((sel & ~v).sum())} selected pixels fail, {int(far.sum())} anchored by more than fw / 2; "
          f"float64 against longdouble: points {worst_p:.2e} rel, residuals {worst_r:.2e} px (largest residual {float(plain['residual'][v].max()):.3g} px)")
    assert worst_p <= 1e-9


# ---- (f) the masks ---------------------------------------------------------------------------------------------------------------------------
def _quad_bits(selected):
    """(H, quads) int: bit k of an entry = pixel k of that quad is selected."""
    H, W = selected.shape
    padded = np.zeros((H, -(-W // 4) * 4), np.int64)
    padded[:, :W] = selected
    return (padded.reshape(H, -1, 4) << np.arange(4)).sum(-1)


@pytest.mark.parametrize("case", [("base", 1.0), ("base", 0.9), ("19x64", 0.9), ("130x3", 1.0), ("views", None)])
def test_selected_is_the_oracle_s_boundary_removal(case):
    masks = EF.view_masks() if case[0] == "views" else [EF.case("flat_17", *case)["mask"]]
    for mask in masks:
        H, W = mask.shape
        o = Oracle(W, H, EF.PW, EF.PH, *EF.N, *EF.FW)
        o.set_mask(mask)
        for a in (0, 1):
            o.compute_wrapped_phase(a, [np.zeros((H, W), np.uint8)] * 3)
            assert np.array_equal(o.valid_map(a), EF.selected(mask)), a
        o.close()


def test_view_masks_select_different_quads_and_lanes():
    A, B, C = EF.view_masks()
    (W, H), _, _ = EF.SHAPES["base"]
    assert all(m.shape == (H, W) and m.dtype == np.uint8 for m in (A, B, C))
    for m in (A, B):                                             # region edges on no multiple of 4
        rows, cols = np.nonzero(m)
        edges = {cols.min(), cols.max() + 1, rows.min(), rows.max() + 1} - {0, W, H}
        assert edges and all(e % 4 for e in edges), edges
    assert (A[:, :67] == 1).any() and not A[:, 67:].any() and (B[:, 34:] == 1).any() and not B[:, :34].any()
    qa, qb, qc = (_quad_bits(EF.selected(m)) for m in (A, B, C))
    # C: exactly one selected pixel in each of 40 quads, at lane positions 0 to 3 in turn
    rows, quads = np.nonzero(qc)
    assert len(rows) == 40 and EF.selected(C).sum() == 40
    assert [int(qc[r, q]) for r, q in zip(rows, quads)] == [1 << (i % 4) for i in range(40)]
    for first, last in ((qa, qc), (qc, qa)):                     # the launch over A, B, C and the one after A and C are swapped
        only_last = (last != 0) & (first == 0) & (qb == 0)
        assert only_last.sum() >= 4, "a quad whose first (and only) selecting view is the last view of the launch"
    only_one = ((qa != 0).astype(int) + (qb != 0) + (qc != 0)) == 1
    assert all((only_one & (q != 0)).sum() >= 4 for q in (qa, qb, qc)), "quads selected by exactly one view, for each view"
    # different views of one quad select different lanes: a lane of C that neither A nor B selects, in a quad A or B selects too
    own_lane = (qc != 0) & ((qa | qb) != 0) & ((qc & (qa | qb)) == 0)
    assert own_lane.sum() >= 1
    differ = (qa != 0) & (qb != 0) & (qa != qb)
    assert differ.sum() >= 10, "quads of which A and B select different lanes"
    print(f"selected pixels: A {int(EF.selected(A).sum())}, B {int(EF.selected(B).sum())}, C 40; quads of one view alone: A {int((only_one & (qa != 0)).sum())}, "
          f"B {int((only_one & (qb != 0)).sum())}, C {int((only_one & (qc != 0)).sum())}; C on a lane of its own beside A or B: {int(own_lane.sum())}")


def test_view_captures_differ_and_decode():
    """The three captures of the per-view-mask test: different frames, and under each of A and B more than 1000 valid pixels per axis."""
    for axis in (0, 1):
        caps = EF.view_captures(axis)
        assert len({np.stack(c[axis]).tobytes() for c in caps}) == 3
        for planes in caps:
            o = Oracle(*EF.SHAPES["base"][0], EF.PW, EF.PH, *EF.N, *EF.FW)
            o.set_mask(EF.view_masks()[0])
            o.set_calibration(*EF.case("flat_17", "base", 1.0, axis)["cal"])
            o.run_scan(*planes)
            ok, _ = OR.correspond(o.unwrapped_phi(axis), EF.FW[axis], EF.EXTENT[axis])
            assert ((o.valid_map(axis) == 1) & ok).sum() > 1000
            o.close()
