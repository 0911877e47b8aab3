"""GPU tests (-m gpu) of the radius outlier filter: sl3d_filter_outliers / k_outlier_support<RADIUS> / k_outlier_apply against the
NumPy restatement of the rule (tests/outlier_reference.py), bit for bit -- support plane, valid, points (as uint32) and counts.

The inputs go into a context's dense planes through tests/dense_planes.put_dense behind sc.run(); sc.synchronize(), with the padding
columns poisoned: a valid byte of 1 over a point that lies within max_dist of the window's last columns (outlier_reference.PAD), so a
kernel that clips the neighbourhood to the pitch instead of the window fails.  The tile of k_outlier_support is 64 x 8.

1. Crafted cases (holes, step, all valid, none valid, corners) x the shapes 1x1, 3x2, 9x9, 67x19, 130x37, 257x9 x radius 1 .. 4.
2. Ties on the integer lattice: <= counts a length of exactly max_dist, the next float below does not, +inf counts the window.
3. Jacobi: a line of samples loses exactly its two ends per call -- a row, a column, a row across a tile seam, samples one and two apart.
4. NaN, +-Inf and +-3e38 coordinates under valid pixels, finite points under invalid ones.
5. A batch of views 1 .. 4 of 7: each its own restatement, the views outside keep every byte.
6. min_neighbours = 0: the support plane alone.
7. The consumers on a decoded scene: points, cloud, mesh, intersection_points / c_p_map, residuals.
8. The call comes behind the launch lanes.
9. Every refusal, each leaving points, valid and support as they were."""
import ctypes as C

import numpy as np
import pytest

import outlier_reference as OR
from conftest import pkg
from dense_planes import put_dense
from test_gpu_mesh import _synth_scanner

pytestmark = pytest.mark.gpu

INF = float("inf")
INVALID_ARG, STATE = -1, -4
SHAPES = [(1, 1), (3, 2), (9, 9), (67, 19), (130, 37), (257, 9)]       # (W, H)


def _context(W, H, V=1, keep=False):
    """a context of the shape behind one run over small synthetic views: every buffer exists, nothing is pending"""
    S, syn = pkg("scanner"), pkg("synth")
    full = (max(W, 300), max(H, 300))
    sc = _synth_scanner(S, syn, W, H, 10, 2, V=V, PW=2048, PH=2048, keep=keep, full=full)
    sc.set_masks(np.ones((full[1], full[0]), np.uint8))
    for v in range(V):
        sc.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
    sc.run(0, V)
    sc.synchronize()
    return sc


def _state(sc, view=0):
    """(valid, points as uint32) of a view"""
    xyz, valid = sc.points(view)
    return valid, xyz.view(np.uint32)


def _put(sc, view, xyz, valid, pad=OR.PAD):
    put_dense(sc, view, xyz, valid, pad_xyz=np.float32(pad), pad_valid=1)


def _same_as(sc, view, want, counts, tag):
    """the support plane, valid, points and counts of a view against filter_outliers' dict"""
    got_v, got_b = _state(sc, view)
    got_s = sc.support(view)
    assert np.array_equal(got_s, want["support"]), (tag, int((got_s != want["support"]).sum()), "support bytes differ")
    assert np.array_equal(got_v, want["valid"]), (tag, int((got_v != want["valid"]).sum()), "valid bytes differ")
    assert np.array_equal(got_b, want["bits"]), (tag, int((got_b != want["bits"]).any(axis=-1).sum()), "points differ")
    if counts is not None:
        assert counts.dtype == np.uint32 and tuple(int(c) for c in counts) == want["counts"], (tag, counts, want["counts"])


def _filter_and_check(sc, xyz, valid, radius, max_dist, min_n, tag, pad=OR.PAD, view=0):
    _put(sc, view, xyz, valid, pad)
    counts = sc.filter_outliers(radius, max_dist, min_n, first_view=view)
    want = OR.filter_outliers(xyz, valid, radius, max_dist, min_n)
    _same_as(sc, view, want, counts[0], tag)
    return want


# ---- 1. crafted cases x shapes x radius ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_crafted_cases_equal_the_restatement(shape, radius):
    W, H = shape
    mixed = 0
    with _context(W, H) as sc:
        for name, xyz, valid in OR.crafted_cases(H, W):
            want = _filter_and_check(sc, xyz, valid, *OR.PARAMS[radius], (shape, radius, name))
            mixed += 0 < want["counts"][1] < want["counts"][0]
            if name == "none_valid":
                assert want["counts"] == (0, 0) and (want["support"] == OR.NO_SAMPLE).all()
            if name == "corners":
                assert want["counts"][0] == len({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)})
    assert mixed >= 2 or W * H <= 81, "the larger shapes reject some samples and keep others"


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_count_and_the_next_float_below_does_not():
    xyz, valid = OR.tie_lattice()
    H, W = valid.shape
    below = float(np.nextafter(np.float32(5), np.float32(0)))
    with _context(W, H) as sc:
        at5 = _filter_and_check(sc, xyz, valid, 1, 5.0, 8, "max_dist 5", pad=0)
        assert (at5["support"][1:-1, 1:-1] == 8).all() and at5["counts"][1] == 2 * (W + H) - 4      # only the border lacks neighbours
        under = _filter_and_check(sc, xyz, valid, 1, below, 8, "the float below 5", pad=0)
        assert (under["support"][1:-1, 1:-1] == 4).all() and under["counts"][1] == W * H
        for radius in (1, 2, 4):
            n = OR.max_support(radius)
            every = _filter_and_check(sc, xyz, valid, radius, INF, n, ("+inf", radius), pad=0)
            r, c = np.mgrid[0:H, 0:W]
            in_window = (np.minimum(r, radius) + np.minimum(H - 1 - r, radius) + 1) * (np.minimum(c, radius) + np.minimum(W - 1 - c, radius) + 1) - 1
            assert np.array_equal(every["support"], in_window)


# ---- 3. Jacobi -------------------------------------------------------------------------------------------------------------------------------
LINES = {
    "row": ((130, 19), [(9, c) for c in range(10, 20)], 1),
    "row_across_a_tile_seam": ((130, 19), [(9, c) for c in range(60, 70)], 1),
    "row_two_apart_across_a_tile_seam": ((130, 19), [(7, c) for c in range(54, 76, 2)], 2),
    "column_across_a_tile_seam": ((67, 19), [(r, 33) for r in range(4, 14)], 1),
    "column_two_apart": ((67, 19), [(r, 64) for r in range(1, 19, 2)], 2),
}


@pytest.mark.parametrize("name", LINES)
def test_a_line_loses_its_two_ends_per_call(name):
    (W, H), cells, radius = LINES[name]
    xyz, valid = OR.jacobi_line(H, W, cells)
    with _context(W, H) as sc:
        _put(sc, 0, xyz, valid, pad=0)
        left = list(cells)
        for call in range(3):
            counts = sc.filter_outliers(radius, 1.0, 2)
            assert tuple(counts[0]) == (len(left), 2), (name, call, counts)
            ends, left = (left[0], left[-1]), left[1:-1]
            got_v, got_b = _state(sc)
            want_v = np.zeros((H, W), np.uint8)
            for r, c in left:
                want_v[r, c] = 1
            assert np.array_equal(got_v, want_v), (name, call, "an in-place sweep eats the line")
            gone = (valid == 1) & (want_v == 0)
            assert (got_b[gone] == OR.NAN_BITS).all() and np.array_equal(got_b[~gone], xyz.view(np.uint32)[~gone])
            s = sc.support()
            assert all(s[r, c] == 2 for r, c in left) and all(s[r, c] == 1 for r, c in ends)      # the support as it was on entry
            assert (s == OR.NO_SAMPLE).sum() == W * H - len(left) - 2


# ---- 4. non-finite and huge coordinates ------------------------------------------------------------------------------------------------------
def test_non_finite_and_huge_coordinates():
    xyz, valid, special = OR.nonfinite_case()
    H, W = valid.shape
    with _context(W, H) as sc:
        for radius, max_dist, min_n in ((2, 1.5, 8), (1, 1.0, 1), (4, 2.5, 20)):
            want = _filter_and_check(sc, xyz, valid, radius, max_dist, min_n, ("non-finite", radius))
            for kind, where in special.items():
                assert all(want["support"][r, c] == 0 and want["rejected"][r, c] for r, c in where), kind
            assert (want["support"][valid == 0] == OR.NO_SAMPLE).all()
        _filter_and_check(sc, xyz, valid, 4, INF, 1, "non-finite, +inf")


# ---- 5. batches ------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_filters_its_views_and_no_other():
    W, H, V = 67, 19, 7
    cases = OR.crafted_cases(H, W)
    content = [cases[0], cases[1], cases[2], (None,) + OR.nonfinite_case(H, W)[:2], cases[4]]
    with _context(W, H, V=V) as sc:
        for v, (_, xyz, valid) in enumerate(content):
            _put(sc, v, xyz, valid)
        sc.filter_outliers(1, 1.0, 0, first_view=0)                                  # views 0 and 5 get a support plane, view 6 none
        sc.filter_outliers(1, 1.0, 0, first_view=5)
        outside = {v: _state(sc, v) + (sc.support(v),) for v in (0, 5)}
        outside[6] = _state(sc, 6)
        counts = sc.filter_outliers(2, 1.5, 8, first_view=1, n_views=4)
        assert counts.shape == (4, 2)
        for k, v in enumerate(range(1, 5)):
            _same_as(sc, v, OR.filter_outliers(content[v][1], content[v][2], 2, 1.5, 8), counts[k], ("view", v))
        assert len({tuple(c) for c in counts.tolist()}) == 4, "the views differ"
        for v, before in outside.items():
            after = _state(sc, v) + ((sc.support(v),) if v != 6 else ())
            assert all(np.array_equal(a, b) for a, b in zip(after, before)), ("view outside the batch", v)
        out = np.zeros((H, W), np.uint8)
        assert sc.L.sl3d_get_support(sc._h, 6, out.ctypes.data, W) == STATE


# ---- 6. min_neighbours == 0 ------------------------------------------------------------------------------------------------------------------
def test_min_neighbours_zero_writes_the_support_plane_alone():
    W, H = 130, 37
    _, xyz, valid = OR.crafted_cases(H, W)[1]
    with _context(W, H) as sc:
        want = _filter_and_check(sc, xyz, valid, 3, 2.0, 0, "min_neighbours 0")
        assert want["counts"][1] == 0 and np.array_equal(want["bits"], xyz.view(np.uint32)) and np.array_equal(want["valid"], valid)
        assert 0 < (want["support"] < 14).sum() < valid.sum(), "a positive min_neighbours would have rejected some samples"
        assert sc.filter_outliers(2, 1.5, 0, counts=False) is None                   # no counts asked: the support launch alone
        _same_as(sc, 0, OR.filter_outliers(xyz, valid, 2, 1.5, 0), None, "asynchronous")


# ---- 7. the consumers on a decoded scene -----------------------------------------------------------------------------------------------------
SCENE = dict(W=101, H=37, PW=512, PH=384, N=7, fw=4, full=(320, 240), origin=(37, 5))
DECODED = {"timed": {}, "keep_stages": dict(keep_stages=True), "subpixel": dict(subpixel=True), "subpixel_vertical": dict(subpixel=True, only_axis=0)}


def _scene_scanner(max_views=1, **kw):
    s, syn = SCENE, pkg("synth")
    sc = pkg("scanner").Scanner(s["W"], s["H"], s["PW"], s["PH"], s["N"], s["N"], s["fw"], s["fw"], max_views=max_views, full_size=s["full"],
                                origin=s["origin"], **kw)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(s["full"][0], s["full"][1], s["PW"], s["PH"])))
    sc.set_masks(np.ones((s["full"][1], s["full"][0]), np.uint8))
    for v in range(max_views):
        sc.synth_view(v, plane=(0.0, 0.05, 0.05) if v == 0 else (4.0, 0.02, -0.04), view_id=v, noise=1)
    return sc


def _scene_distance(xyz, valid):
    """max_dist for (radius 2, min_neighbours 8) from the scene's pixel spacing: the first multiple of the median distance between row
    neighbours at which the restatement rejects some samples and keeps at least a third"""
    both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
    spacing = float(np.median(np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)[both]))
    for factor in (1.6, 2.0, 2.5, 3.0):
        d = float(np.float32(factor * spacing))
        samples, rejected = OR.filter_outliers(xyz, valid, 2, d, 8)["counts"]
        if 0 < rejected < 2 * samples // 3:
            return d
    raise AssertionError("no multiple of the pixel spacing rejects some samples and keeps a third")


@pytest.mark.parametrize("name", DECODED)
def test_consumers_see_the_filtered_scan(name):
    kw = DECODED[name]
    with _scene_scanner(**kw) as sc:
        sc.run()
        xyz, valid = sc.points()
        assert (valid == 1).mean() > 0.5
        keep, residual = bool(kw.get("keep_stages")), bool(kw.get("subpixel")) and "only_axis" not in kw
        before = dict(ip=sc.intersection_points(), cp=sc.c_p_map()) if keep else {}
        if residual:
            before["res"] = sc.residuals().view(np.uint32)
        d = _scene_distance(xyz, valid)
        want = OR.filter_outliers(xyz, valid, 2, d, 8)
        counts = sc.filter_outliers(2, d, 8)
        print(f"{name}: max_dist {d:.4f}: {counts[0][1]} of {counts[0][0]} samples rejected")
        assert 0 < counts[0][1] < counts[0][0] and counts[0][0] > 0
        _same_as(sc, 0, want, counts[0], name)
        after_xyz, after_valid = sc.points()
        cloud, kept = sc.cloud(), np.ascontiguousarray(after_xyz[after_valid == 1])
        assert cloud.shape == kept.shape and np.array_equal(cloud.view(np.uint32), kept.view(np.uint32))
        assert len(kept) == counts[0][0] - counts[0][1]
        verts, faces = sc.mesh(INF)
        assert len(verts) == len(kept) and np.array_equal(verts.view(np.uint32), kept.view(np.uint32)) and len(faces) > 0
        if keep:
            ip = sc.intersection_points()
            assert (ip[want["rejected"]] == 0).all() and not np.signbit(ip[want["rejected"]]).any()
            assert np.array_equal(ip[~want["rejected"]].view(np.uint64), before["ip"][~want["rejected"]].view(np.uint64))
            assert np.array_equal(sc.c_p_map(), before["cp"])
        if residual:
            assert np.array_equal(sc.residuals().view(np.uint32), before["res"])
        sc.run()                                                                      # a run over the view restores it
        again_xyz, again_valid = sc.points()
        assert np.array_equal(again_valid, valid) and np.array_equal(again_xyz.view(np.uint32), xyz.view(np.uint32))


# ---- 8. ordering -----------------------------------------------------------------------------------------------------------------------------
def _ordering_sequence(sc, d, series):
    """everything a caller can observe of: a series of runs, the filter right behind it, a run, an asynchronous filter"""
    sc.synchronize()
    if series:
        for i in range(10):                                             # the two views in turn: the last launches go to the lanes
            sc.run(i % 2, 1)
        assert sc.launch_counts()[1] > 0, "the series put the launch lanes to use"
    else:
        sc.run(0, 2)
    out = [sc.filter_outliers(2, d, 8, first_view=0, n_views=2)]
    out += [a for v in (0, 1) for a in _state(sc, v) + (sc.support(v),)]
    sc.run(1, 1)
    assert sc.filter_outliers(1, d, 3, first_view=1, counts=False) is None
    out += [a for v in (0, 1) for a in _state(sc, v) + (sc.support(v),)]
    return out


def test_the_filter_comes_behind_the_launch_lanes():
    with _scene_scanner(2) as lanes, _scene_scanner(2, serial_launches=True) as serial:
        serial.run(0, 2)
        scan = [serial.points(v) for v in (0, 1)]
        d = _scene_distance(*scan[0])
        got, want = _ordering_sequence(lanes, d, True), _ordering_sequence(serial, d, False)
        assert serial.launch_counts()[1] == 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), ("step", k)
    first = [OR.filter_outliers(xyz, valid, 2, d, 8) for xyz, valid in scan]
    assert [tuple(c) for c in got[0].tolist()] == [f["counts"] for f in first] and got[0][:, 1].all()
    for v in (0, 1):
        assert np.array_equal(got[1 + 3 * v], first[v]["valid"]) and np.array_equal(got[2 + 3 * v], first[v]["bits"])
        assert np.array_equal(got[3 + 3 * v], first[v]["support"])
    second = OR.filter_outliers(*scan[1], 1, d, 3)                                    # view 1 was run again, then filtered with radius 1
    assert np.array_equal(got[10], second["valid"]) and np.array_equal(got[11], second["bits"]) and np.array_equal(got[12], second["support"])
    assert np.array_equal(got[7], first[0]["valid"]) and np.array_equal(got[9], first[0]["support"])      # view 0 stays filtered


# ---- 9. contracts ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_points_valid_and_support_as_they_were():
    S = pkg("scanner")
    W, H, V = 67, 19, 3
    _, xyz, valid = OR.crafted_cases(H, W)[0]
    nan = float("nan")
    with _synth_scanner(S, pkg("synth"), W, H, 10, 2, V=V, PW=2048, PH=2048, full=(300, 300)) as sc:      # before any run: no sample
        out = np.zeros((H, W), np.uint8)
        assert sc.L.sl3d_get_support(sc._h, 0, out.ctypes.data, W) == STATE          # no filter call yet on this context
        assert "no sl3d_filter_outliers" in sc.L.sl3d_last_error(sc._h).decode()
        assert sc.filter_outliers(2, 1.5, 8, 0, V).tolist() == [[0, 0]] * V and (sc.support(1) == OR.NO_SAMPLE).all()
    with _context(W, H, V=V) as sc:
        L, h = sc.L, sc._h
        assert L.sl3d_get_support(h, 1, out.ctypes.data, W) == STATE
        for v in (0, 1):
            _put(sc, v, xyz, valid)
        first = _filter_and_check(sc, xyz, valid, 2, 1.5, 8, "the call the refusals follow", view=1)
        before = [_state(sc, v) for v in range(V)] + [sc.support(1)]
        counts = (C.c_uint32 * (2 * V))(*[0xDEADBEEF] * (2 * V))
        refused = [(-1, 1, 2, 1.5, 8), (V, 1, 2, 1.5, 8), (0, 0, 2, 1.5, 8), (0, -1, 2, 1.5, 8), (1, V, 2, 1.5, 8), (0, V + 1, 2, 1.5, 8),   # bad views
                   (0, 1, 0, 1.5, 0), (0, 1, 5, 1.5, 8), (0, 1, -1, 1.5, 0),                                                            # radius outside 1 .. 4
                   (0, 1, 2, nan, 8), (0, 1, 2, 0.0, 8), (0, 1, 2, -0.0, 8), (0, 1, 2, -1.5, 8), (0, 1, 2, -INF, 8),                    # max_dist NaN or <= 0
                   (0, 1, 1, 1.5, 9), (0, 1, 2, 1.5, 25), (0, 1, 3, 1.5, 49), (0, 1, 4, 1.5, 81), (0, 1, 2, 1.5, -1)]                   # min_neighbours
        for first_view, n, radius, max_dist, min_n in refused:
            for c in (counts, None):
                assert L.sl3d_filter_outliers(h, first_view, n, radius, max_dist, min_n, c) == INVALID_ARG, (first_view, n, radius, max_dist, min_n)
        assert all(c == 0xDEADBEEF for c in counts)
        for view, ptr, stride in ((1, None, W), (1, out.ctypes.data, W - 1), (V, out.ctypes.data, W), (-1, out.ctypes.data, W)):
            assert L.sl3d_get_support(h, view, ptr, stride) == INVALID_ARG, (view, stride)
        for view in (0, 2):
            assert L.sl3d_get_support(h, view, out.ctypes.data, W) == STATE             # views no filter call has written
        with pytest.raises(S.Sl3dError):
            sc.support(0)
        assert not out.any()
        after = [_state(sc, v) for v in range(V)] + [sc.support(1)]
        for k, (a, b) in enumerate(zip(after, before)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b), ("after the refusals", k)
        assert np.array_equal(after[3], first["support"])
        # the largest min_neighbours of each radius is taken, +infinity is taken
        for radius in (1, 2, 3, 4):
            _filter_and_check(sc, xyz, valid, radius, INF, OR.max_support(radius), ("largest min_neighbours", radius))
