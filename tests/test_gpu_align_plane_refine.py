"""GPU tests (-m gpu) of sl3d_refine_turntable_plane on the ray-cast scene of tests/test_align_plane_recovery_reference.py: an
ellipsoid off the turntable axis and a sphere beside it, 160 x 120, 4 views, step 20 degrees, put into a context's dense planes through
tests/dense_planes.put_dense behind sc.run(); sc.synchronize(), ray-cast through the camera sl3d_get_align_camera hands out.

The loop on the device is held to the restatement's loop (tests/align_plane_reference.refine) entry by entry: the same n_done, every
entry's estimate BIT FOR BIT, its accepted pairs, sources and rms_plane, and the same out.  The words are exact integers and the solve is
the same sequence of double operations over the same libm on both sides, so nothing separates them.  Every entry's pass is repeated
through sl3d_align_plane_sums and compared word for word.  Through this twin the recovery bar of the restatement -- a tenth of the
point-to-point loop's errors -- holds on the device; it is asserted here once more on the library's own numbers.  Then: sl3d_register_views
accepts the result; the points and valid planes of every view are byte-identical to before; a subset of the views; a degenerate scene; the
refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import align_plane_reference as PR
import align_reference as AR
from conftest import pkg
from dense_planes import put_dense

pytestmark = pytest.mark.gpu

S = AR.SCENE
EDGE = 2.0
INVALID_ARG = -1


@pytest.fixture(scope="module")
def sc():
    Sc = pkg("scanner")
    with Sc.Scanner(S["W"], S["H"], 256, 256, 7, 7, 2, 2, max_views=S["V"]) as s:
        s.set_calibration(*AR.scene_calibration())
        s.set_masks(np.ones((S["H"], S["W"]), np.uint8))
        for v in range(S["V"]):
            s.synth_view(v, plane=(0.0, 0.05, 0.05), view_id=v, noise=0)
        s.run(0, S["V"])
        s.synchronize()
        yield s


@pytest.fixture(scope="module")
def scene(sc):
    cam = sc.align_camera()
    points, valid, truth = AR.raycast_scene(cam)
    return cam, points, valid, truth


def _put(sc, points, valid):
    for v in range(len(points)):
        put_dense(sc, v, points[v], valid[v], pad_xyz=np.float32(0.0), pad_valid=0)


def _planes(sc):
    out = []
    for v in range(S["V"]):
        xyz, valid = sc.points(v)
        out += [xyz.view(np.uint32).copy(), valid.copy()]
    return out


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _same_entries(got, want):
    assert got["n_done"] == want["n_done"] == len(got["log"]) and got["degenerate"] == want["degenerate"]
    for i, (g, w) in enumerate(zip(got["log"], want["log"])):
        assert np.array_equal(g["est"], w["est"]), (i, g["est"], w["est"])                      # bit for bit
        assert (g["n"], g["sources"]) == (w["n"], w["sources"]) and _same_float(g["rms_xz"], w["rms_xz"]) and math.isnan(g["rms_y"]), i
    assert np.array_equal(got["est"], want["est"]) and (got["n"], got["sources"]) == (want["n"], want["sources"])
    assert _same_float(got["rms_xz"], want["rms_xz"]) and math.isnan(got["rms_y"])
    assert all(got[k] == want[k] and got[k].dtype == np.float32 for k in ("tx", "ty", "tz", "rot_step"))


def test_the_loop_entry_by_entry_against_the_restatement(sc, scene):
    cam, points, valid, truth = scene
    _put(sc, points, valid)
    before = _planes(sc)
    tx, ty, tz, rot = AR.scene_start(truth)
    args = (S["rng"], S["max_dist"], EDGE, S["window"])
    got = sc.refine_turntable_plane(0, S["V"], tx, ty, tz, rot, *args, iterations=S["iterations"])
    want = PR.refine(points, valid, cam, 0, 0, tx, ty, tz, rot, *args, S["iterations"])
    assert 2 <= want["n_done"] < S["iterations"] and not want["degenerate"]                     # by the restatement alone: the early stop
    _same_entries(got, want)
    ox, oz = float(tx), float(tz)
    for i, entry in enumerate(got["log"]):                                                      # (the pass itself, once more)
        words = PR.pass_sums(points, valid, cam, 0, 0, entry["est"], ox, oz, *args)
        assert np.array_equal(sc.align_plane_sums(0, S["V"], entry["est"], ox, oz, *args), words), i
        assert entry["n"] == int(words[:, 0].sum()) and entry["sources"] == int(words[:, 16].sum())
    # the recovery bar, on the library's own numbers: a tenth of what the library's point-to-point loop reaches from the same start
    parent = sc.refine_turntable(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], S["window"], iterations=S["iterations"])
    bar, last = AR.errors(parent["est"], truth), AR.errors(got["est"], truth)
    print(f"point-to-point {bar[0]:.4f} deg {bar[1]:.4f} mm; point-to-plane {last[0]:.4f} deg {last[1]:.4f} mm after {got['n_done']} iterations")
    assert 10.0 * last[0] <= bar[0] and 10.0 * last[1] <= bar[1] and 2 * got["log"][0]["n"] >= got["log"][0]["sources"]
    assert got["ty"] == ty and got["rot_step"] == np.float32(math.atan2(got["est"][1], got["est"][0]) * 180.0 * 7.0 / 22.0)
    # fewer iterations: the same first entries; without a log and without n_done
    two = sc.refine_turntable_plane(0, S["V"], tx, ty, tz, rot, *args, iterations=2)
    assert two["n_done"] == 2 and all(np.array_equal(a["est"], b["est"]) and a["n"] == b["n"] for a, b in zip(two["log"], got["log"]))
    out = pkg("scanner").Turntable()
    assert sc.L.sl3d_refine_turntable_plane(sc._h, 0, S["V"], tx, ty, tz, rot, *args, 2, C.byref(out), None, None) == 0
    assert np.array_equal(np.array(out.est[:]), two["est"]) and out.n == two["n"] and math.isnan(out.rms_y)
    # after the calls the points and valid planes of every view are byte-identical to before
    assert all(np.array_equal(a, b) for a, b in zip(_planes(sc), before))
    # the registration takes the refined numbers
    reg = sc.register_views(0, S["V"], got["tx"], got["ty"], got["tz"], got["rot_step"])
    assert len(reg) == int(valid.sum()) and np.isfinite(reg).all()
    assert np.allclose(reg[:int(valid[0].sum())], points[0][valid[0] == 1], rtol=0, atol=1e-3)                     # view 0 is not turned
    # ... and turns view 1 by the refined step about the refined axis: the restatement's own step, to float32 rounding (as for view 0)
    n0, n1 = int(valid[0].sum()), int(valid[1].sum())
    p = points[1][valid[1] == 1]
    assert np.allclose(reg[n0:n0 + n1], AR.step(p, got["est"]), rtol=0, atol=1e-3)


def test_a_subset_of_the_views_and_the_truth_as_a_start(sc, scene):
    cam, points, valid, truth = scene
    _put(sc, points, valid)
    tx, ty, tz, rot = AR.scene_start(truth)
    got = sc.refine_turntable_plane(1, 3, tx, ty, tz, rot, S["rng"], S["max_dist"], EDGE, 1, iterations=3)
    want = PR.refine(points[1:], valid[1:], cam, 0, 0, tx, ty, tz, rot, S["rng"], S["max_dist"], EDGE, 1, 3)
    _same_entries(got, want)
    a = (np.float32(truth[2]), np.float32(0.0), np.float32(truth[3]), AR.degrees_22_7(S["step_deg"]))
    got = sc.refine_turntable_plane(0, S["V"], *a, S["rng"], S["max_dist"], EDGE, S["window"], iterations=S["iterations"])
    _same_entries(got, PR.refine(points, valid, cam, 0, 0, *a, S["rng"], S["max_dist"], EDGE, S["window"], S["iterations"]))
    assert got["n_done"] < S["iterations"] and AR.errors(got["est"], truth)[0] < 0.05           # it stays at the truth


def test_a_degenerate_scene_and_the_refusals(sc, scene):
    cam, points, valid, truth = scene
    tx, ty, tz, rot = AR.scene_start(truth)
    none = np.zeros_like(valid)
    _put(sc, points, none)
    got = sc.refine_turntable_plane(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], EDGE, 2, iterations=20)
    assert got["n_done"] == 1 and got["degenerate"] and got["n"] == 0 and got["sources"] == 0 and math.isnan(got["rms_xz"])
    assert np.array_equal(got["est"], AR.first_estimate(tx, tz, rot)) and got["tx"] == tx and got["tz"] == tz
    _put(sc, points, valid)
    before = _planes(sc)
    ref = sc.refine_turntable_plane(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], EDGE, 2, iterations=3)
    Sc = pkg("scanner")
    nan, inf = float("nan"), float("inf")
    ok = dict(first=0, n=S["V"], tx=tx, ty=ty, tz=tz, rot=rot, rng=S["rng"], md=S["max_dist"], edge=EDGE, window=2, it=3)
    bad = [dict(n=1), dict(n=0), dict(n=-2), dict(n=S["V"] + 1), dict(first=-1), dict(first=3, n=2), dict(rng=0.0), dict(rng=nan), dict(rng=inf), dict(rng=-4.0),
           dict(md=0.0), dict(md=nan), dict(md=inf), dict(md=S["rng"] * 2), dict(edge=0.0), dict(edge=nan), dict(edge=inf), dict(edge=-1.0),
           dict(window=-1), dict(window=5), dict(it=0), dict(it=65), dict(it=-1), dict(tx=nan), dict(ty=inf), dict(tz=-inf), dict(rot=nan),
           dict(null_out=True)]
    for kw in bad:
        a = dict(ok, **kw)
        out, log, done = Sc.Turntable(), (Sc.AlignIteration * 64)(), C.c_int(-7)
        out.n, log[0].n = -7, -7
        rc = sc.L.sl3d_refine_turntable_plane(sc._h, a["first"], a["n"], a["tx"], a["ty"], a["tz"], a["rot"], a["rng"], a["md"], a["edge"], a["window"],
                                              a["it"], None if a.get("null_out") else C.byref(out), log, C.byref(done))
        assert rc == INVALID_ARG and out.n == -7 and log[0].n == -7 and done.value == -7, kw
    assert all(np.array_equal(a, b) for a, b in zip(_planes(sc), before))
    again = sc.refine_turntable_plane(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], EDGE, 2, iterations=3)
    assert np.array_equal(again["est"], ref["est"]) and again["n"] == ref["n"]                  # ... and the next call works as before
