"""GPU tests (-m gpu) of sl3d_refine_turntable on the ray-cast scene of tests/test_align_recovery_reference.py: an ellipsoid off the
turntable axis and a sphere beside it, 160 x 120, 4 views, step 20 degrees, put into a context's dense planes through
tests/dense_planes.put_dense behind sc.run(); sc.synchronize(), ray-cast through the camera sl3d_get_align_camera hands out.

Every log entry is held to the restatement (tests/align_reference.py) on its own: the pass of the restatement AT THE ENTRY'S ESTIMATE gives
the entry's accepted pairs and sources exactly, its solve the entry's two rms and the next entry's estimate to 1e-12 relative (the host's
libm and some twenty double operations separate the two).  Then the loop as a whole against the restatement's loop: n_done, the
estimates, the result.  The early stop on views that are aligned already; register_views with the refined numbers; every byte of points,
valid, cloud, a previous registration and a previous voxel grid unchanged by the calls; every refusal leaves the last state."""
import ctypes as C
import math

import numpy as np
import pytest

import align_reference as AR
from conftest import pkg
from dense_planes import put_dense

pytestmark = pytest.mark.gpu

S = AR.SCENE
REL = 1e-12
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


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= REL * max(abs(b), 1e-300)


def _state(sc, leaf):
    """every byte a refinement must leave alone: the views' planes and clouds, the last voxel result, and the grid of the registered cloud"""
    out = []
    for v in range(S["V"]):
        xyz, valid = sc.points(v)
        out += [xyz.view(np.uint32), valid, sc.cloud(v).view(np.uint32)]
    out += [a.view(np.uint32) if a.dtype == np.float32 else a for a in sc._fill("sl3d_get_voxel_grid", (), (np.float32, 3), (np.int32,), (np.uint32,))]
    return out


def test_every_iteration_against_the_restatement(sc, scene):
    cam, points, valid, truth = scene
    _put(sc, points, valid)
    tx, ty, tz, rot = AR.scene_start(truth)
    args = (S["rng"], S["max_dist"], S["window"])
    got = sc.refine_turntable(0, S["V"], tx, ty, tz, rot, *args, iterations=S["iterations"])
    log = got["log"]
    assert got["n_done"] == len(log) and 1 <= len(log) <= S["iterations"]
    first = AR.first_estimate(tx, tz, rot)
    assert all(_close(a, b) for a, b in zip(log[0]["est"], first)) and np.array_equal(log[0]["est"][2:], first[2:])
    ox, oz = float(tx), float(tz)
    for i, entry in enumerate(log):
        words = AR.pass_sums(points, valid, cam, 0, 0, entry["est"], ox, oz, *args)
        nxt, stats = AR.solve(words, S["rng"], ox, oz, entry["est"])
        assert entry["n"] == stats["n"] == int(words[:, 0].sum()) and entry["sources"] == int(words[:, 11].sum()), i
        assert _close(entry["rms_xz"], stats["rms_xz"]) and _close(entry["rms_y"], stats["rms_y"]), i
        after = log[i + 1]["est"] if i + 1 < len(log) else got["est"]
        assert all(_close(a, b) for a, b in zip(after, nxt)), i
        assert np.array_equal(sc.align_sums(0, S["V"], entry["est"], ox, oz, *args), words), i       # (the pass itself, once more)
    # ... and the loop as a whole
    want = AR.refine(points, valid, cam, 0, 0, tx, ty, tz, rot, *args, S["iterations"])
    assert got["n_done"] == want["n_done"] and got["degenerate"] == want["degenerate"] is False
    for g, w in zip(log, want["log"]):
        assert all(_close(a, b) for a, b in zip(g["est"], w["est"])) and (g["n"], g["sources"]) == (w["n"], w["sources"])
        assert _close(g["rms_xz"], w["rms_xz"]) and _close(g["rms_y"], w["rms_y"])
    assert all(_close(a, b) for a, b in zip(got["est"], want["est"]))
    assert (got["n"], got["sources"]) == (want["n"], want["sources"]) and _close(got["rms_xz"], want["rms_xz"]) and _close(got["rms_y"], want["rms_y"])
    assert got["ty"] == ty and got["tx"] == np.float32(got["est"][2]) and got["tz"] == np.float32(got["est"][3])
    assert got["rot_step"] == np.float32(math.atan2(got["est"][1], got["est"][0]) * 180.0 * 7.0 / 22.0)
    # what the recovery test of the restatement asserts holds for the library's numbers too
    e0, e1 = AR.errors(log[0]["est"], truth), AR.errors(got["est"], truth)
    assert 2 * log[0]["n"] >= log[0]["sources"] and e1[0] < e0[0] and e1[1] < e0[1] and log[-1]["rms_xz"] < log[0]["rms_xz"]
    # fewer iterations: the same first entries; without a log and without n_done
    two = sc.refine_turntable(0, S["V"], tx, ty, tz, rot, *args, iterations=2)
    assert two["n_done"] == 2 and all(np.array_equal(a["est"], b["est"]) and a["n"] == b["n"] for a, b in zip(two["log"], log))
    out = pkg("scanner").Turntable()
    assert sc.L.sl3d_refine_turntable(sc._h, 0, S["V"], tx, ty, tz, rot, *args, 2, C.byref(out), None, None) == 0
    assert np.array_equal(np.array(out.est[:]), two["est"]) and out.n == two["n"]
    # the registration takes the refined numbers
    reg = sc.register_views(0, S["V"], got["tx"], got["ty"], got["tz"], got["rot_step"])
    assert len(reg) == int(valid.sum()) and np.isfinite(reg).all()
    assert np.allclose(reg[:int(valid[0].sum())], points[0][valid[0] == 1], rtol=0, atol=1e-3)                     # view 0 is not turned


def test_a_subset_of_the_views(sc, scene):
    cam, points, valid, truth = scene
    _put(sc, points, valid)
    tx, ty, tz, rot = AR.scene_start(truth)
    got = sc.refine_turntable(1, 3, tx, ty, tz, rot, S["rng"], S["max_dist"], 1, iterations=3)
    want = AR.refine(points[1:], valid[1:], cam, 0, 0, tx, ty, tz, rot, S["rng"], S["max_dist"], 1, 3)
    assert got["n_done"] == want["n_done"] == 3
    assert [(e["n"], e["sources"]) for e in got["log"]] == [(e["n"], e["sources"]) for e in want["log"]]
    assert all(_close(a, b) for a, b in zip(got["est"], want["est"]))


def test_the_early_stop_on_aligned_views(sc):
    cam = sc.align_camera()
    points, valid, est, _ = AR.crafted_views(cam, S["W"], S["H"], 0, 0, S["V"], 5, noise=0.0, outlier=0.0)
    _put(sc, points, valid)
    tx, tz, rot = np.float32(est[2]), np.float32(est[3]), AR.degrees_22_7(0.2)
    want = AR.refine(points, valid, cam, 0, 0, tx, 0.0, tz, rot, 256.0, 0.5, 2, 20)
    assert want["n_done"] == 2 and np.array_equal(want["log"][0]["n"], want["log"][1]["n"])     # by the restatement alone: the second pass repeats the first
    got = sc.refine_turntable(0, S["V"], tx, 0.0, tz, rot, 256.0, 0.5, 2, iterations=20)
    assert got["n_done"] == 2 and len(got["log"]) == 2 and not got["degenerate"]
    assert (got["n"], got["sources"]) == (want["n"], want["sources"]) and got["n"] > 0.9 * got["sources"]
    assert all(_close(a, b) for a, b in zip(got["est"], want["est"]))
    assert AR.errors(got["est"], est)[0] < 1e-3 and AR.errors(got["est"], est)[1] < 0.01
    # a degenerate solve ends the loop too: two views without a valid pixel
    none = np.zeros_like(valid)
    _put(sc, points, none)
    got = sc.refine_turntable(0, S["V"], tx, 0.0, tz, rot, 256.0, 0.5, 2, iterations=20)
    assert got["n_done"] == 1 and got["degenerate"] and got["n"] == 0 and got["sources"] == 0 and math.isnan(got["rms_xz"])
    assert np.array_equal(got["est"], AR.first_estimate(tx, tz, rot)) and got["tx"] == tx and got["tz"] == tz


def test_the_calls_change_nothing_and_every_refusal_leaves_the_state(sc, scene):
    cam, points, valid, truth = scene
    _put(sc, points, valid)
    tx, ty, tz, rot = AR.scene_start(truth)
    reg = sc.register_views(0, S["V"], tx, ty, tz, rot)
    grid = sc.voxel_grid(2.0, 1, True, stats=True)
    before = _state(sc, 2.0)
    got = sc.refine_turntable(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], S["window"], iterations=3)
    sc.align_sums(0, S["V"], got["est"], float(tx), float(tz), S["rng"], S["max_dist"], 4)
    sc.align_camera()

    def unchanged():
        assert all(np.array_equal(a, b) for a, b in zip(_state(sc, 2.0), before))
        again = sc.voxel_grid(2.0, 1, True, stats=True)                     # over the registered cloud as it lies on the device
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], grid[:3])) and again[3] == grid[3]
    unchanged()
    assert np.array_equal(sc.register_views(0, S["V"], tx, ty, tz, rot).view(np.uint32), reg.view(np.uint32))
    Sc = pkg("scanner")
    nan, inf = float("nan"), float("inf")
    ok = dict(first=0, n=S["V"], tx=tx, ty=ty, tz=tz, rot=rot, rng=S["rng"], md=S["max_dist"], window=2, it=3)
    bad = [dict(n=1), dict(n=0), dict(n=-2), dict(n=S["V"] + 1), dict(first=-1), dict(first=3, n=2), dict(rng=0.0), dict(rng=nan), dict(rng=inf), dict(rng=-4.0),
           dict(md=0.0), dict(md=nan), dict(md=inf), dict(md=S["rng"] * 2), dict(window=-1), dict(window=5), dict(it=0), dict(it=65), dict(it=-1),
           dict(tx=nan), dict(ty=inf), dict(tz=-inf), dict(rot=nan), dict(null_out=True)]
    for kw in bad:
        a = dict(ok, **kw)
        out, log, done = Sc.Turntable(), (Sc.AlignIteration * 64)(), C.c_int(-7)
        out.n, log[0].n = -7, -7
        rc = sc.L.sl3d_refine_turntable(sc._h, a["first"], a["n"], a["tx"], a["ty"], a["tz"], a["rot"], a["rng"], a["md"], a["window"], a["it"],
                                        None if a.get("null_out") else C.byref(out), log, C.byref(done))
        assert rc == INVALID_ARG and out.n == -7 and log[0].n == -7 and done.value == -7, kw
    unchanged()
    # ... and the next call works as before
    again = sc.refine_turntable(0, S["V"], tx, ty, tz, rot, S["rng"], S["max_dist"], S["window"], iterations=3)
    assert np.array_equal(again["est"], got["est"]) and again["n"] == got["n"]
