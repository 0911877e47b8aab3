"""GPU tests of the voxel grid end to end (sl3d_voxel_grid with xyz_in == NULL: over the registered cloud a registration left on the
device): three synthetic views of ONE plane, each with its own noise seed and its own mask, at the frame size of
tests/test_gpu_next_rows.py's registration test.  Everything bit for bit against the restatement (tests/voxel_reference.py) over the
cloud the registration downloads; no tolerance anywhere.
A: rot_step = 0, the views overlap fully; leaf = four times the median distance between neighbouring points of view 0.  The restatement
   alone shows the case cannot pass on an identity: nothing dropped, fewer than n / 2 cells kept, cells that hold points of two views.
B: rot_step = 30 about an off-centre axis, both modes, min_points = 2, which removes some cells and not all.
C: through register_clouds after run_clouds: the same grid as through register_views.
D: filter_outliers, then the registration, then the grid: the rejected pixels are in no cell.
E: the scanner's state is untouched: cloud(v), points(v) and a second register_views are byte-identical before and after."""
import numpy as np
import pytest

from conftest import pkg

import voxel_reference as VR

pytestmark = pytest.mark.gpu

W, H, PW, PH, N, FW = 200, 96, 256, 256, 6, 4
PLANE = (1.0, 0.05, 0.03)
AXIS = (50.0, 30.0, -5.0)


@pytest.fixture(scope="module")
def captures():
    syn = pkg("synth")
    caps = [syn.make_capture(W, H, PW, PH, N, N, FW, FW, view=v, noise=1, plane=PLANE) for v in range(3)]
    rng = np.random.default_rng(23)
    masks = []
    for v, c in enumerate(caps):
        m = c["mask"].copy()
        m[rng.random((H, W)) < 0.02 * (v + 1)] = 0
        masks.append(m)
    return caps, masks


def _loaded(captures):
    S, syn = pkg("scanner"), pkg("synth")
    caps, masks = captures
    sc = S.Scanner(W, H, PW, PH, N, N, FW, FW, max_views=3)
    sc.set_calibration(*syn.cal_tuple(caps[0]["cal"]))
    for v, c in enumerate(caps):
        sc.set_mask(masks[v], view=v)
        sc.set_frames(0, c["planes_v"], view=v)
        sc.set_frames(1, c["planes_h"], view=v)
    return sc


@pytest.fixture(scope="module")
def sc(captures):
    with _loaded(captures) as s:
        s.run(0, 3)
        yield s


def _spacing(xyz, valid):
    """the median distance between neighbouring (next column) valid points of a view"""
    both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
    d = np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1].astype(np.float64), axis=-1)[both]
    assert len(d) > 1000
    return float(np.median(d))


@pytest.fixture(scope="module")
def leaf(sc):
    return float(np.float32(4.0 * _spacing(*sc.points(0))))


def _same(got, ref):
    assert got[3] == ref[3]
    assert got[0].shape == ref[0].shape and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[1])
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], ref[2])


def test_a_fully_overlapping_views(sc, leaf):
    counts = [len(sc.cloud(v)) for v in range(3)]
    reg = sc.register_views(0, 3, 0.0, 0.0, 0.0, 0.0)
    n = len(reg)
    assert n == sum(counts) and len(set(counts)) == 3
    ref = VR.grid(reg, leaf)
    # the case cannot pass on an identity, by the restatement alone
    assert ref[3][0] == n and ref[3][1] == 0                               # nothing is dropped
    assert 0 < ref[3][3] < n / 2                                           # far fewer cells than points
    ref0 = VR.grid(reg[:counts[0]], leaf)                                  # view 0 alone: the cells that appear first in view 0, with
    k = len(ref0[1])                                                       # their view-0 points only
    assert (ref[1][:k] < counts[0]).all() and np.array_equal(ref[1][:k], ref0[1])
    assert (ref[2][:k] > ref0[2]).sum() > k / 2                            # most of them hold points of another view as well
    assert not np.array_equal(ref[0][:k].view(np.uint32), ref0[0].view(np.uint32))
    for centroid in (True, False):
        _same(sc.voxel_grid(leaf, 1, centroid, stats=True), VR.grid(reg, leaf, 1, centroid))


@pytest.mark.parametrize("centroid", [True, False], ids=["centroid", "first"])
def test_b_turntable_with_min_points(sc, leaf, centroid):
    reg = sc.register_views(0, 3, *AXIS, 30.0)
    ref = VR.grid(reg, leaf, 2, centroid)
    assert ref[3][1] == 0 and 0 < ref[3][3] < ref[3][2]                    # min_points = 2 removes some cells and not all of them
    _same(sc.voxel_grid(leaf, 2, centroid, stats=True), ref)
    v, stats = sc.voxel_grid_device(leaf, 2, centroid)
    assert stats == ref[3] and v.xyz and v.first and v.count


def test_c_through_register_clouds(sc, leaf):
    reg = sc.register_views(0, 3, *AXIS, 30.0)
    via_views = sc.voxel_grid(leaf, 2, True, stats=True)
    sc.run_clouds(0, 3)
    reg_c = sc.register_clouds(0, 3, *AXIS, 30.0)
    assert np.array_equal(reg_c.view(np.uint32), reg.view(np.uint32))
    via_clouds = sc.voxel_grid(leaf, 2, True, stats=True)
    _same(via_clouds, via_views)
    _same(via_clouds, VR.grid(reg_c, leaf, 2, True))


def test_e_the_state_is_untouched(sc, leaf):
    sc.run(0, 3)
    before = [(sc.cloud(v), *sc.points(v)) for v in range(3)]
    reg = sc.register_views(0, 3, *AXIS, 30.0)
    for centroid in (True, False):
        sc.voxel_grid(leaf, 1, centroid)
        sc.voxel_grid(leaf, 1, centroid, cloud=reg[:777])                  # the host route does not touch the registered cloud either
        _same(sc.voxel_grid(leaf, 1, centroid, stats=True), VR.grid(reg, leaf, 1, centroid))
    for v, (cloud, xyz, valid) in enumerate(before):
        a, (b, c) = sc.cloud(v), sc.points(v)
        assert np.array_equal(a.view(np.uint32), cloud.view(np.uint32)) and np.array_equal(b.view(np.uint32), xyz.view(np.uint32))
        assert np.array_equal(c, valid)
    assert np.array_equal(sc.register_views(0, 3, *AXIS, 30.0).view(np.uint32), reg.view(np.uint32))


def test_d_after_the_outlier_filter(captures):
    with _loaded(captures) as s:
        s.run(0, 3)
        pts = [s.points(v) for v in range(3)]
        space = _spacing(*pts[0])
        leaf = float(np.float32(4.0 * space))
        counts = s.filter_outliers(2, 4.0 * space, 12, 0, 3)             # half of the 24 neighbours: pixels between mask holes go
        assert (counts[:, 1] > 0).all() and (counts[:, 1] < counts[:, 0]).all()
        rejected = np.concatenate([p[0][(p[1] == 1) & (s.points(v)[1] == 0)] for v, p in enumerate(pts)])
        assert len(rejected) == int(counts[:, 1].sum())
        reg = s.register_views(0, 3, 0.0, 0.0, 0.0, 0.0)                    # (rotation by 0 about the origin: the points' own bits)
        assert len(reg) == int((counts[:, 0] - counts[:, 1]).sum())
        kept = np.concatenate([p[0][s.points(v)[1] == 1] for v, p in enumerate(pts)])
        assert np.array_equal(reg.view(np.uint32), kept.view(np.uint32))
        for centroid in (True, False):
            got = s.voxel_grid(leaf, 1, centroid, stats=True)
            _same(got, VR.grid(reg, leaf, 1, centroid))
            assert got[3][0] == len(reg) and got[3][1] == 0 and int(got[2].sum()) == len(reg)   # every cell is made of kept pixels only
        # Through `first`: the pixel a cell's first point came from is a pixel the filter kept, and in first mode the cell's position is
        # that pixel's point.  (Point bits cannot tell a rejected pixel from a kept one: the views see one plane, and a pixel rejected
        # in one view often has the very same point in another, where it is kept.)
        after = np.stack([s.points(v)[1] for v in range(3)]).reshape(-1)
        was = np.stack([p[1] for p in pts]).reshape(-1)
        source = np.flatnonzero(after == 1)                                  # registered point i is pixel source[i] of views x rows x columns
        xyz, first, count = s.voxel_grid(leaf, 1, False)
        assert (after[source[first]] == 1).all() and not ((was == 1) & (after == 0))[source[first]].any()
        assert np.array_equal(xyz.view(np.uint32), np.concatenate([p[0].reshape(-1, 3) for p in pts])[source[first]].view(np.uint32))
