"""GPU tests of the voxel grid on the crafted clouds (tests/voxel_cases.py, what each is built for: tests/test_voxel_cases.py): every
cloud through the host-cloud route of sl3d_voxel_grid, in both modes and with every min_points of the case, bit for bit against the
restatement (tests/voxel_reference.py) -- xyz as uint32, first, count and the four counts; no tolerance anywhere.  Then the call's
protocol: the same input twice gives the same bytes, a smaller cloud after a larger one reuses the table, sl3d_get_voxel_grid with null
outputs, a short and a full capacity, SL3D_E_STATE before any call and without a registered cloud, refusals that leave the last result
untouched."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

import voxel_cases as VC
import voxel_reference as VR

pytestmark = pytest.mark.gpu

CASES = VC.all_cases()
E_INVALID_ARG, E_STATE = -1, -4   # SL3D_E_INVALID_ARG, SL3D_E_STATE of include/sl3d.h


@pytest.fixture(scope="module")
def S():
    return pkg("scanner")


@pytest.fixture(scope="module")
def sc(S):
    with S.Scanner(64, 48, 64, 48, 5, 5, 2, 2) as s:
        yield s


@pytest.fixture(scope="module")
def want():
    """the restatement of every (case, min_points, mode), computed once"""
    return {(name, m, cen): VR.grid(xyz, leaf, m, cen) for name, (xyz, leaf, mins) in CASES.items() for m in mins for cen in (False, True)}


def _same(got, ref):
    xyz, first, count, stats = got
    rxyz, rfirst, rcount, rstats = ref
    assert stats == rstats
    assert xyz.dtype == np.float32 and first.dtype == np.int32 and count.dtype == np.uint32
    assert xyz.shape == rxyz.shape and np.array_equal(xyz.view(np.uint32), rxyz.view(np.uint32))
    assert np.array_equal(first, rfirst) and np.array_equal(count, rcount)


def test_the_status_codes_are_the_headers():
    import os
    import re
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "sl3d.h")).read()
    assert int(re.search(r"SL3D_E_INVALID_ARG\s*=\s*(-?\d+)", txt).group(1)) == E_INVALID_ARG
    assert int(re.search(r"SL3D_E_STATE\s*=\s*(-?\d+)", txt).group(1)) == E_STATE


def test_state_before_any_call(S):
    with S.Scanner(64, 48, 64, 48, 5, 5, 2, 2) as fresh:
        n, counts = C.c_int64(-7), (C.c_int64 * 4)(*([-7] * 4))
        assert fresh.L.sl3d_get_voxel_grid(fresh._h, None, None, None, 0, C.byref(n)) == E_STATE and n.value == -7
        # no registration has run: the registered cloud cannot be taken, and the refusal leaves "no result" as it is
        assert fresh.L.sl3d_voxel_grid(fresh._h, None, 0, 0.5, 1, 1, None, counts) == E_STATE and list(counts) == [-7] * 4
        assert fresh.L.sl3d_get_voxel_grid(fresh._h, None, None, None, 0, C.byref(n)) == E_STATE
        xyz, leaf, _ = CASES["counts"]
        _same(fresh.voxel_grid(leaf, cloud=xyz, stats=True), VR.grid(xyz, leaf))


@pytest.mark.parametrize("centroid", [False, True], ids=["first", "centroid"])
@pytest.mark.parametrize("name", list(CASES))
def test_crafted_cloud(sc, want, name, centroid):
    xyz, leaf, mins = CASES[name]
    for m in mins:
        got = sc.voxel_grid(leaf, m, centroid, cloud=xyz, stats=True)
        _same(got, want[(name, m, centroid)])
        again = sc.voxel_grid(leaf, m, centroid, cloud=xyz, stats=True)           # the same input: the same bytes
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]


def test_the_modes_differ_where_they_should(sc, want):
    a, b = want[("n2049", 1, False)], want[("n2049", 1, True)]
    many = a[2] > 1
    assert many.any() and (~many).any() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[0][~many].view(np.uint32), b[0][~many].view(np.uint32)) and (a[0][many] != b[0][many]).any(axis=1).all()


def test_a_smaller_cloud_after_a_larger_one(sc, want):
    """the table and the buffers of the larger call are kept and initialised anew"""
    for big, small in (("one_cell_5000", "counts"), ("distinct_3000", "collide_wrap"), ("n2049", "n1"), ("n2049", "n0"), ("n0", "n65")):
        for cen in (True, False):
            _same(sc.voxel_grid(CASES[big][1], 1, cen, cloud=CASES[big][0], stats=True), want[(big, 1, cen)])
            _same(sc.voxel_grid(CASES[small][1], 1, cen, cloud=CASES[small][0], stats=True), want[(small, 1, cen)])


def test_the_getter_sizes_then_fills(sc, want):
    xyz, leaf, _ = CASES["n1025"]
    ref = want[("n1025", 1, True)]
    m = len(ref[1])
    v, counts = sc.voxel_grid_device(leaf, 1, True, cloud=xyz)
    assert counts == ref[3] and v.xyz and v.first and v.count
    get, n = sc.L.sl3d_get_voxel_grid, C.c_int64(0)
    assert get(sc._h, None, None, None, 0, C.byref(n)) == 0 and n.value == m             # null outputs: the total
    assert get(sc._h, None, None, None, m, C.byref(n)) == 0 and n.value == m
    short = m // 3
    pos, first, count = np.full((m, 3), 7.0, np.float32), np.full(m, -7, np.int32), np.full(m, 7, np.uint32)
    assert get(sc._h, pos.ctypes.data, first.ctypes.data, count.ctypes.data, short, C.byref(n)) == 0 and n.value == m
    assert np.array_equal(pos[:short].view(np.uint32), ref[0][:short].view(np.uint32)) and (pos[short:] == 7.0).all()   # rows past it untouched
    assert np.array_equal(first[:short], ref[1][:short]) and (first[short:] == -7).all()
    assert np.array_equal(count[:short], ref[2][:short]) and (count[short:] == 7).all()
    only = np.full(m, -7, np.int32)                                                       # one output alone, at full capacity
    assert get(sc._h, None, only.ctypes.data, None, m + 100, C.byref(n)) == 0 and n.value == m and np.array_equal(only, ref[1])
    assert get(sc._h, None, None, None, -1, C.byref(n)) == E_INVALID_ARG and get(sc._h, None, None, None, 0, None) == E_INVALID_ARG
    _same((*sc._fill("sl3d_get_voxel_grid", (), (np.float32, 3), (np.int32,), (np.uint32,)), counts), ref)


def test_asynchronous_call_without_counts(sc, want):
    xyz, leaf, _ = CASES["dropped"]
    a = np.ascontiguousarray(xyz)
    assert sc.L.sl3d_voxel_grid(sc._h, a.ctypes.data, len(a), leaf, 2, 1, None, None) == 0
    ref = want[("dropped", 2, True)]
    _same((*sc._fill("sl3d_get_voxel_grid", (), (np.float32, 3), (np.int32,), (np.uint32,)), ref[3]), ref)


def test_every_refusal_leaves_the_last_result(sc, want):
    xyz, leaf, _ = CASES["counts"]
    ref = want[("counts", 3, True)]
    _same(sc.voxel_grid(leaf, 3, True, cloud=xyz, stats=True), ref)
    a = np.ascontiguousarray(CASES["n65"][0])
    grid = sc.L.sl3d_voxel_grid
    bad = [dict(leaf=float("nan")), dict(leaf=float("inf")), dict(leaf=0.0), dict(leaf=-0.5), dict(min_points=0), dict(min_points=-3),
           dict(flags=2), dict(flags=0x80000001), dict(n=-1), dict(n=1 << 31), dict(n=1 << 40)]
    for kw in bad:
        counts = (C.c_int64 * 4)(*([-7] * 4))
        rc = grid(sc._h, a.ctypes.data, kw.get("n", len(a)), kw.get("leaf", 0.5), kw.get("min_points", 1), kw.get("flags", 1), None, counts)
        assert rc == E_INVALID_ARG and list(counts) == [-7] * 4, kw
        _same((*sc._fill("sl3d_get_voxel_grid", (), (np.float32, 3), (np.int32,), (np.uint32,)), ref[3]), ref)
    # no registration on this context either: SL3D_E_STATE, and the result is still the last one
    assert grid(sc._h, None, 0, 0.5, 1, 1, None, None) == E_STATE
    _same((*sc._fill("sl3d_get_voxel_grid", (), (np.float32, 3), (np.int32,), (np.uint32,)), ref[3]), ref)
