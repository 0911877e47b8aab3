"""CPU tests of the crafted clouds of the voxel grid (tests/voxel_cases.py): each contains what it is built for, by the restatement
(tests/voxel_reference.py) alone -- the GPU tests (tests/test_gpu_voxel_cases.py) then hold the kernels to the restatement on them."""
import numpy as np
import pytest

import voxel_cases as VC
import voxel_reference as VR


@pytest.fixture(scope="module")
def cases():
    return VC.all_cases()


def _keys(xyz, leaf):
    c, ok = VR.cell(xyz, leaf)
    sample = np.isfinite(xyz).all(axis=1) & ok.all(axis=1)
    k = np.full(len(xyz), VR.EMPTY, dtype=np.uint64)
    k[sample] = VR.key(c[sample])
    return k, sample


def test_the_sizes_and_the_shapes(cases):
    assert VC.SIZES == (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
    for n in VC.SIZES:
        xyz, leaf, mins = cases[f"n{n}"]
        assert xyz.shape == (n, 3) and xyz.dtype == np.float32
        pos, first, count, stats = VR.grid(xyz, leaf)
        assert stats[0] == n and stats[1] == 0 and int(count.sum()) == n
        if n >= 1023:
            assert (count > 1).any() and (count == 1).any() and VR.grid(xyz, leaf, 2)[3][3] < stats[3]
    for name, (xyz, leaf, mins) in cases.items():
        assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] == 3 and 1 in mins, name


def test_the_runs_cross_a_wave_and_a_block(cases):
    xyz, leaf, mins = cases["runs"]
    k, sample = _keys(xyz, leaf)
    assert sample.all()
    head = np.concatenate([[True], k[1:] != k[:-1]])
    for lo, hi in VC.RUNS:
        assert (k[lo:hi + 1] == k[lo]).all() and head[lo] and head[hi + 1] and not head[lo + 1:hi + 1].any()
        assert (k == k[lo]).sum() == hi - lo + 1                          # the run is the whole cell
    (a, b), (c, d), (e, f), (g, h) = VC.RUNS
    assert a // 64 != b // 64 and c // 256 != d // 256 and e // 1024 != f // 1024 and (g % 64, h % 64) == (0, 63)
    assert head.sum() == len(xyz) - sum(hi - lo for lo, hi in VC.RUNS)   # every other point is alone in its cell
    assert VR.grid(xyz, leaf, 12)[3][3] == 3                              # min_points 12 keeps the runs of 31, 51 and 64, drops the one of 11


def test_one_cell_and_distinct_cells(cases):
    xyz, leaf, mins = cases["one_cell_5000"]
    pos, first, count, stats = VR.grid(xyz, leaf)
    assert stats == [5000, 0, 1, 1] and first[0] == 0 and count[0] == 5000 and mins == (1, 5000, 5001)
    assert VR.grid(xyz, leaf, 5000)[3][3] == 1 and VR.grid(xyz, leaf, 5001)[3][3] == 0
    assert not np.array_equal(pos[0], xyz[0]) and not np.array_equal(pos[0], VR.grid(xyz, leaf, 1, False)[0][0])
    xyz, leaf, mins = cases["distinct_3000"]
    pos, first, count, stats = VR.grid(xyz, leaf)
    assert stats == [3000, 0, 3000, 3000] and np.array_equal(first, np.arange(3000)) and (count == 1).all()
    assert np.array_equal(pos.view(np.uint32), xyz.view(np.uint32))       # a one-point cell gives its point's bits, in both modes


def test_a_cell_whose_first_point_is_the_last(cases):
    xyz, leaf, mins = cases["last_is_first"]
    pos, first, count, stats = VR.grid(xyz, leaf)
    assert len(xyz) % 4 and first[-1] == len(xyz) - 1 and count[-1] == 1


def test_the_collisions(cases):
    hits = VC.colliding_cells(1021, 1)
    g = np.stack(np.meshgrid(np.arange(1024), np.arange(1024), [0], indexing="ij"), -1).reshape(-1, 3)
    assert 850 <= (VR.home_slot(VR.key(g), 1024) == 1021).sum() <= 1200 and len(hits) == 1   # about 1,000 of 2^20 cells per home slot
    for name, home in (("collide_300", 512), ("collide_wrap", 1021)):
        xyz, leaf, mins = cases[name]
        k, sample = _keys(xyz, leaf)
        assert sample.all() and len(xyz) <= 512 and VR.table_capacity(len(xyz)) == 1024
        u = np.unique(k)
        assert len(u) == 300 and (VR.home_slot(u, 1024) == home).all()
    assert 512 + 300 <= 1024 < 1021 + 300                                  # the second chain wraps past the end of the table
    xyz, leaf, mins = cases["collide_wrap"]
    assert sorted(set(VR.grid(xyz, leaf)[2].tolist())) == [1, 2]


def test_the_dropped_points(cases):
    xyz, leaf, mins = cases["dropped"]
    bad_xyz, at = VC.dropped_case()
    k, sample = _keys(xyz, leaf)
    assert np.array_equal(np.flatnonzero(~sample), at) and 0 in at and len(xyz) - 1 in at and len(at) > 50
    assert np.isnan(xyz[at]).any() and np.isinf(xyz[at]).any() and np.isfinite(xyz[at]).all(axis=1).any()   # out of range, yet finite
    pos, first, count, stats = VR.grid(xyz, leaf)
    assert stats[1] == len(at) and not np.isin(first, at).any() and int(count.sum()) == len(xyz) - len(at)


def test_min_points_at_below_and_above_a_count(cases):
    xyz, leaf, mins = cases["counts"]
    assert mins == (1, 3, 4)
    assert sorted(VR.grid(xyz, leaf, 1)[2].tolist()) == [1, 2, 3, 3, 5]
    assert sorted(VR.grid(xyz, leaf, 3)[2].tolist()) == [3, 3, 5] and VR.grid(xyz, leaf, 4)[2].tolist() == [5]
    pos, first, count, stats = VR.grid(xyz, leaf, 3)
    assert (np.diff(first) > 0).all() and stats[2] == 5 and stats[3] == 3


def test_the_interleaved_cells(cases):
    for name, cells in (("abab", 2), ("abcabc", 3)):
        xyz, leaf, mins = cases[name]
        k, sample = _keys(xyz, leaf)
        assert sample.all() and (k[1:] != k[:-1]).all() and len(np.unique(k)) == cells
        pos, first, count, stats = VR.grid(xyz, leaf)
        assert first.tolist() == list(range(cells)) and (count == 1200 // cells).all()
        assert VR.grid(xyz, leaf, mins[1])[3][3] == (cells if mins[1] <= 1200 // cells else 0)
    assert VR.grid(*cases["fine_leaf"][:2])[3][3] > 1400 and VR.grid(*cases["coarse_leaf"][:2])[3][3] == 8


def test_the_restatement_is_the_rule_in_plain_python(cases):
    """the vectorised restatement against a dictionary walk over the points, on the case with everything in it"""
    for name in ("dropped", "counts", "n1025"):
        xyz, leaf, mins = cases[name]
        L = float(np.float32(leaf))
        cells = {}
        for i, p in enumerate(xyz):
            if not np.isfinite(p).all():
                continue
            c = [float(np.floor(float(v) / L)) for v in p]
            if not all(-(1 << 20) <= v < 1 << 20 for v in c):
                continue
            cells.setdefault(tuple(c), []).append(i)
        for m in mins:
            pos, first, count, stats = VR.grid(xyz, leaf, m)
            kept = [(ix[0], len(ix), c) for c, ix in cells.items() if len(ix) >= m]
            assert [f for f, _, _ in kept] == first.tolist() and [n for _, n, _ in kept] == count.tolist()   # (dicts keep insertion order)
            assert stats[2] == len(cells)
            for (f, n, c), got in zip(kept, pos):
                if n == 1:
                    assert np.array_equal(got.view(np.uint32), xyz[f].view(np.uint32))
                    continue
                for j in range(3):
                    base = c[j] * L
                    S = sum(int(np.rint(((float(xyz[i, j]) - base) / L) * 16777216.0)) for i in cells[c])
                    assert np.float32(base + ((float(S) / float(n)) / 16777216.0) * L) == got[j]
