"""The crafted clouds of the voxel grid's tests: each is built for one thing the kernels (3dscan_amd/csrc/sl3d_voxel.hip) can get wrong.
tests/test_voxel_cases.py asserts on the CPU, with the restatement alone, that each contains what it is built for;
tests/test_gpu_voxel_cases.py sends every one through the host-cloud route of sl3d_voxel_grid, in both modes.

A case is (xyz float32 (n, 3), leaf, the min_points to run it with).  The geometry the clouds aim at: k_voxel_insert takes a point per
lane, 64 lanes a wave, 256 a block; the emission walks blocks of 1024 points, 4 per lane; the table has voxel_table_capacity(n) slots,
1024 for n <= 512."""
import numpy as np

import voxel_reference as VR

LEAF = 0.5
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)


def in_cells(cells, rng, leaf=LEAF):
    """a float32 point strictly inside each of the (n, 3) integer cells"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return ((cells + rng.uniform(0.1, 0.9, cells.shape)) * np.float64(np.float32(leaf))).astype(np.float32)


def distinct_cells(n, offset=0):
    """n distinct cells on a 3-D lattice, negative indices among them"""
    i = np.arange(n) + offset
    return np.stack([i % 37 - 18, (i // 37) % 41 - 20, i // (37 * 41) - 1], axis=1)


def blob(n, seed):
    """n points of a small box: about 1700 cells, so that cells hold several points and lanes next to each other rarely share one"""
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (n, 3)).astype(np.float32)


def runs_case():
    """2100 points in distinct cells, but for four runs of one cell each: across a wave boundary (lanes 50 .. 80), across a 256-point
    block of the insertion (250 .. 260), across a 1024-point block of the emission (1000 .. 1050), and the whole of one wave (1280 .. 1343)"""
    rng = np.random.default_rng(5)
    cells = distinct_cells(2100)
    for lo, hi in RUNS:
        cells[lo:hi + 1] = cells[lo]
    return in_cells(cells, rng)


RUNS = ((50, 80), (250, 260), (1000, 1050), (1280, 1343))


def colliding_cells(home, count, capacity=1024):
    """`count` cells (cx, cy, 0), 0 <= cx, cy < 1024, whose home slot in a table of `capacity` slots is `home`"""
    g = np.stack(np.meshgrid(np.arange(1024), np.arange(1024), [0], indexing="ij"), -1).reshape(-1, 3)
    hits = g[VR.home_slot(VR.key(g), capacity) == home]
    assert len(hits) >= count, len(hits)
    return hits[:count]


def dropped_case():
    """a blob with points that are no samples in between: NaN and infinities in any coordinate, the first index out of range on either
    side, a huge coordinate; at the cloud's first and last place, alone and in runs"""
    rng = np.random.default_rng(9)
    xyz = blob(1500, 8)
    limit = np.float32((1 << 20) * LEAF)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [limit, 0, 0], [0, np.nextafter(-limit, np.float32(-np.inf)), 0],
                    [1e30, 1, 1], [np.nan, np.nan, np.nan], [0, -1e30, 0]], dtype=np.float32)
    at = np.unique(np.concatenate([[0, 1499], np.arange(60, 70), np.arange(1020, 1030), rng.integers(0, 1500, 40)]))
    xyz[at] = bad[np.arange(len(at)) % len(bad)]
    return xyz, at


def counts_case():
    """cells of 1, 2, 3, 3 and 5 points, shuffled: min_points 1, 3 (the exact count of two cells) and 4 (one above)"""
    rng = np.random.default_rng(13)
    cells = np.repeat(distinct_cells(5, 100), [1, 2, 3, 3, 5], axis=0)
    return in_cells(cells[rng.permutation(len(cells))], rng)


def interleaved_case(k):
    """1200 points that go round k cells: ABAB.. for k = 2 -- no two neighbouring lanes share a cell, no run collapses"""
    rng = np.random.default_rng(20 + k)
    return in_cells(distinct_cells(k, 7)[np.arange(1200) % k], rng)


def last_first_case():
    """1027 points of a blob, the last one alone in a cell nobody else is in: a cell whose first point is the last point of the cloud"""
    xyz = blob(1027, 3)
    xyz[-1] = (40.25, -40.25, 40.25)
    return xyz


def all_cases():
    rng = np.random.default_rng(1)
    cases = {f"n{n}": (blob(n, 100 + n), LEAF, (1, 2)) for n in SIZES}
    cases["runs"] = (runs_case(), LEAF, (1, 12))
    cases["one_cell_5000"] = (in_cells(np.tile([[3, -2, 1]], (5000, 1)), rng), LEAF, (1, 5000, 5001))
    cases["distinct_3000"] = (in_cells(distinct_cells(3000), rng), LEAF, (1, 2))
    cases["last_is_first"] = (last_first_case(), LEAF, (1,))
    cases["collide_300"] = (in_cells(colliding_cells(512, 300), rng), LEAF, (1,))
    cases["collide_wrap"] = (in_cells(np.repeat(colliding_cells(1021, 300), 1 + np.arange(300) % 2, axis=0)[:512], rng), LEAF, (1, 2))
    cases["dropped"] = (dropped_case()[0], LEAF, (1, 2))
    cases["counts"] = (counts_case(), LEAF, (1, 3, 4))
    cases["abab"] = (interleaved_case(2), LEAF, (1, 601))
    cases["abcabc"] = (interleaved_case(3), LEAF, (1, 400, 401))
    cases["fine_leaf"] = (blob(1500, 4), 0.01, (1,))           # nearly every point its own cell
    cases["coarse_leaf"] = (blob(1500, 4), 64.0, (1,))         # 8 cells around the origin
    return cases
