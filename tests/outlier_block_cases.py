"""The inputs of the outlier filter's tests past the first block (tests/test_outlier_block_cases.py on the CPU,
tests/test_gpu_outlier_blocks.py on the device).  Inputs only: this module imports no scanner.

k_outlier_apply: quad t of a view is quad (t mod lpr) of window row (t / lpr), lpr = ceil(W / 4); a block owns OUTLIER_APPLY_RUNS runs of
256 consecutive quads.  k_outlier_support: a block owns a tile of OUTLIER_TILE_W x OUTLIER_TILE_H window pixels.  The three numbers are
read from the TEXT of 3dscan_amd/csrc/sl3d_outlier.hip, not written down a second time: when the kernel's blocking changes, the table
below loses the properties its cases are labelled with and tests/test_outlier_block_cases.py fails.

CASES    (W, H, radius, max_dist, min_neighbours, content, labels), the contents those of outlier_reference.crafted_cases and `torus`.
         Labels: `multi` (two or more apply blocks), `mixed` (every apply block holds a rejected and a kept sample in the restatement),
         one of BLOCK_KINDS where the shape is in the table for its block count, `edge_w` / `edge_h` (the window's right / lower edge is a
         tile edge of k_outlier_support), `line` (one row or one column: PARAMS would reject everything, a line has at most 2 * radius
         neighbours, so the rule is scaled to the line).
torus    the `holes` case with its points rolled by half the width where W is a multiple of 16 (the pitch is W: no padding column, the
         pixel behind a row's last is the next row's first) and by half the height where H is a multiple of the tile height: the points
         beyond such an edge, wrapped around, lie next to the edge's own, so a neighbourhood that is not clipped there counts them
         (support_beyond: the restatement over the plane continued that way)."""
import itertools
import os
import re

import numpy as np

import outlier_reference as OR

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dscan_amd", "csrc", "sl3d_outlier.hip")
INF = float("inf")


def _define(name):
    with open(SOURCE) as f:
        found = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*$" % name, f.read(), re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


RUNS, TILE_W, TILE_H = _define("OUTLIER_APPLY_RUNS"), _define("OUTLIER_TILE_W"), _define("OUTLIER_TILE_H")
RUN_QUADS = 256                              # the quads of one run: a lane each (__launch_bounds__(256))
BLOCK_QUADS = RUN_QUADS * RUNS


# ---- the launch geometry --------------------------------------------------------------------------------------------------------------------
def quads(W, H):
    return (W + 3) // 4 * H


def apply_block(W, r, c):
    """the block of k_outlier_apply that owns pixel (r, c) (integers or arrays): quad t = r * ceil(W / 4) + c // 4, block = t // (256 * runs)"""
    return (np.asarray(r) * ((W + 3) // 4) + np.asarray(c) // 4) // BLOCK_QUADS


def apply_blocks(W, H):
    """int [H][W]: apply_block of every window pixel"""
    r, c = np.mgrid[0:H, 0:W]
    return apply_block(W, r, c)


def n_apply_blocks(W, H):
    return (quads(W, H) + BLOCK_QUADS - 1) // BLOCK_QUADS


def last_run(W, H):
    """the run of the last block in which the view's last quad lies: the `break` comes in the run behind it"""
    return (quads(W, H) - 1) % BLOCK_QUADS // RUN_QUADS


def support_grid(W, H):
    """(tiles across, tiles down) of k_outlier_support"""
    return (W + TILE_W - 1) // TILE_W, (H + TILE_H - 1) // TILE_H


def seam_row_cells(W, H, n=10):
    """n cells of one row, one pixel apart, half of them in apply block 0 and half in block 1: the row in which block 1 begins"""
    flat = apply_blocks(W, H).ravel()
    first = int(np.argmax(flat == 1))
    assert flat[first] == 1, "the shape has a second block"
    r, c = divmod(first, W)
    assert n // 2 <= c <= W - (n - n // 2), "block 1 begins inside a row, far enough from both ends"
    return [(r, k) for k in range(c - n // 2, c - n // 2 + n)]


# ---- the contents ---------------------------------------------------------------------------------------------------------------------------
def rolls(W, H):
    """(columns, rows) the torus content is rolled by"""
    return (W // 2 if W % 16 == 0 else 0), (H // 2 if H % TILE_H == 0 else 0)


def content(name, W, H):
    """(xyz float32 [H][W][3], valid uint8 [H][W])"""
    cases = {n: (xyz, valid) for n, xyz, valid in OR.crafted_cases(H, W)}
    if name != "torus":
        return cases[name]
    xyz, valid = cases["holes"]
    dc, dr = rolls(W, H)
    return np.ascontiguousarray(np.roll(xyz, (dr, dc), axis=(0, 1))), valid


def support_beyond(xyz, valid, radius, max_dist, columns, rows):
    """The restatement's support plane if the neighbourhood were NOT clipped at the window's left and right edges (`columns`: the pixel
    behind a row's last is the next row's first, as in memory when the pitch is W) and / or at its upper and lower edges (`rows`: the row
    behind the last is the first)."""
    H, W = valid.shape
    R = radius
    r, c = np.mgrid[-R:H + R, -R:W + R]
    inside = ((c >= 0) & (c < W) | bool(columns)) & ((r >= 0) & (r < H) | bool(rows))
    at = ((r % H) * W + c) % (H * W)
    ext_xyz = xyz.reshape(H * W, 3)[at]
    ext_valid = np.where(inside, valid.reshape(H * W)[at], 0).astype(np.uint8)
    return OR.support_plane(np.ascontiguousarray(ext_xyz), ext_valid, radius, max_dist)[R:R + H, R:R + W]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
BLOCK_KINDS = ("exact_multiple", "break_in_run_0", "break_in_a_later_run", "three_blocks")
LINE_RULES = ((2, 1.5, 2), (1, 1.0, 1))
ROW_SHAPE, COLUMN_SHAPE = (8240, 1), (1, 2060)
BATCH_SHAPE = (130, 125)
# shape -> (labels of the shape, [(rule, content, labels of the case)])
_P = OR.PARAMS
_TABLE = {
    (64, 128): (("exact_multiple", "edge_w", "edge_h"), [(_P[1], "holes", ("mixed",)), (_P[4], "step", ("mixed",)), (_P[4], "all_valid", ()), (_P[2], "torus", ())]),
    (64, 129): (("multi", "break_in_run_0", "edge_w"), [(_P[1], "holes", ("mixed",)), (_P[4], "step", ("mixed",)), (_P[4], "all_valid", ()),
                                                         (_P[2], "torus", ())]),
    (257, 33): (("multi", "break_in_run_0"), [(_P[1], "holes", ("mixed",)), (_P[4], "step", ("mixed",)), (_P[2], "holes", ("mixed",)),
                                               (_P[3], "none_valid", ())]),
    (130, 125): (("multi", "three_blocks", "break_in_run_0"),
                 [(_P[1], "holes", ("mixed",)), (_P[4], "step", ("mixed",)), (_P[3], "step", ("mixed",)), ((2, 1.5, 0), "holes", ()),
                  ((4, INF, OR.max_support(4)), "all_valid", ()), (_P[2], "corners", ())]),
    (130, 80): (("multi", "break_in_a_later_run", "edge_h"), [(_P[1], "holes", ("mixed",)), (_P[4], "step", ("mixed",)), (_P[1], "torus", ())]),
    ROW_SHAPE: (("multi", "line", "break_in_run_0"), [(rule, "holes", ("mixed",)) for rule in LINE_RULES]),
    COLUMN_SHAPE: (("multi", "line", "break_in_run_0"), [(rule, "holes", ("mixed",)) for rule in LINE_RULES]),
    (64, 8): (("edge_w", "edge_h"), [(_P[1], "torus", ()), (_P[4], "torus", ()), (_P[2], "holes", ())]),
    (128, 16): (("edge_w", "edge_h"), [(_P[1], "torus", ()), (_P[4], "torus", ()), (_P[3], "step", ())]),
    (65, 8): (("edge_h",), [(_P[1], "torus", ()), (_P[4], "torus", ()), (_P[2], "step", ())]),
    (64, 9): (("edge_w",), [(_P[1], "torus", ()), (_P[4], "torus", ()), (_P[2], "step", ())]),
}
SHAPES = tuple(_TABLE)
CASES = tuple((W, H) + rule + (name, shape_labels + labels) for (W, H), (shape_labels, rows) in _TABLE.items() for rule, name, labels in rows)
LARGEST = 130 * 125                           # pixels of the largest input


def cases_of(shape):
    return [c for c in CASES if c[:2] == tuple(shape)]


def restated(case):
    """outlier_reference.filter_outliers of a case of the table"""
    W, H, radius, max_dist, min_n, name, _ = case
    return OR.filter_outliers(*content(name, W, H), radius, max_dist, min_n)


def block_counts(case):
    """[(samples, rejected)] of the restatement per apply block"""
    W, H = case[:2]
    f, blocks = restated(case), apply_blocks(W, H)
    sample = f["support"] != OR.NO_SAMPLE
    return [(int((sample & (blocks == b)).sum()), int((f["rejected"] & (blocks == b)).sum())) for b in range(n_apply_blocks(W, H))]


def subset_sums(per_block):
    """the (samples, rejected) sums over every proper subset of the blocks, the empty one included"""
    n = len(per_block)
    return [tuple(int(x) for x in np.sum([per_block[b] for b in pick] + [(0, 0)], axis=0))
            for k in range(n) for pick in itertools.combinations(range(n), k)]
