"""Crafted candidate maps and planes for the hole filling, shared by the CPU test (tests/test_mesh_holes_arith.py: every case goes
through the host header) and the GPU test (tests/test_gpu_mesh_holes.py: every case is written into a context's dense planes).  A case is

    (name, xyz float32 (H, W, 3), valid uint8 (H, W) of 0/1, [(max_hole, fill_edge), ...])

SHAPES are the smallest (H, W) at which the kernels' indexing can go wrong: the quad, the pitch of 16, the wave seam at column 256, the
chunk seam at 1024, widths 4k + 1, one row, one column (no interior: nothing is filled there).

The feature map (features) cuts these out of a full frame; what does not fit a shape is clipped by it and then touches its border:
  tiny        (1, 1..2): the only interior a 3 x 5 frame has
  quad        rows 2-3 x columns 3-5: 6 pixels across the quad seam at column 4
  wave        rows 1-2 x columns 254-258: across the wave seam at column 256
  chunk       rows 4-6 x columns 1022-1026: 15 pixels = MAX_HOLE across the chunk seam at 1024 (filled)
  too_large   rows 4-7 x columns 40-43: 16 pixels = MAX_HOLE + 1 (not filled; filled at MAX_HOLE_LARGE)
  borders     holes that touch row 0, row H-1, column 0, column W-1 and a corner (never filled)
  corner      rows 1-3 x columns 100-102 and rows 4-6 x columns 103-105: 9 pixels each, meeting at a corner -- 18 together
  annulus     rows 2-4 x columns 120-122 around the candidate (3, 121): 8 pixels, every one with the island on one side
  u_shape     columns 140 and 144 of rows 2-5 joined along row 5: 11 pixels
  wall        a hole one candidate away from a hole that touches the border
"""
import numpy as np

import mesh_cases as MC
from mesh_components_reference import serpentine

INF = float("inf")
SHAPES = [(3, 5), (4, 257), (9, 1021), (9, 1025), (9, 2049), (33, 1), (1, 33), (2, 17)]
MAX_HOLE, MAX_HOLE_LARGE = 15, 40
SERPENTINE_SHAPE = (38, 2049)
FEATURES = {
    "tiny": [(1, 2, 1, 3)],
    "quad": [(2, 4, 3, 6)],
    "wave": [(1, 3, 254, 259)],
    "chunk": [(4, 7, 1022, 1027)],
    "too_large": [(4, 8, 40, 44)],
    "borders": [(0, 2, 60, 62), (7, 9, 70, 72), (4, 6, 0, 2), (7, 9, 0, 2)],
    "corner": [(1, 4, 100, 103), (4, 7, 103, 106)],
    "annulus": [(2, 5, 120, 123)],
    "u_shape": [(2, 6, 140, 141), (2, 6, 144, 145), (5, 6, 140, 145)],
    "wall": [(0, 3, 160, 162), (1, 3, 163, 165)],
}


def features(H, W):
    m = np.ones((H, W), np.uint8)
    for rects in FEATURES.values():
        for r0, r1, c0, c1 in rects:
            m[r0:r1, c0:c1] = 0
    if H > 3 and W > 121:
        m[3, 121] = 1                                   # the island
    if H > 5 and W > 2:
        m[4:6, W - 2:] = 0                              # column W-1
    return m


def _nonfinite_rim(xyz, valid):
    """NaN, +inf, -inf, 1e30 and a mixed triple on candidates next to the holes (a pixel that is no candidate is left alone)"""
    H, W = valid.shape
    kinds = [(np.nan, None, None), (None, np.inf, None), (None, None, -np.inf), (1e30, None, None), (np.nan, np.inf, -np.inf)]
    spots = [(1, 3), (2, 2), (4, 3), (2, 6), (0, 255), (3, 256), (1, 253), (3, 1024), (5, 1021), (7, 1023), (5, 1027), (2, 119), (5, 121), (3, 121), (4, 142),
             (1, 0), (1, 4)]
    for i, (r, c) in enumerate(spots):
        if r < H and c < W and valid[r, c]:
            for k, v in enumerate(kinds[i % len(kinds)]):
                if v is not None:
                    xyz[r, c, k] = v


def cases_of(shape):
    H, W = shape
    rng = np.random.default_rng([7, H, W])
    fm = features(H, W)
    rm = (rng.random((H, W)) < 0.85).astype(np.uint8)
    runs = [(MAX_HOLE, INF), (MAX_HOLE, 0.25), (MAX_HOLE_LARGE, 0.25), (0, INF)]
    base = (MC.plane(H, W) + rng.normal(0.0, 0.03, size=(H, W, 3))).astype(np.float32)
    rim = base.copy()
    _nonfinite_rim(rim, fm)
    garbage = rim.copy()
    garbage[fm == 0] = MC.GARBAGE
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    denormal = (1e-40 * np.stack([cc % 100, rr, 0.0 * cc], axis=-1) + rng.uniform(0.0, 3e-41, size=(H, W, 3))).astype(np.float32)
    far = (1e5 + MC.plane(H, W) + rng.normal(0.0, 1e-3, size=(H, W, 3))).astype(np.float32)
    return [(f"holes-{H}x{W}-features", base, fm, runs),
            (f"holes-{H}x{W}-rim-clean", rim, fm, runs[:3]),
            (f"holes-{H}x{W}-rim-garbage", garbage, fm.copy(), runs[:3]),
            (f"holes-{H}x{W}-random", base, rm, [(3, INF), (MAX_HOLE_LARGE, 0.25)]),
            (f"holes-{H}x{W}-denormal", denormal, rm, [(MAX_HOLE, 1.5e-40), (MAX_HOLE, INF)]),
            (f"holes-{H}x{W}-1e5", far, fm, [(MAX_HOLE, 0.3), (MAX_HOLE_LARGE, INF)])]


def serpentine_case():
    """one hole that winds through the frame: corridors 1 pixel high, 2 rows apart, joined at alternating ends, inside a frame of
    candidates; filled at max_hole = its size, left alone at one less"""
    H, W = SERPENTINE_SHAPE
    snake = serpentine(H - 2, W - 2, 1, 2)
    valid = np.ones((H, W), np.uint8)
    valid[1:-1, 1:-1] = 1 - snake
    size = int(snake.sum())
    xyz = MC.plane(H, W).astype(np.float32)
    return ("holes-serpentine", xyz, valid, [(size, INF), (size - 1, INF), (size, 0.25)]), size
