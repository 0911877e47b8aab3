"""Crafted dense planes for the mesh kernels, shared by the CPU test (tests/test_mesh_cases.py: the conditions below are asserted there,
with the restatements alone, and every case goes through the host headers) and the GPU test (tests/test_gpu_mesh_crafted.py: every case
is written into a context's dense planes, tests/dense_planes.py).  Every generator returns a list of cases

    (name, xyz float32 (H, W, 3), valid uint8 (H, W) of 0/1, max_edges)

built from fixed seeds.  BASE_SHAPES are the smallest (H, W) at which the kernels' indexing can go wrong: the quad (a lane owns 4 pixels),
the pitch of 16, the wave seam at pixel 256, the chunk seam at 1024 (MESH_CHUNK), widths 4k + 1 (the pixel right of the last quad is alone
in the window), one row, one column.

  integers     coordinates in -2..2 times a power of two: exact ties len2(a,e) == len2(b,d), len2 == max_edge^2, coincident points,
               zero-area faces (a vertex in a face with the zero normal)
  swapped      4-valid cells with a - e = (p, q, 0), b - d = (q, p, 0), p and q inexact squares: p*p + q*q == q*q + p*p only as long as
               neither product is fused into the add -- the case a contracted build of the device code fails
  nonfinite    NaN, +inf, -inf and a mixed triple under valid pixels next to every seam; a twin with 1e30 under the invalid pixels and
               in the padding columns, which are marked valid there (PADDING): the results are those of the clean twin
  range        float32 denormals; coordinates near the top of the float range, where the second (mu) step of an iteration overflows;
               1e5 with millimetre detail
  topologies   on the plane (0.2 col, 0.2 row, 500) without an edge-length test: checkerboard, comb, rectangular spiral, two blocks joined
               by one face across the chunk seam, a face whose chunk holds none of its vertices, a percolating sheet
"""
from fractions import Fraction

import numpy as np

INF = float("inf")
BASE_SHAPES = [(3, 5), (2, 17), (4, 257), (3, 1023), (3, 1025), (3, 2049), (33, 1), (1, 33)]
TOPOLOGY_SHAPES = {"comb": (12, 2049), "spiral": (38, 2049), "blocks": (6, 2049), "lone_face": (5, 2049), "percolation": (40, 1025)}
GARBAGE = np.float32(1e30)
PADDING = dict(pad_xyz=GARBAGE, pad_valid=1)       # of the cases whose name ends in "garbage"
# the smoothing runs of the crafted suite: (iterations, mu, flags); lambda is 0.5.  Odd and even step counts: 1, 4 and 6 steps
SMOOTH_RUNS = [(1, 0.0, 0), (2, -0.53, 1), (3, -0.53, 3)]
LAMBDA = 0.5


def plane(H, W):
    """(0.2 col, 0.2 row, 500) in double"""
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([0.2 * cc, 0.2 * rr, np.full((H, W), 500.0)], axis=-1)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _mask(rng, H, W, p):
    return np.ones((H, W), np.uint8) if p >= 1.0 else (rng.random((H, W)) < p).astype(np.uint8)


# ---- integers ---------------------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 2.0 ** -10, 2.0 ** 20)
SELECTIONS = (0.5, 0.95, 1.0)


def integer_cases(shape):
    H, W = shape
    out = []
    for si, scale in enumerate(SCALES):
        for pi, p in enumerate(SELECTIONS):
            rng = _rng(1, H, W, si, pi)
            xyz = (rng.integers(-2, 3, size=(H, W, 3)).astype(np.float64) * scale).astype(np.float32)
            out.append((f"integers-{H}x{W}-scale{si}-p{p}", xyz, _mask(rng, H, W, p), (2.0 * scale, 3.0 * scale, INF)))
    return out


# ---- swapped cells ----------------------------------------------------------------------------------------------------------------------
def swapped_cells(shape):
    """the cells (r, c) of corner a the swapped case of a shape builds: every third column of every third row, so that no two share a
    pixel and no other cell has three valid corners"""
    H, W = shape
    return [(r, c) for r in range(0, H - 1, 3) for c in range(0, W - 1, 3)]


def swapped_cases(shape):
    """a = (X, Y), e = (x, y), b = (Y, X), d = (y, x) with X, Y about 1e3 and x, y about 1e-2, all float32: a - e = (p, q) and
    b - d = (q, p) with p = X - x, q = Y - y exact in double and about 40 bits wide."""
    H, W = shape
    cells = swapped_cells(shape)
    if not cells:
        return []
    rng = _rng(2, H, W)
    xyz = np.zeros((H, W, 3), np.float32)
    valid = np.zeros((H, W), np.uint8)
    for r, c in cells:
        X, Y = np.float32(rng.uniform(500.0, 2000.0, 2))
        x, y = np.float32(rng.uniform(0.005, 0.02, 2))
        xyz[r, c], xyz[r, c + 1], xyz[r + 1, c], xyz[r + 1, c + 1] = (X, Y, 500.0), (Y, X, 500.0), (y, x, 500.0), (x, y, 500.0)
        valid[r:r + 2, c:c + 2] = 1
    return [(f"swapped-{H}x{W}", xyz, valid, (INF,))]


def swapped_diagonals(xyz, cells):
    """Per swapped cell, exactly (fractions.Fraction; float() of one rounds correctly): (ties uncontracted, takes b-d if dx*dx is fused
    into the add -- fma(dx, dx, dy*dy) --, takes b-d if dy*dy is -- fma(dy, dy, dx*dx)).  dz is 0: the last term changes nothing in
    any form."""
    def fl(v):
        return Fraction(float(v))
    tie, fused_x, fused_y = [], [], []
    for r, c in cells:
        a, b, d, e = (xyz[r, c], xyz[r, c + 1], xyz[r + 1, c], xyz[r + 1, c + 1])
        p, q = Fraction(float(a[0])) - Fraction(float(e[0])), Fraction(float(a[1])) - Fraction(float(e[1]))
        assert fl(p) == p and fl(q) == q                                          # the differences are exact in double
        assert Fraction(float(b[0])) - Fraction(float(d[0])) == q and Fraction(float(b[1])) - Fraction(float(d[1])) == p
        assert a[2] == e[2] and b[2] == d[2]
        pp, qq = fl(p * p), fl(q * q)
        assert pp != p * p and qq != q * q                                        # both squares are inexact
        tie.append(fl(pp + qq) == fl(qq + pp))
        ae_x, bd_x = fl(p * p + qq), fl(q * q + pp)                               # fma(dx, dx, dy*dy): a-e has dx = p, b-d has dx = q
        fused_x.append(ae_x > bd_x)
        fused_y.append(bd_x > ae_x)                                               # fma(dy, dy, dx*dx): the two swap
    return np.array(tie), np.array(fused_x), np.array(fused_y)


def swapped_took_bd(faces, valid, cells):
    """how many of the swapped cells have the faces of the diagonal b-d in a face list of the case (ids: scan order of valid)"""
    vid = (np.cumsum(valid.ravel()) - 1).reshape(valid.shape)
    have = {tuple(f) for f in np.asarray(faces).tolist()}
    return sum((int(vid[r, c]), int(vid[r + 1, c]), int(vid[r, c + 1])) in have for r, c in cells)      # (a, d, b)


# ---- non-finite coordinates -------------------------------------------------------------------------------------------------------------
KINDS = ("nan", "+inf", "-inf", "mixed")


def special_positions(H, W):
    """[(row, col, kind)]: columns 0, 3 / 4, 255 / 256, 1023 / 1024 and the last, alternating between the first and the last row, then
    the remaining corners and the middle row; no two within one pixel of each other, diagonals included."""
    cols = sorted({c for c in (0, 3, 4, 255, 256, 1023, 1024, W - 1) if 0 <= c < W})
    rows = [0, H - 1] if H > 1 else [0]
    cand = []
    for i, c in enumerate(cols):
        cand.append([(rows[i % len(rows)], c), (rows[(i + 1) % len(rows)], c)])
    cand += [[(H - 1, 0)], [(0, W - 1)], [(H - 1, W - 1)]] + [[(H // 2, c)] for c in cols]
    used = []
    for options in cand:
        for r, c in options:
            if all(max(abs(r - r2), abs(c - c2)) >= 2 for r2, c2 in used):
                used.append((r, c))
                break
    return [(r, c, KINDS[i % 4]) for i, (r, c) in enumerate(used)]


def nonfinite_cases(shape):
    H, W = shape
    rng = _rng(3, H, W)
    xyz = (plane(H, W) + rng.normal(0.0, 0.05, size=(H, W, 3))).astype(np.float32)
    valid = _mask(rng, H, W, 0.9)
    for i, (r, c, kind) in enumerate(special_positions(H, W)):
        valid[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = 1                       # the point and the pixels around it
        if kind == "mixed":
            xyz[r, c] = (np.nan, np.inf, -np.inf)
        else:
            xyz[r, c, i % 3] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    garbage = xyz.copy()
    garbage[valid == 0] = GARBAGE
    edges = (0.35, INF)
    return [(f"nonfinite-{H}x{W}-clean", xyz, valid, edges), (f"nonfinite-{H}x{W}-garbage", garbage, valid.copy(), edges)]


# ---- the float range --------------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
HUGE_PEAK, HUGE_AMPLITUDE, HUGE_PERIOD = 3.4028e38, 1.0e38, 16
HUGE_SHAPE = (40, 1025)


def huge_case(shape):
    """x: a cosine of period 16 columns whose crests stand 2.3e33 below FLT_MAX.  Over the neighbours of an inner vertex -- 4 of 6 one
    column away -- the crest is an eigenvector of the step with k = (2/3)(1 - cos(pi/8)) = 0.0507: one step with 0.5, one with -0.53
    multiply its height above the mean by (1 - 0.5k)(1 + 0.53k) = 1.00084, 8e34 more than it was: beyond the float range.  That needs
    moving neighbours all around: with fixed boundary rows, a shape of more than 4 rows (HUGE_SHAPE); on the base shapes the case stays
    finite."""
    H, W = shape
    rng = _rng(6, H, W)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x = HUGE_PEAK - HUGE_AMPLITUDE * (1.0 - np.cos(2.0 * np.pi * cc / HUGE_PERIOD)) + rng.normal(0.0, 1e32, size=(H, W))
    huge = np.stack([x, 0.2 * rr, 500.0 + 0.0 * cc], axis=-1).astype(np.float32)
    return (f"range-{H}x{W}-huge", huge, np.ones((H, W), np.uint8), (INF,))


def range_cases(shape):
    H, W = shape
    rng = _rng(4, H, W)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    # a grid of 1e-40 that starts again every 100 columns (2048e-40 would be a normal number), so a few edges are long
    denormal = (1e-40 * np.stack([cc % 100, rr, 0.0 * cc], axis=-1) + rng.uniform(0.0, 3e-41, size=(H, W, 3))).astype(np.float32)
    far = (1e5 + plane(H, W) + rng.normal(0.0, 1e-3, size=(H, W, 3))).astype(np.float32)
    return [(f"range-{H}x{W}-denormal", denormal, _mask(rng, H, W, 0.9), (1.5e-40, INF)), huge_case(shape),
            (f"range-{H}x{W}-1e5", far, _mask(rng, H, W, 0.9), (0.3, INF))]


# ---- topologies -------------------------------------------------------------------------------------------------------------------------
def checkerboard(H, W):
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((rr + cc) % 2 == 0).astype(np.uint8)


COMB_TEETH = (0, 60, 254, 500, 1022, 1500, 2045)        # first column of a tooth 4 columns wide: 254..257 and 1022..1025 straddle the seams


def comb(H, W):
    m = np.zeros((H, W), np.uint8)
    for t in COMB_TEETH:
        m[:, t:t + 4] = 1
    m[H - 2:] = 1                                       # the spine
    return m


def spiral(H, W):
    """Corridors 2 pixels wide between walls 1 pixel wide, wound inwards: ring k (the pixels 3k or 3k + 1 away from the border) is cut
    in its top corridor at column 100 - 10k, and a door 2 pixels wide right of the cut leads down into ring k + 1 -- so ring k is walked
    from the door all the way round to the cut, where the next door is.  Vertex 0 sits at the far end of ring 0."""
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.minimum(np.minimum(rr, cc), np.minimum(H - 1 - rr, W - 1 - cc))
    m = (d % 3 != 2).astype(np.uint8)
    rings = spiral_rings(H, W)
    for k in range(rings - 1):
        m[3 * k:3 * k + 2, _spiral_cut(k, W)] = 0       # the cut through ring k's top corridor (the innermost ring just ends)
    for r, c in spiral_doors(H, W):
        m[r, c] = 1
    return m


def spiral_rings(H, W):
    return ((min(H, W) - 1) // 2 + 3) // 3


def _spiral_cut(k, W):
    cut = 100 - 10 * k
    assert cut > 3 * k + 8 and cut + 5 < W - 3 * k - 8
    return cut


def spiral_doors(H, W):
    """the door pixels: in the wall above ring k's top corridor, 2 pixels wide, for k = 1 .. rings - 1"""
    return [(3 * k - 1, _spiral_cut(k, W) + j) for k in range(1, spiral_rings(H, W)) for j in (3, 4)]


def blocks(H, W):
    """columns 0..1023 and 1025.. full; column 1024 only in the last row: the blocks meet in the face (a, d, e) of the cell at column
    1023 of the last cell row and nowhere else"""
    m = np.ones((H, W), np.uint8)
    m[:H - 1, 1024] = 0
    return m


def lone_face(H, W):
    """row 0 holds no pixel left of column 1024 and every pixel from there on, row 1 every pixel: the face (b, d, e) of the cell at column
    1023 belongs to the chunk (row 0, columns 0..1023), which has no vertex.  Rows 3 and 4: small islands, the components a filter drops."""
    m = np.zeros((H, W), np.uint8)
    m[0, 1024:] = 1
    m[1] = 1
    m[3:5, 10:12] = 1
    m[3:5, 1023:1025] = 1
    m[3, 40:43] = 1
    m[4, 40] = 1
    m[4, 100] = m[3, 2000] = 1
    return m


def percolation_z(rng, H, W, amplitude=1.0):
    """random z whose spread grows with the column, from 0 to `amplitude`: at the median edge length the left part is one sheet of more
    than a quarter of the vertices, the right part single vertices, and in between the sheet breaks up into thousands of fragments.
    (Noise of one spread everywhere does not percolate at its median: no component above 1 % of the vertices.)"""
    return rng.normal(0.0, 1.0, size=(H, W)) * (amplitude * np.arange(W) / (W - 1))[None, :]


def topology_cases(shape):
    H, W = shape
    base = plane(H, W).astype(np.float32)
    out = []
    if shape in BASE_SHAPES:
        out.append((f"checkerboard-{H}x{W}", base, checkerboard(H, W), (INF,)))
    for name, build in (("comb", comb), ("spiral", spiral), ("blocks", blocks), ("lone_face", lone_face)):
        if TOPOLOGY_SHAPES[name] == shape:
            out.append((f"{name}-{H}x{W}", base, build(H, W), (INF,)))
    if TOPOLOGY_SHAPES["percolation"] == shape:
        from mesh_reference import np_mesh
        rng = _rng(5, H, W)
        xyz = plane(H, W)
        xyz[..., 2] += percolation_z(rng, H, W)
        xyz = xyz.astype(np.float32)
        valid = np.ones((H, W), np.uint8)
        st = {}
        np_mesh(xyz, valid, INF, st)
        out.append((f"percolation-{H}x{W}", xyz, valid, (float(np.float32(np.sqrt(np.median(st["len2"])))),)))
    return out


# ---- everything -------------------------------------------------------------------------------------------------------------------------
ALL_SHAPES = BASE_SHAPES + [s for s in dict.fromkeys(TOPOLOGY_SHAPES.values()) if s not in BASE_SHAPES]


def cases_of(shape):
    """every case of one shape"""
    out = topology_cases(shape)
    if shape in BASE_SHAPES:
        out = integer_cases(shape) + swapped_cases(shape) + nonfinite_cases(shape) + range_cases(shape) + out
    if shape == HUGE_SHAPE:
        out.append(huge_case(shape))
    return out


def padding_of(name):
    """put_dense's pad_xyz / pad_valid of a case"""
    return PADDING if name.endswith("garbage") else {}


def second_largest(labels):
    """s of the filter thresholds {1, 2, s, s + 1}: the second-largest component size (the largest if there is one component, 1 if none)"""
    sizes = np.sort(np.bincount(labels)[np.unique(labels)])[::-1] if len(labels) else np.zeros(0, int)
    return int(sizes[1]) if len(sizes) > 1 else int(sizes[0]) if len(sizes) else 1


def bits_differ(got, want, produced=False):
    """Number of float32 entries that differ: bit for bit (+0 is not -0, a NaN's sign and payload count); with `produced` -- values the
    arithmetic made, not copies -- a NaN of the restatement only asks for a NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if produced:
        diff &= ~(np.isnan(want) & np.isnan(got))
    return int(diff.sum())
