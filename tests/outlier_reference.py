"""NumPy restatement of the radius outlier filter (the rule: include/sl3d_filter.h; the device: sl3d_filter_outliers, k_outlier_support /
k_outlier_apply; the C arithmetic: 3dscan_amd/csrc/sl3d_outlier.h) and the inputs its tests share.

float64 arithmetic in the rule's order -- len2 = (dx*dx + dy*dy) + dz*dz of the float32 coordinates widened to double, every operation a
NumPy ufunc of its own (nothing is contracted) -- in one shifted-slice pass per (dr, dc).  The neighbourhood is clipped to the window: the
arrays ARE the window, there is no padding here."""
import numpy as np

NO_SAMPLE = 0xFF
NAN_BITS = 0x7FC00000          # __builtin_nanf(""): what every dense kernel writes under an invalid pixel


def max_support(radius):
    return (2 * radius + 1) ** 2 - 1


def support_plane(xyz, valid, radius, max_dist):
    """uint8 [H][W]: support(p) at every sample (valid == 1), 0xFF elsewhere.  xyz: float32 [H][W][3], max_dist: a float32 value."""
    assert xyz.dtype == np.float32 and xyz.shape == valid.shape + (3,) and valid.dtype == np.uint8
    H, W = valid.shape
    sample = valid == 1
    p = xyz.astype(np.float64)
    thr2 = np.float64(np.float32(max_dist)) * np.float64(np.float32(max_dist))
    n = np.zeros((H, W), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dr in range(-radius, radius + 1):
            for dc in range(-radius, radius + 1):
                r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
                if (dr, dc) == (0, 0) or r0 >= r1 or c0 >= c1:
                    continue
                d = p[r0:r1, c0:c1] - p[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
                len2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                n[r0:r1, c0:c1] += (len2 <= thr2) & sample[r0 + dr:r1 + dr, c0 + dc:c1 + dc]      # (NaN <= thr2 is False)
    assert n.max(initial=0) <= max_support(radius)
    return np.where(sample, n, NO_SAMPLE).astype(np.uint8)


def filter_outliers(xyz, valid, radius, max_dist, min_neighbours):
    """The post-state of one view: dict(support, valid, bits -- the points as uint32 --, rejected -- the mask --, counts = (samples on entry,
    rejected samples))."""
    assert 0 <= min_neighbours <= max_support(radius)
    support = support_plane(xyz, valid, radius, max_dist)
    sample = valid == 1
    rejected = sample & (support < min_neighbours) if min_neighbours > 0 else np.zeros_like(sample)
    bits = np.ascontiguousarray(xyz).view(np.uint32).copy()
    bits[rejected] = NAN_BITS
    return dict(support=support, valid=np.where(rejected, 0, valid).astype(np.uint8), bits=bits, rejected=rejected,
                counts=(int(sample.sum()), int(rejected.sum())))


def step_scene(H=37, W=130, seed=7):
    """Two fronto-parallel planes 30 mm apart with a step between them, 0.5 mm pixel spacing: 3 % holes, 2 % of the valid pixels lifted by
    20 mm (speckle), and four columns of flying pixels across the step with depths anywhere between the two planes.  Returns (xyz float32
    [H][W][3], valid uint8 [H][W], planted bool [H][W]: the valid pixels that are speckle or flying).  At 37 x 130 the step is at column 70
    and the flying pixels are columns 68 .. 71; at other widths the step is in the middle."""
    rng = np.random.default_rng(seed)
    step = 70 if W == 130 else (W + 1) // 2
    r, c = np.mgrid[0:H, 0:W]
    x, y = (0.5 * c).astype(np.float32), (0.5 * r).astype(np.float32)
    z = np.where(c < step, 500, 530).astype(np.float32)
    valid = rng.random((H, W)) < 0.97
    speck = (rng.random((H, W)) < 0.02) & valid
    z[speck] += np.float32(20)
    flying = (c >= step - 2) & (c < step + 2)
    z = np.where(flying, (500 + 30 * rng.random((H, W))).astype(np.float32), z)
    return np.stack([x, y, z], axis=-1).astype(np.float32), valid.astype(np.uint8), (speck | flying) & valid


# ---- the crafted inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------------
# (radius, max_dist, min_neighbours) of the crafted cases: at 0.5 mm pixel spacing each rejects some samples and keeps others
PARAMS = {1: (1, 1.0, 3), 2: (2, 1.5, 8), 3: (3, 2.0, 14), 4: (4, 2.5, 20)}
# What the tests poison the padding columns [W, pitch) with, beside a valid byte of 1: the point (PAD, PAD, PAD).  grid() puts it where the
# pixel (H // 2, W) -- the first padding column -- would lie, 0.5 mm from the window's last column: a kernel that clips to the pitch
# instead of the window counts it for every pixel within `radius` columns of the right edge in the rows around H // 2
PAD = np.float32(500)


def grid(H, W):
    r, c = np.mgrid[0:H, 0:W]
    return np.stack([500 + 0.5 * (c - W), 500 + 0.5 * (r - H // 2), np.full((H, W), 500.0)], axis=-1).astype(np.float32)


def crafted_cases(H, W):
    """[(name, xyz, valid)]: a noisy plane with 30 % holes; the step scene's construction at the shape (mirrored, so that its 500 mm plane
    meets the padding); all valid; none valid (finite points lie under the invalid pixels); a single valid pixel in each corner,
    everything else invalid with points close by."""
    rng = np.random.default_rng(1000 * H + W)
    noisy = grid(H, W)
    noisy[..., 2] += (0.6 * rng.standard_normal((H, W))).astype(np.float32)
    holes = (rng.random((H, W)) >= 0.3).astype(np.uint8)
    sx, sv, _ = step_scene(H, W, seed=7 + H + W)
    sx, sv = sx[:, ::-1].copy(), sv[:, ::-1].copy()                      # the 500 mm plane on the right, laid over the grid: PAD is next to it
    sx[..., :2] = grid(H, W)[..., :2]
    corners = np.zeros((H, W), np.uint8)
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = 1
    return [("holes", noisy, holes), ("step", sx, sv), ("all_valid", noisy, np.ones((H, W), np.uint8)),
            ("none_valid", grid(H, W), np.zeros((H, W), np.uint8)), ("corners", grid(H, W), corners)]


def tie_lattice(H=7, W=9):
    """the integer lattice (3 c, 4 r, 0): the diagonal neighbours are at offset (+-3, +-4, 0), len2 = 25 exactly"""
    r, c = np.mgrid[0:H, 0:W]
    return np.stack([3.0 * c, 4.0 * r, 0.0 * c], axis=-1).astype(np.float32), np.ones((H, W), np.uint8)


def nonfinite_case(H=9, W=13):
    """a 0.5 mm grid, all valid but a sprinkling of invalid pixels whose finite points lie ON the grid (they must not count); samples
    with NaN, +-Inf and +-3e38 coordinates.  Returns (xyz, valid, special: {name: [(r, c)]})."""
    xyz, valid = grid(H, W), np.ones((H, W), np.uint8)
    valid[1::3, 2::4] = 0
    special = {"nan": [(0, 0), (4, 6)], "inf": [(2, 3), (8, 12)], "ninf": [(5, 1)], "huge": [(3, 9), (6, 5)], "nhuge": [(7, 8), (0, 12)]}
    value = {"nan": np.nan, "inf": np.inf, "ninf": -np.inf, "huge": 3e38, "nhuge": -3e38}
    for k, (name, where) in enumerate(special.items()):
        for j, (r, c) in enumerate(where):
            valid[r, c] = 1
            xyz[r, c, (k + j) % 3] = np.float32(value[name])
    xyz[4, 7] = xyz[4, 8] = np.float32(3e38)                             # two equal huge samples side by side: len2 == 0, they count each other
    valid[4, 7] = valid[4, 8] = 1
    return xyz, valid, special


def jacobi_line(H, W, cells):
    """valid pixels at `cells` [(r, c)] -- a line of pixels one spacing apart --, the k-th at distance k from the first along x: with
    max_dist 1 and a radius of at least the spacing each has exactly its two line neighbours in range, the two ends one.  Everything else
    is invalid, with the first cell's point under it."""
    xyz, valid = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.uint8)
    for k, (r, c) in enumerate(cells):
        xyz[r, c, 0], valid[r, c] = k, 1
    return xyz, valid
