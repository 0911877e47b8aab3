"""Crafted segmented clouds for the consumers of sl3d_run_clouds' output (k_seg_scan, the three k_seg_close forms and the host routes around
them), and a NumPy restatement of what the consumers must return.  tests/cloud_segments.py writes a case into a context,
tests/test_gpu_cloud_segments_crafted.py runs the consumers over it, tests/test_segment_cases.py asserts on the CPU what the cases contain.

A view is n_segs = 4 * tiles segments of 256 point slots and one uint32 count per segment.  Its REAL segments are the s with
256 * s < pitch * H; the last real one may own fewer than 256 slots, the segments behind it own none (room()).

The restatement:
  offsets   the exclusive uint64 cumulative sum of the counts
  total     their sum
  cloud     the concatenation of every segment's first `count` slots (bits, not values)
  clamped   the cloud's first `capacity` points
  registered  the oracle's register_point_clouds over the restated clouds"""
import numpy as np

SEG = 256                      # SL3D_SEG_POINTS
SCAN_PARTS, SCAN_CHUNK = 8, 4096   # k_seg_scan: SL3D_SCAN_PARTS blocks per view, 1024 threads x SL3D_SCAN_RUN counts per chunk
SENTINEL = np.float32(1e30)    # in every slot behind a count: it must never appear in any output
SENTINEL_BITS = int(np.array([SENTINEL]).view(np.uint32)[0])

# (W, H) -- the smallest shapes at which each code path of the consumers exists
SMALL_SHAPES = ((64, 3), (1021, 64), (1024, 260), (1024, 1100))
# the k_seg_scan paths no decode in the suite reaches: part 7 non-empty; two chunks per part, the last one 336 counts; part 7 with two chunks
# (the only part whose carry behind its LAST chunk is used: it is the view's total); three chunks per part
LONG_SHAPES = ((4096, 1800), (4096, 2325), (4096, 3900), (4096, 4100))
ORDER_SHAPE = (1021, 64)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def geometry(W, H):
    """(pitch, slots of a view = its view stride in points, n_segs, number of real segments)"""
    pitch = (W + 15) // 16 * 16
    px = pitch * H
    n_tiles = (px // 4 + 255) // 256
    return pitch, px, 4 * n_tiles, (px + SEG - 1) // SEG


def room(W, H):
    """int64[n_segs]: the slots segment s owns -- min(256, pitch*H - 256*s), 0 behind the last real segment"""
    _, px, n_segs, _ = geometry(W, H)
    return np.clip(px - SEG * np.arange(n_segs, dtype=np.int64), 0, SEG)


def check_bounds(W, H, counts):
    """what keeps every consumer inside the allocation: counts[s] <= 256, <= pitch*H - 256*s, == 0 beyond the last real segment"""
    _, px, n_segs, n_real = geometry(W, H)
    counts = np.asarray(counts)
    assert counts.dtype == np.uint32 and counts.shape == (n_segs,), (counts.dtype, counts.shape, n_segs)
    c, s = counts.astype(np.int64), np.arange(n_segs, dtype=np.int64)
    assert (c <= SEG).all(), "a count above 256"
    assert (c[:n_real] <= px - SEG * s[:n_real]).all(), "a count beyond the view's last slot"
    assert not c[n_real:].any(), "a count behind the last real segment"


def part_len(n_segs):
    """k_seg_scan: counts per part -- whole chunks"""
    per = (n_segs + SCAN_PARTS - 1) // SCAN_PARTS
    return (per + SCAN_CHUNK - 1) // SCAN_CHUNK * SCAN_CHUNK


def scan_layout(n_segs):
    """(parts that own counts, chunks of the longest part, counts in the last chunk of the last non-empty part)"""
    pl = part_len(n_segs)
    parts = (n_segs + pl - 1) // pl
    last = n_segs - (parts - 1) * pl
    return parts, (min(pl, n_segs) + SCAN_CHUNK - 1) // SCAN_CHUNK, last - (last - 1) // SCAN_CHUNK * SCAN_CHUNK


SEAM_KINDS = ("lane_run_256", "front_stride_1024", "chunk_4096", "part")


def seam_indices(W, H):
    """kind -> the indices m*k - 1 and m*k + 1 (k >= 1) among the real segments: m = 256 (the counts one wave of k_seg_scan loads), 1024 (the
    stride of the n_front loop of k_seg_close<SCAN>), 4096 (a chunk of k_seg_scan), part_len (a part of k_seg_scan)"""
    _, _, n_segs, n_real = geometry(W, H)
    out = {}
    for kind, m in zip(SEAM_KINDS, (256, 1024, 4096, part_len(n_segs))):
        k = np.arange(m, n_real + 2, m, dtype=np.int64)
        idx = np.concatenate([k - 1, k + 1])
        out[kind] = np.unique(idx[idx < n_real])
    return out


def block4_indices(W, H):
    """the indices 4k - 1 and 4k (k >= 1) among the real segments: the last wave of a block of k_seg_close and the first of the next"""
    _, _, _, n_real = geometry(W, H)
    k = np.arange(4, n_real + 1, 4, dtype=np.int64)
    idx = np.concatenate([k - 1, k])
    return np.unique(idx[idx < n_real])


# ---- count patterns ---------------------------------------------------------------------------------------------------------------------
def _only_at(W, H, idx, rng):
    rm = room(W, H)
    c = np.zeros(len(rm), np.int64)
    c[idx] = rng.integers(1, SEG + 1, len(idx))
    return np.minimum(c, rm).astype(np.uint32)


def count_patterns(W, H, seed=0):
    """name -> uint32[n_segs]"""
    _, _, n_segs, n_real = geometry(W, H)
    rm = room(W, H)
    rng = np.random.default_rng([W, H, seed])
    s = np.arange(n_segs)
    first, last = np.zeros(n_segs, np.uint32), np.zeros(n_segs, np.uint32)
    first[0], last[n_real - 1] = 1, 1
    sparse = np.where(rng.random(n_segs) < 0.03, rng.integers(1, 4, n_segs), 0)
    sparse[rng.integers(0, n_real)] = 2                                       # (never empty)
    seams = np.concatenate(list(seam_indices(W, H).values())).astype(np.int64)
    p = {
        "zeros": np.zeros(n_segs, np.uint32),
        "full": rm.astype(np.uint32),                                          # (the last real segment at its own maximum)
        "first_only": first,
        "last_only": last,
        "alternating": np.minimum(np.where(s % 2 == 1, SEG, 0), rm).astype(np.uint32),
        "random": np.minimum(rng.integers(0, SEG + 1, n_segs), rm).astype(np.uint32),
        "random2": np.minimum(rng.integers(0, SEG + 1, n_segs), rm).astype(np.uint32),
        "sparse": np.minimum(sparse, rm).astype(np.uint32),
        "block4": _only_at(W, H, block4_indices(W, H), rng),
        "seams": _only_at(W, H, np.unique(seams), rng),
    }
    for c in p.values():
        check_bounds(W, H, c)
    return p


# ---- payloads ---------------------------------------------------------------------------------------------------------------------------
PAYLOADS = ("finite", "nan", "special", "reg_nan_y", "reg_flt_max")


def payload(kind, n, seed=0):
    """float32 [n, 3] for the slots of a view"""
    rng = np.random.default_rng([PAYLOADS.index(kind), n, seed])
    xyz = rng.uniform(-1000.0, 1000.0, (n, 3)).astype(np.float32)
    if kind == "finite":
        return xyz
    if kind == "nan":
        # every slot a NaN of its own: distinct payloads (quiet and signalling), both signs
        i = np.arange(3 * n, dtype=np.uint64)
        mant = (1 + i * 2654435761) % 0x7FFFFF
        mant[mant == 0] = 1
        bits = (0x7F800000 | mant | ((i & 1) << 31)).astype(np.uint32)
        return bits.view(np.float32).reshape(n, 3).copy()
    if kind == "special":
        pool = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000],
                        np.uint32)   # +inf -inf -0 +0, denormals of both signs, +-FLT_MAX, the smallest normal
        pick = rng.integers(0, len(pool) + 4, (n, 3))
        bits = np.where(pick < len(pool), pool[np.minimum(pick, len(pool) - 1)], xyz.view(np.uint32))
        return bits.astype(np.uint32).view(np.float32).copy()
    if kind == "reg_nan_y":
        # an infinite or NaN y beside finite x, z: the definition multiplies y by an exact 0.0, so X and Z of the registered point are NaN
        y = np.array([np.inf, -np.inf, np.nan], np.float32)[rng.integers(0, 3, n)]
        xyz[:, 1] = np.where(rng.random(n) < 0.5, y, xyz[:, 1])
        return xyz
    if kind == "reg_flt_max":
        # coordinates near FLT_MAX: the double sum r00*x + r02*z leaves the float range on the way back to float
        big = (rng.uniform(0.85, 1.0, (n, 3)) * 3.4e38 * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
        xyz = np.where(rng.random((n, 1)) < 0.5, big, xyz).astype(np.float32)
        return xyz
    raise ValueError(kind)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# (count pattern, payload): every pattern over finite randoms, the non-finite payloads and the two registration cases over random counts.
# Consecutive triples share a context (views 0..2); the registration cases lie in views 1 and 2, where the rotation angle is not 0
CASE_LIST = (("zeros", "finite"), ("full", "finite"), ("first_only", "finite"),
             ("last_only", "finite"), ("alternating", "finite"), ("random", "finite"),
             ("sparse", "finite"), ("block4", "finite"), ("seams", "finite"),
             ("random2", "nan"), ("random", "reg_nan_y"), ("random2", "reg_flt_max"),
             ("sparse", "nan"), ("random", "special"), ("alternating", "special"))


def cases_of(shape):
    """[(name, counts uint32[n_segs], xyz float32[n_segs*256, 3])] -- xyz before the sentinel goes behind the counts"""
    W, H = shape
    _, _, n_segs, _ = geometry(W, H)
    pats = count_patterns(W, H)
    return [(f"{p}-{q}", pats[p], payload(q, n_segs * SEG, seed=i)) for i, (p, q) in enumerate(CASE_LIST)]


def triples_of(shape):
    c = cases_of(shape)
    assert len(c) % 3 == 0
    return [c[i:i + 3] for i in range(0, len(c), 3)]


def with_fill(W, H, counts, xyz, fill):
    """xyz with `fill` in every slot behind a count (the slots the view does not own are left as they are: nobody writes them)"""
    _, _, n_segs, _ = geometry(W, H)
    out = np.array(xyz, np.float32).reshape(n_segs, SEG, 3)
    out[np.arange(SEG)[None, :] >= np.asarray(counts)[:, None].astype(np.int64)] = np.float32(fill)
    return out.reshape(n_segs * SEG, 3)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def restate(counts, xyz):
    """(offsets uint64[n_segs], total, cloud float32[total, 3]); xyz: [>= 256 * (last segment with a count + 1), 3], rows beyond it are not read"""
    counts = np.asarray(counts, np.uint32)
    n = len(counts)
    c64 = counts.astype(np.uint64)
    incl = np.cumsum(c64, dtype=np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64), incl[:-1]])
    total = int(incl[-1])
    used = int(np.flatnonzero(counts)[-1]) + 1 if total else 0
    take = np.arange(SEG)[None, :] < counts[:used, None].astype(np.int64)
    slots = np.asarray(xyz)[:used * SEG]
    if len(slots) < used * SEG:                                   # (a last real segment that owns fewer than 256 slots)
        slots = np.concatenate([slots, np.zeros((used * SEG - len(slots), 3), np.float32)])
    cloud = np.ascontiguousarray(slots.reshape(used, SEG, 3)[take]) if used else np.zeros((0, 3), np.float32)
    assert cloud.shape == (total, 3) and len(offsets) == n
    return offsets, total, cloud


def restate_loop(counts, xyz):
    """the same, literally: one segment after the other"""
    offsets, cloud, run = [], [], 0
    for s, c in enumerate(counts):
        offsets.append(run)
        for i in range(int(c)):
            cloud.append(xyz[SEG * s + i])
        run += int(c)
    cloud = np.array(cloud, np.float32).reshape(-1, 3) if cloud else np.zeros((0, 3), np.float32)
    return np.array(offsets, np.uint64), run, cloud


def clamped(cloud, capacity):
    return cloud[:max(int(capacity), 0)]


def registered(clouds, t, rot_step):
    """the oracle's register_point_clouds (9/register_point_clouds.cpp:83-148) over restated clouds"""
    from oracle import oracle as O
    return O.register_point_clouds(clouds, t[0], t[1], t[2], rot_step)


REG_SETTINGS = (((12.5, -3.25, 310.0), 17.5), ((0.0, 0.0, 0.0), -120.0))


def capacities(counts, offsets, total, seams):
    """the capacities of the clamped download: 1, total - 1, total, and offsets[s] - 1, offsets[s], offsets[s] + 1 of a handful of seam
    segments -- a capacity that ends exactly on a segment seam among them; only those > 0"""
    want = {1, total - 1, total}
    for s in seams:
        o = int(offsets[s])
        want |= {o - 1, o, o + 1}
    return sorted(c for c in want if c > 0)


def seam_segments(W, H, counts):
    """a handful of segments whose offsets the clamped capacities straddle: the first segments with a count at or behind a block-of-4, 1024 and
    part seam, and the last segment with a count"""
    _, _, n_segs, _ = geometry(W, H)
    nz = np.flatnonzero(counts)
    if not len(nz):
        return []
    picks = {int(nz[-1])}
    for at in (4, 1024, part_len(n_segs)):
        later = nz[nz >= at]
        if len(later):
            picks.add(int(later[0]))
    return sorted(picks)[:4]


def bits_differ(got, want, produced=False):
    """Number of float32 entries that differ bit for bit (+0 is not -0, a NaN's sign and payload count); with `produced` -- values the
    arithmetic made, not copies -- a NaN of the reference only asks for a NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if produced:
        diff &= ~(np.isnan(want) & np.isnan(got))
    return int(diff.sum())


def holds_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENTINEL_BITS).any())
