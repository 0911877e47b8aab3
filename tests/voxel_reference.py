"""NumPy restatement of the voxel grid (the rule: include/sl3d_voxel.h; the device: sl3d_voxel_grid, k_voxel_insert / k_voxel_count /
k_voxel_scatter; the C arithmetic: 3dscan_amd/csrc/sl3d_voxel.h), written from the rule and from nothing else: IEEE doubles and int64,
np.unique for the cells.  It includes the hash and the capacity of the table, because the crafted clouds (tests/voxel_cases.py) need them
to make collisions."""
import numpy as np

LIMIT = 1 << 20
Q_ONE = 16777216.0
EMPTY = 0xFFFFFFFFFFFFFFFF


def cell(x, leaf):
    """(the floored cell index as float64, is it in range) of float32 coordinates of any shape"""
    L = np.float64(np.float32(leaf))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = np.floor(np.asarray(x, dtype=np.float32).astype(np.float64) / L)
        return c, (c >= -LIMIT) & (c < LIMIT)


def key(c):
    """the 63-bit keys (uint64) of (n, 3) in-range cell indices"""
    k = np.asarray(c).astype(np.int64) + LIMIT
    return ((k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]).astype(np.uint64)


def q(x, c, leaf):
    """the fixed-point offset (int64) of float32 coordinates x inside their cells c"""
    L = np.float64(np.float32(leaf))
    base = c * L
    d = np.asarray(x, dtype=np.float32).astype(np.float64) - base
    return np.rint((d / L) * Q_ONE).astype(np.int64)


def centroid(c, leaf, S, count):
    """the float32 centroid coordinate of cells of index c, sums S (int64) and counts"""
    L = np.float64(np.float32(leaf))
    base = c * L
    return (base + ((np.asarray(S, dtype=np.int64).astype(np.float64) / np.asarray(count).astype(np.float64)) / Q_ONE) * L).astype(np.float32)


def mix(k):
    """the splitmix64 finaliser"""
    k = np.array(k, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30)
        k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27)
        k *= np.uint64(0x94d049bb133111eb)
        k ^= k >> np.uint64(31)
    return k


def table_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return cap


def home_slot(k, capacity):
    return (mix(k) & np.uint64(capacity - 1)).astype(np.int64)


def grid(xyz, leaf, min_points=1, centroid_mode=True):
    """(xyz float32 (m, 3), first int32 (m,), count uint32 (m,), [points in, points dropped, occupied cells, cells kept]) of rules 1-7"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    c, ok = cell(xyz, leaf)
    sample = np.isfinite(xyz).all(axis=1) & ok.all(axis=1)
    idx = np.flatnonzero(sample)
    if len(idx) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32), [n, n, 0, 0]
    cs = c[idx]
    _, first, inv, cnt = np.unique(key(cs), return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    pos = xyz[idx[first]].copy()                       # the bits of p_first: first mode, and every one-point cell
    if centroid_mode:
        S = np.zeros((len(first), 3), np.int64)
        np.add.at(S, inv, q(xyz[idx], cs, leaf))
        cen = centroid(cs[first], leaf, S, cnt[:, None])
        many = cnt > 1
        pos[many] = cen[many]
    order = np.argsort(first, kind="stable")
    keep = order[cnt[order] >= min_points]
    return (pos[keep], idx[first][keep].astype(np.int32), cnt[keep].astype(np.uint32), [n, n - len(idx), len(first), len(keep)])
