"""NumPy restatement of the TSDF volume (the rule: include/sl3d_tsdf.h; the library's arithmetic: 3dscan_amd/csrc/sl3d_tsdf.h): one
integration of views into the planes sum / weight, and the extraction of the oriented points of the zero level.

Every operation is one float64 operation in the header's order (NumPy evaluates a * b + c as two roundings); sum and weight are exact
integers.

turns(est, n) -> (n, 2) float64: (c_m, s_m) of the turntable indices 0 .. n - 1, by the recurrence
integrate(sum, weight, vol, points, valid, cam, col0, row0, est, first_step=0) -> (samples taken, voxels with weight > 0); in place
extract(sum, weight, vol, min_weight) -> (xyz float32 (m, 3), normals float32 (m, 3), edge int32 (m,), [voxels, known, m])
vol: dict(origin=float32[3], voxel=float32, trunc=float32, dims=(nx, ny, nz)); sum / weight: flat int32 / uint32 of nx * ny * nz words,
v = (k * ny + j) * nx + i.  cam: float64[26] as in tests/align_reference.py."""
import numpy as np

F8 = np.float64
Q_ONE = 32767.0
MAX_STEPS = 65535


def new_volume(vol):
    n = int(np.prod(vol["dims"]))
    return np.zeros(n, np.int32), np.zeros(n, np.uint32)


def turns(est, n):
    c, s = F8(est[0]), F8(est[1])
    out = np.empty((n, 2), F8)
    cm, sm = F8(1.0), F8(0.0)
    for m in range(n):
        out[m] = cm, sm
        cn = cm * c
        cn = cn - sm * s
        sn = sm * c
        sn = sn + cm * s
        cm, sm = cn, sn
    return out


def centres(vol):
    """(n, 3) float64 voxel centres in ascending v, and their (i, j, k)"""
    nx, ny, nz = vol["dims"]
    L = F8(np.float32(vol["voxel"]))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    o = np.asarray(vol["origin"], np.float32).astype(F8)
    X = ijk.astype(F8) + 0.5
    X = X * L
    X = X + o
    return X, ijk


def step(X, turn, tx, tz):
    """step 1: X (n, 3) float64 into the view's own frame by the inverse turn (c_m, -s_m, tx, tz)"""
    c, s = F8(turn[0]), -F8(turn[1])
    tx, tz = F8(tx), F8(tz)
    x = X[:, 0] - tx
    z = X[:, 2] - tz
    px = c * x
    px = px - s * z
    px = px + tx
    pz = s * x
    pz = pz + c * z
    pz = pz + tz
    return np.stack([px, X[:, 1], pz], axis=1)


def project(P, cam):
    """step 2: (u, v, xc.z, ok) -- the camera algebra of align_reference.centre with u and v unrounded"""
    cam = np.asarray(cam, dtype=F8)
    Rc, tc, K = cam[0:9], cam[9:12], cam[12:21]
    k1, k2, p1, p2, k3 = cam[21:26]
    with np.errstate(all="ignore"):
        xc = [((Rc[3 * i] * P[:, 0] + Rc[3 * i + 1] * P[:, 1]) + Rc[3 * i + 2] * P[:, 2]) + tc[i] for i in range(3)]
        ok = (xc[2] > 0.0) & np.isfinite(xc[2])
        xn, yn = xc[0] / xc[2], xc[1] / xc[2]
        r2 = xn * xn + yn * yn
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = xn * rad + (2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn))
        yd = yn * rad + (p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn)
        w = (K[6] * xd + K[7] * yd) + K[8]
        u, v = ((K[0] * xd + K[1] * yd) + K[2]) / w, ((K[3] * xd + K[4] * yd) + K[5]) / w
    return u, v, xc[2], ok


def cell(u, v, W, H, col0, row0):
    """step 3: (c, r, a, b, ok); c and r are 0 where there is no cell"""
    with np.errstate(all="ignore"):
        flu, flv = np.floor(u), np.floor(v)
        fu, fv = flu - F8(col0), flv - F8(row0)
        ok = (0.0 <= fu) & (fu + 1.0 < F8(W)) & (0.0 <= fv) & (fv + 1.0 < F8(H))
        a, b = u - flu, v - flv
    c = np.where(ok, fu, 0.0).astype(np.int64)
    r = np.where(ok, fv, 0.0).astype(np.int64)
    return c, r, a, b, ok


def depth(q, cam):
    """step 4: the camera depth of the points q (n, 3) float32"""
    cam = np.asarray(cam, dtype=F8)
    Rc, tc = cam[0:9], cam[9:12]
    q = q.astype(F8)
    with np.errstate(all="ignore"):
        z = Rc[6] * q[:, 0]
        z = z + Rc[7] * q[:, 1]
        z = z + Rc[8] * q[:, 2]
        z = z + tc[2]
    return z


def quant(z, a, b, zc, T):
    """steps 5 to 7: z (n, 4) = z00, z10, z01, z11 -> (ok, q int32; 0 where there is no sample)"""
    T = F8(T)
    with np.errstate(all="ignore"):
        spread = z.max(axis=1) - z.min(axis=1)
        ok = spread <= T
        one_a, one_b = 1.0 - a, 1.0 - b
        top = z[:, 0] * one_a
        top = top + z[:, 1] * a
        top = top * one_b
        bot = z[:, 2] * one_a
        bot = bot + z[:, 3] * a
        bot = bot * b
        zq = top + bot
        sdf = zq - zc
        ok &= sdf >= -T
        d = sdf / T
        d = np.where(d > 1.0, 1.0, d)
        q = np.rint(np.where(ok, d, 0.0) * Q_ONE)
    return ok, np.where(ok, q, 0.0).astype(np.int32)


def view_votes(X, turn, tx, tz, points, valid, cam, col0, row0, T):
    """steps 1 to 7 of every centre for one view: (ok, q).  points (H, W, 3) float32, valid (H, W) uint8"""
    H, W = valid.shape
    u, v, zc, ok = project(step(X, turn, tx, tz), cam)
    c, r, a, b, in_cell = cell(u, v, W, H, col0, row0)
    ok = ok & in_cell
    c, r = np.where(ok, c, 0), np.where(ok, r, 0)
    usable = (valid == 1) & np.isfinite(points).all(axis=2)
    z = np.zeros((len(X), 4), F8)
    for kk, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        rr, cc = np.minimum(r + dy, H - 1), np.minimum(c + dx, W - 1)
        ok = ok & usable[rr, cc]
        z[:, kk] = depth(points[rr, cc], cam)
    z = np.where(ok[:, None], z, 0.0)
    good, q = quant(z, np.where(ok, a, 0.0), np.where(ok, b, 0.0), np.where(ok, zc, 0.0), T)
    ok = ok & good
    return ok, np.where(ok, q, 0).astype(np.int32)


def integrate(sum_, weight, vol, points, valid, cam, col0, row0, est, first_step=0):
    """points (V, H, W, 3) float32, valid (V, H, W) uint8: view j has turntable index first_step + j.  sum_ / weight are updated in place."""
    V = len(points)
    assert first_step >= 0 and first_step + V <= MAX_STEPS
    X, _ = centres(vol)
    tab = turns(est, first_step + V)
    T = F8(np.float32(vol["trunc"]))
    taken = 0
    for j in range(V):
        ok, q = view_votes(X, tab[first_step + j], est[2], est[3], points[j], valid[j], cam, col0, row0, T)
        sum_ += q
        weight += ok.astype(np.uint32)
        taken += int(ok.sum())
    return taken, int((weight > 0).sum())


# ---- extraction ------------------------------------------------------------------------------------------------------------------------------
def _shift(a, axis, d, fill):
    """a's neighbour at +d (d = 1) or -d (d = -1) along `axis` of a (nz, ny, nx) array; `fill` outside"""
    out = np.full_like(a, fill)
    ax = 2 - axis
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if d == 1:
        src[ax], dst[ax] = slice(1, None), slice(0, -1)
    else:
        src[ax], dst[ax] = slice(0, -1), slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def gradients(f, known):
    """g[b] (nz, ny, nx) float64 for b = 0, 1, 2; meaningless where a voxel is not known"""
    g = []
    for b in range(3):
        kp, km = _shift(known, b, 1, False), _shift(known, b, -1, False)
        fp, fm = _shift(f, b, 1, 0.0), _shift(f, b, -1, 0.0)
        with np.errstate(all="ignore"):
            both = (fp - fm) * 0.5
            plus = fp - f
            minus = f - fm
        g.append(np.where(kp & km, both, np.where(kp, plus, np.where(km, minus, 0.0))))
    return g


def extract(sum_, weight, vol, min_weight=1):
    nx, ny, nz = vol["dims"]
    n = nx * ny * nz
    L = F8(np.float32(vol["voxel"]))
    known = (weight.astype(np.int64) >= int(min_weight)).reshape(nz, ny, nx)
    with np.errstate(all="ignore"):
        f = np.where(known, sum_.astype(F8).reshape(nz, ny, nx) / weight.astype(F8).reshape(nz, ny, nx), 0.0)
    X, _ = centres(vol)
    X = X.reshape(nz, ny, nx, 3)
    g = gradients(f, known)
    rows = []
    for a in range(3):
        f1, k1 = _shift(f, a, 1, 0.0), _shift(known, a, 1, False)
        cross = known & k1 & ((f < 0.0) != (f1 < 0.0))
        v0 = np.flatnonzero(cross.ravel())
        if not len(v0):
            continue
        idx = np.unravel_index(v0, (nz, ny, nx))
        f0, f1 = f[idx], f1[idx]
        t = f0 / (f0 - f1)
        pos = X[idx].copy()
        pos[:, a] = pos[:, a] + t * L
        nrm = np.empty((len(v0), 3), F8)
        for b in range(3):
            g1 = _shift(g[b], a, 1, 0.0)
            nb = g[b][idx] * (1.0 - t)
            nb = nb + g1[idx] * t
            nrm[:, b] = nb
        ln = nrm[:, 0] * nrm[:, 0]
        ln = ln + nrm[:, 1] * nrm[:, 1]
        ln = ln + nrm[:, 2] * nrm[:, 2]
        ln = np.sqrt(ln)
        ok = (ln > 0.0) & np.isfinite(ln)
        with np.errstate(all="ignore"):
            unit = nrm / ln[:, None]
        unit = np.where(ok[:, None], unit, np.nan)
        rows.append((3 * v0 + a, pos.astype(np.float32), unit.astype(np.float32)))
    if not rows:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), [n, int(known.sum()), 0]
    edge = np.concatenate([r[0] for r in rows])
    order = np.argsort(edge, kind="stable")
    xyz = np.concatenate([r[1] for r in rows])[order]
    nrm = np.concatenate([r[2] for r in rows])[order]
    return xyz, nrm, edge[order].astype(np.int32), [n, int(known.sum()), len(edge)]


def bounds(cloud, voxel, margin=2):
    """origin float32[3] and dims of the volume around a cloud: the rule of scanner.tsdf_bounds"""
    p = np.asarray(cloud, F8).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    L = float(np.float32(voxel))
    origin = ((np.floor(p.min(axis=0) / L) - margin) * L).astype(np.float32)
    dims = np.ceil((p.max(axis=0) - origin.astype(F8)) / L).astype(np.int64) + margin
    return origin, tuple(int(max(d, 1)) for d in dims)
