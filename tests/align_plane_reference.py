"""NumPy restatement of the point-to-plane turntable refinement (the rule: include/sl3d_align_plane.h; the library's arithmetic:
3dscan_amd/csrc/sl3d_align_plane.h): a view's normals, one pass, the solve and the loop, on the shared pieces of tests/align_reference.py
(the step, the centre pixel, the squared distance, the cameras and the scene builders).

Every operation is one float64 operation in the header's order; the sums are exact Python integers, the solve rounds each moment once.

normals(points, valid, normal_edge) -> (H, W, 3) float32, NaN where a pixel has no normal
pass_sums(points, valid, cam, col0, row0, est, ox, oz, rng, max_dist, normal_edge, window) -> (V - 1, 18) int64
solve(sums, rng, ox, oz, est) -> (est_out float64[4], dict(n, rms_xz, rms_y, degenerate)); rms_xz carries rms_plane, rms_y is NaN
refine(points, valid, cam, col0, row0, tx, ty, tz, rot_step, rng, max_dist, normal_edge, window, iterations) -> the dict of
Scanner.refine_turntable_plane"""
import math

import numpy as np

import align_reference as AR

WORDS = 18
Q_ONE = 65536.0
LIMIT = 262144.0
STEPS = 8
PIVOT = 2.0**-40
F8 = np.float64


# ---- the normals ------------------------------------------------------------------------------------------------------------------------------
def normal_of(q, l, r, u, d, normal_edge):
    """q, l, r, u, d: (n, 3) float32 -- a pixel's point and its left, right, upper and lower neighbours, all under valid bytes of 1 inside
    the frame window -> (n, 3) float32 normals, NaN where there is none"""
    edge2 = F8(np.float32(normal_edge)) * F8(np.float32(normal_edge))
    with np.errstate(all="ignore"):
        ok = np.ones(len(q), bool)
        for m in (q, l, r, u, d):
            ok &= np.isfinite(m).all(axis=1)
        c = q.astype(F8)
        for m in (l, r, u, d):
            ok &= AR.dist2(m, c) <= edge2
        a, b = r.astype(F8) - l.astype(F8), d.astype(F8) - u.astype(F8)
        nx = (a[:, 1] * b[:, 2]) - (a[:, 2] * b[:, 1])
        ny = (a[:, 2] * b[:, 0]) - (a[:, 0] * b[:, 2])
        nz = (a[:, 0] * b[:, 1]) - (a[:, 1] * b[:, 0])
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok &= (ln > 0.0) & np.isfinite(ln)
        n = np.stack([nx / ln, ny / ln, nz / ln], axis=1).astype(np.float32)
    n[~ok] = np.nan
    return n


def normals(points, valid, normal_edge):
    """points (H, W, 3) float32, valid (H, W) uint8 -> (H, W, 3) float32"""
    H, W = valid.shape
    out = np.full((H, W, 3), np.nan, np.float32)
    if H < 3 or W < 3:
        return out
    v = valid == 1
    inner = v[1:-1, 1:-1] & v[1:-1, :-2] & v[1:-1, 2:] & v[:-2, 1:-1] & v[2:, 1:-1]
    r, c = np.nonzero(inner)
    r, c = r + 1, c + 1
    out[r, c] = normal_of(points[r, c], points[r, c - 1], points[r, c + 1], points[r - 1, c], points[r + 1, c], normal_edge)
    return out


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------------
def scale(rng):
    return F8(Q_ONE) / F8(np.float32(rng))


def features(p, q, n, ox, oz, Qp):
    """p, q, n: (m, 3) float32 -> (all five in range (m,), the integers (m, 5) int64, 0 where out of range)"""
    ox, oz, Qp = F8(ox), F8(oz), F8(Qp)
    with np.errstate(all="ignore"):
        nx, ny, nz = (n[:, k].astype(F8) for k in range(3))
        px, pz, qx, qz = p[:, 0].astype(F8) - ox, p[:, 2].astype(F8) - oz, q[:, 0].astype(F8) - ox, q[:, 2].astype(F8) - oz
        A = nx * px + nz * pz
        B = nz * px - nx * pz
        D = ny * (p[:, 1].astype(F8) - q[:, 1].astype(F8)) - (nx * qx + nz * qz)
        e = np.stack([A * Qp, B * Qp, nx * F8(Q_ONE), nz * F8(Q_ONE), D * Qp], axis=1)
        ok = np.abs(e) < LIMIT
        f = np.where(ok, np.rint(np.where(ok, e, 0.0)), 0.0).astype(np.int64)
    return ok.all(axis=1), f


def best_candidates(p, ph, tp, tv, cam, col0, row0, window):
    """steps 2 - 4 of include/sl3d_align.h for sources p (turned: ph): (best d2, the candidate's point, its row, its column), +inf and -1
    where a source has no candidate"""
    H, W = tv.shape
    n = len(p)
    cc, rr, ok = AR.centre(ph, cam, col0, row0)
    cc, rr = np.where(ok, cc, 0.0).astype(np.int64), np.where(ok, rr, 0.0).astype(np.int64)
    best = np.full(n, np.inf)
    q = np.zeros((n, 3), np.float32)
    br, bc = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    tfinite = np.isfinite(tp).all(axis=2)
    for dy in range(-window, window + 1):                     # row-major: a later candidate must be strictly nearer
        for dx in range(-window, window + 1):
            r, c = rr + dy, cc + dx
            inside = ok & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            ri, ci = np.where(inside, r, 0), np.where(inside, c, 0)
            cand = inside & (tv[ri, ci] == 1) & tfinite[ri, ci]
            d2 = AR.dist2(tp[ri, ci], ph)
            with np.errstate(invalid="ignore"):
                better = cand & (d2 < best)
            best = np.where(better, d2, best)
            q[better] = tp[ri, ci][better]
            br, bc = np.where(better, ri, br), np.where(better, ci, bc)
    return best, q, br, bc


def pair_words(sp, sv, tp, tv, tn, cam, col0, row0, est, ox, oz, rng, max_dist, window):
    """the 18 words of one pair: source planes sp / sv, target planes tp / tv and the target's normals tn (H, W, 3) float32"""
    p = sp.reshape(-1, 3)
    src = (sv.reshape(-1) == 1) & np.isfinite(p).all(axis=1)
    p = p[src]
    words = [0] * WORDS
    words[16] = int(src.sum())
    best, q, br, bc = best_candidates(p, AR.step(p, est), tp, tv, cam, col0, row0, window)
    thr2 = F8(np.float32(max_dist)) * F8(np.float32(max_dist))
    near = np.isfinite(best) & (best <= thr2)
    n = tn[np.where(near, br, 0), np.where(near, bc, 0)]
    has = near & ~np.isnan(n[:, 0])
    words[17] = int((near & ~has).sum())
    ok, f = features(p, q, np.where(has[:, None], n, np.float32(0.0)), ox, oz, scale(rng))
    acc = has & ok
    f = f[acc]
    words[0] = int(acc.sum())
    k = 1
    for i in range(5):
        for j in range(i, 5):
            words[k] = int((f[:, i] * f[:, j]).sum())                        # exact in int64: a product is below 2^36, a frame below 2^25 pixels
            k += 1
    return words


def pass_sums(points, valid, cam, col0, row0, est, ox, oz, rng, max_dist, normal_edge, window, nrm=None):
    """points (V, H, W, 3) float32, valid (V, H, W) uint8: pair j is (source view j + 1, target view j); nrm: the targets' normals, if the
    caller has them"""
    nrm = [normals(points[j], valid[j], normal_edge) for j in range(len(points) - 1)] if nrm is None else nrm
    return np.array([pair_words(points[j + 1], valid[j + 1], points[j], valid[j], nrm[j], cam, col0, row0, est, ox, oz, rng, max_dist, window)
                     for j in range(len(points) - 1)], dtype=np.int64).reshape(-1, WORDS)


# ---- the solve and the loop -------------------------------------------------------------------------------------------------------------------
def moments(sums):
    """(N, M): the pairs' words added as Python integers, each moment rounded to double once, the normals' rows and columns scaled by 2^-16"""
    S = [sum(int(v) for v in col) for col in np.asarray(sums, dtype=np.int64).reshape(-1, WORDS).T]
    M = [[0.0] * 5 for _ in range(5)]
    k = 1
    for i in range(5):
        for j in range(i, 5):
            nrm = (i in (2, 3)) + (j in (2, 3))
            M[i][j] = M[j][i] = float(S[k]) * (2.0**-32 if nrm == 2 else 2.0**-16 if nrm == 1 else 1.0)
            k += 1
    return S[0], M


def solve(sums, rng, ox, oz, est):
    N, M = moments(sums)
    est = np.array(est, dtype=F8)
    bad = dict(n=N, rms_xz=math.nan, rms_y=math.nan, degenerate=True)
    if N < 3:
        return est, bad
    Qp, ox, oz = float(scale(rng)), float(ox), float(oz)
    th = math.atan2(float(est[1]), float(est[0]))
    c, s = math.cos(th), math.sin(th)
    tpx, tpz = (float(est[2]) - ox) * Qp, (float(est[3]) - oz) * Qp
    u, w = (1.0 - c) * tpx + s * tpz, (1.0 - c) * tpz - s * tpx
    for it in range(STEPS + 1):
        c, s = math.cos(th), math.sin(th)
        g = (c, s, u, w, 1.0)
        Mg = [(((M[i][0] * g[0] + M[i][1] * g[1]) + M[i][2] * g[2]) + M[i][3] * g[3]) + M[i][4] * g[4] for i in range(5)]
        if it == STEPS:
            break
        j0, j1 = -s, c
        bu, bw, bt = Mg[2], Mg[3], j0 * Mg[0] + j1 * Mg[1]
        Huu, Huw, Hww = M[2][2], M[2][3], M[3][3]
        Hut, Hwt = M[2][0] * j0 + M[2][1] * j1, M[3][0] * j0 + M[3][1] * j1
        Htt = j0 * (M[0][0] * j0 + M[0][1] * j1) + j1 * (M[1][0] * j0 + M[1][1] * j1)
        d0 = Huu
        if not d0 > PIVOT * Huu:
            return est, bad
        l10, l20 = Huw / d0, Hut / d0
        d1 = Hww - l10 * Huw
        if not d1 > PIVOT * Hww:
            return est, bad
        e21 = Hwt - l10 * Hut
        l21 = e21 / d1
        d2 = (Htt - l20 * Hut) - l21 * e21
        if not d2 > PIVOT * Htt:
            return est, bad
        y0 = -bu
        y1 = -bw - l10 * y0
        y2 = (-bt - l20 * y0) - l21 * y1
        z2 = y2 / d2
        z1 = y1 / d1 - l21 * z2
        z0 = (y0 / d0 - l10 * z1) - l20 * z2
        u, w, th = u + z0, w + z1, th + z2
        if not (math.isfinite(u) and math.isfinite(w) and math.isfinite(th)):
            return est, bad
    if c == 1.0:
        return est, bad
    m = 1.0 - c
    det = m * m + s * s
    tx, tz = (m * u - s * w) / det, (s * u + m * w) / det
    E = (((g[0] * Mg[0] + g[1] * Mg[1]) + g[2] * Mg[2]) + g[3] * Mg[3]) + g[4] * Mg[4]
    if not E > 0.0 and E == E:
        E = 0.0
    ex, ez = ox + tx / Qp, oz + tz / Qp
    rms = math.sqrt(E / float(N)) / Qp if E == E else math.nan
    if not (math.isfinite(ex) and math.isfinite(ez) and math.isfinite(rms)):
        return est, bad
    return np.array([c, s, ex, ez]), dict(n=N, rms_xz=rms, rms_y=math.nan, degenerate=False)


def refine(points, valid, cam, col0, row0, tx, ty, tz, rot_step, rng, max_dist, normal_edge, window=2, iterations=20):
    ox, oz = float(np.float32(tx)), float(np.float32(tz))
    est = AR.first_estimate(tx, tz, rot_step)
    nrm = [normals(points[j], valid[j], normal_edge) for j in range(len(points) - 1)]          # once, before the first pass
    log, before, stats, sources = [], None, None, 0
    for i in range(iterations):
        words = pass_sums(points, valid, cam, col0, row0, est, ox, oz, rng, max_dist, normal_edge, window, nrm)
        nxt, stats = solve(words, rng, ox, oz, est)
        sources = int(words[:, 16].sum())
        log.append(dict(est=est.copy(), n=stats["n"], sources=sources, rms_xz=stats["rms_xz"], rms_y=stats["rms_y"], lost=int(words[:, 17].sum())))
        if stats["degenerate"]:
            break
        est = nxt
        if before is not None and np.array_equal(words, before):
            break
        before = words
    return dict(tx=np.float32(est[2]), ty=np.float32(ty), tz=np.float32(est[3]), rot_step=np.float32(math.atan2(est[1], est[0]) * 180.0 * 7.0 / 22.0),
                est=est, n=stats["n"], sources=sources, rms_xz=stats["rms_xz"], rms_y=stats["rms_y"], degenerate=stats["degenerate"],
                n_done=len(log), log=log)


# ---- crafted planes for the special cases (tests/test_gpu_align_plane_cases.py) -------------------------------------------------------------
SPECIAL = dict(W=AR.SPECIAL["W"], H=AR.SPECIAL["H"], est=AR.SPECIAL["est"], max_dist=AR.SPECIAL["max_dist"], normal_edge=1.0)


def special_planes(cam, col0, row0):
    """Two views for the special cases of a point-to-plane pass, under the identity estimate (the idea of align_reference.special_planes).
    Every target pixel holds the point of its own pixel centre at depth 100 mm, snapped to 1/64 mm, under an INVALID byte; a case makes a
    pixel and its four neighbours valid (a `plus`), as they are or with points of its own.  The sources sit one per pixel from the source
    view's first pixel on.  Returns points (2, H, W, 3) float32, valid (2, H, W) uint8, the names of the cases in source order, and `at`:
    name -> (row, column) of the case's target pixel."""
    W, H, edge = SPECIAL["W"], SPECIAL["H"], np.float32(SPECIAL["normal_edge"])
    snap = lambda P: (np.round(np.asarray(P, F8) * 64.0) / 64.0).astype(np.float32)
    base = snap(AR.backproject(cam, W, H, col0, row0, 100.0))
    tp, tv = base.copy(), np.zeros((H, W), np.uint8)
    src, names, at = [], [], {}
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))

    def plus(r, c, flat=None):
        """(r, c) and its neighbours inside the frame valid; flat: their points on the plane z = const through the centre, 0.25 mm apart:
        a = (0.5, 0, 0), b = (0, 0.5, 0), the normal (0, 0, 1) exactly"""
        for dr, dc in ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)):
            if 0 <= r + dr < H and 0 <= c + dc < W:
                assert tv[r + dr, c + dc] == 0
                tv[r + dr, c + dc] = 1
                if flat is not None:
                    tp[r + dr, c + dc] = flat + f([0.25 * dc, 0.25 * dr, 0.0])

    def case(name, r, c, p=None):
        names.append(name)
        at[name] = (r, c)
        src.append(np.asarray(tp[r, c] if p is None else p, np.float32))
    plus(3, 4)
    case("a normal", 3, 4, base[3, 4] + f([0.0625, 0.0, 0.0]))
    plus(3, 10)
    tv[3, 9] = 0
    case("a neighbour invalid", 3, 10)
    plus(3, 16)
    tp[2, 16] = f([np.nan, tp[2, 16][1], tp[2, 16][2]])
    case("a neighbour NaN under a valid byte", 3, 16)
    plus(3, 22)
    tp[3, 23] = tp[3, 22] + f([edge, 0.0, 0.0])                              # (coordinates are multiples of 1/64: the sum is exact)
    case("a neighbour exactly at normal_edge", 3, 22)
    plus(3, 28)
    tp[3, 29] = tp[3, 28] + f([edge, 0.0, 0.0])
    tp[3, 29][0] = up(tp[3, 29][0])
    case("a neighbour one ulp beyond normal_edge", 3, 28)
    plus(3, 34)
    tp[4, 34] = tp[3, 34] - f([0.0, 0.0, edge])
    tp[4, 34][2] = np.nextafter(tp[4, 34][2], f(-np.inf))
    case("a lower neighbour one ulp beyond normal_edge", 3, 34)
    plus(9, 4)
    tp[8, 4], tp[10, 4] = tp[9, 3], tp[9, 5]                                 # up = left, down = right: b = a, a zero cross product
    case("collinear neighbours", 9, 4)
    plus(9, 10)
    tp[9, 9] = tp[9, 11]                                                     # left = right: a = 0
    case("coincident neighbours", 9, 10)
    plus(0, 8), plus(H - 1, 20), plus(9, 0), plus(9, W - 1), plus(H - 1, W - 1)
    for name, (r, c) in (("top border", (0, 8)), ("bottom border", (H - 1, 20)), ("left border", (9, 0)), ("right border", (9, W - 1)),
                         ("corner", (H - 1, W - 1))):
        case(name, r, c)
    plus(9, 17)                                                              # (9, 16) is valid, but (9, 15) is not: the best candidate of the source
    case("best without a normal, a farther one with", 9, 16)                 # on (9, 16) has no normal, its neighbour (9, 17) has
    plus(15, 36, flat=base[15, 36])                                          # (the largest x of all sources: the others stay in range)
    case("feature exactly at the range limit", 15, 36)                       # the test puts ox 4 * range below this source's x
    below = base[19, 36].copy()
    below[0] = np.nextafter(base[15, 36][0], f(-np.inf))
    plus(19, 36, flat=below)
    case("feature just below the range limit", 19, 36)
    plus(15, 20, flat=base[15, 20])
    case("a flat plus: the normal (0, 0, 1)", 15, 20)
    sp, sv = base.copy(), np.zeros((H, W), np.uint8)                          # (finite points under invalid bytes everywhere else)
    n = len(src)
    sp.reshape(-1, 3)[:n], sv.reshape(-1)[:n] = np.stack(src), 1
    return np.stack([tp, sp]), np.stack([tv, sv]), names, at
