"""The sub-pixel triangulation of include/sl3d.h (sl3d_triangulate_subpixel) restated in NumPy, float64, written from the
definition alone (shared by tests/test_subpixel_arith.py and tests/test_gpu_subpixel.py):

  coordinates   xs = (double)fw_v * ((double)unwrapped_v / ((2.0 * 22.0) / 7.0)), ys likewise: the arguments of stage 5's lrint
  undistortion  cvUndistortPoints' five fixed-point iterations on (p - c) * (1 / f), then K * (x, y, 1) and the homogeneous divide
  solve         P (4 x 3), F (4) of 7/triangulation.cpp:1152-1188, V = ((P^T P)^-1 P^T) F in that order, the inverse by the adjugate,
                zero where the determinant is zero (cvInvert)
  residual      h = A_D (X, 1), e_D = (h0 / h2 - u_D, h1 / h2 - v_D), (float)sqrt(e_c . e_c + e_p . e_p)
  rejection     only for a finite max_residual: !((double)residual <= max_residual) on the float
"""
import numpy as np

TWO_PI_REF = (2.0 * 22.0) / 7.0


def continuous(unwrapped, fw):
    """The double stage 5 hands to lrint, per pixel of an absolute-phase plane (float32)."""
    assert unwrapped.dtype == np.float32
    return np.float64(fw) * (unwrapped.astype(np.float64) / TWO_PI_REF)


def correspondences(unw_v, unw_h, valid_v, valid_h, fw_v, fw_h):
    """(H, W, 2) float64 (xs, ys); NaN where either per-axis valid byte is not 1 (sl3d_get_correspondences_subpixel)."""
    xy = np.stack([continuous(unw_v, fw_v), continuous(unw_h, fw_h)], axis=-1)
    xy[~((valid_v == 1) & (valid_h == 1))] = np.nan
    return xy


def undistort_reproject(px, py, K, d):
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = (float(v) for v in np.asarray(d, np.float64).ravel())
    ifx, ify = 1.0 / K[0, 0], 1.0 / K[1, 1]
    x0, y0 = (px - K[0, 2]) * ifx, (py - K[1, 2]) * ify
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    h = [K[i, 0] * x + K[i, 1] * y + K[i, 2] for i in range(3)]
    return h[0] / h[2], h[1] / h[2]


def _inv3(M):
    """cvInvert of 3 x 3 matrices (..., 3, 3): adjugate over determinant, zeros where the determinant is zero."""
    m = lambda i, j: M[..., i, j]
    det = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) + m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0))
    with np.errstate(divide="ignore"):
        d = np.where(det != 0.0, 1.0 / np.where(det != 0.0, det, 1.0), 0.0)
    t = [m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2), m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1),
         m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0), m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2),
         m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0), m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1), m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)]
    return np.stack([v * d for v in t], axis=-1).reshape(M.shape)


def solve(A_cam, A_proj, u, v, up, vp):
    """X (n, 3) of the 4 x 3 least-squares system at the undistorted points (n,) each: V = ((P^T P)^-1 P^T) F, sums in index order."""
    Ac, Ap = np.asarray(A_cam, np.float64).reshape(3, 4), np.asarray(A_proj, np.float64).reshape(3, 4)
    rows = [(Ac, 0, u), (Ac, 1, v), (Ap, 0, up), (Ap, 1, vp)]
    P = np.stack([np.stack([A[r, q] - t * A[2, q] for q in range(3)], axis=-1) for A, r, t in rows], axis=-2)     # (n, 4, 3)
    F = np.stack([A[2, 3] * t - A[r, 3] for A, r, t in rows], axis=-1)                                            # (n, 4)
    I1 = np.stack([np.stack([sum(P[:, a, i] * P[:, a, j] for a in range(4)) for j in range(3)], axis=-1) for i in range(3)], axis=-2)
    inv = _inv3(I1)
    I2 = np.stack([np.stack([sum(inv[:, i, k] * P[:, a, k] for k in range(3)) for a in range(4)], axis=-1) for i in range(3)], axis=-2)   # (n, 3, 4)
    return np.stack([sum(I2[:, i, a] * F[:, a] for a in range(4)) for i in range(3)], axis=-1)


def reprojection_error2(A, X, u, v):
    A = np.asarray(A, np.float64).reshape(3, 4)
    h = [A[i, 0] * X[:, 0] + A[i, 1] * X[:, 1] + A[i, 2] * X[:, 2] + A[i, 3] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        eu, ev = h[0] / h[2] - u, h[1] / h[2] - v
    return eu * eu + ev * ev


def triangulate(xy, valid, cal, A_cam, A_proj, origin=(0, 0), max_residual=np.inf):
    """Steps 2-6 over one view.  xy: (H, W, 2) projector coordinates (continuous, or the integers of c_p_map), valid: the merged valid
    map before the call, cal: the tuple (Kc, dc, rc, tc, Kp, dp, rp, tp), origin: (col0, row0) of the window in the camera frame.
    Returns dict(points float32 NaN where not valid after the call, ipoints float64 0 there, residual float32 NaN where not
    triangulated, valid uint8 after the call, counts (triangulated, rejected))."""
    Kc, dc, _, _, Kp, dp, _, _ = cal
    H, W = valid.shape
    m = valid == 1
    rows, cols = np.nonzero(m)
    u, v = undistort_reproject(cols.astype(np.float64) + origin[0], rows.astype(np.float64) + origin[1], Kc, dc)
    up, vp = undistort_reproject(xy[m][:, 0].astype(np.float64), xy[m][:, 1].astype(np.float64), Kp, dp)
    X = solve(A_cam, A_proj, u, v, up, vp)
    with np.errstate(invalid="ignore"):
        res = np.sqrt(reprojection_error2(A_cam, X, u, v) + reprojection_error2(A_proj, X, up, vp)).astype(np.float32)
    rejected = ~(res.astype(np.float64) <= max_residual) if np.isfinite(max_residual) else np.zeros(len(res), bool)
    out_valid = valid.copy()
    out_valid[rows[rejected], cols[rejected]] = 0
    points = np.full((H, W, 3), np.nan, np.float32)
    ipoints = np.zeros((H, W, 3), np.float64)
    residual = np.full((H, W), np.nan, np.float32)
    keep = ~rejected
    points[rows[keep], cols[keep]] = X[keep].astype(np.float32)
    ipoints[rows[keep], cols[keep]] = X[keep]
    residual[rows, cols] = res
    return dict(points=points, ipoints=ipoints, residual=residual, valid=out_valid, counts=(int(m.sum()), int(rejected.sum())))
