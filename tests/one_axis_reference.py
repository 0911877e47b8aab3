"""The one-axis scan of SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL (include/sl3d.h) restated in NumPy, float64,
written from the comment above the flags alone (shared by tests/test_one_axis_arith.py and tests/test_gpu_one_axis.py).  a is the coded
axis (0: the projector column, 1: the row), b the other one.  Per pixel, from the planes stage 4 leaves for axis a:

  3. ok = rint(fw_a * (unw_a / P2)) in [0, extent_a - 1] (NaN and infinities fail);  valid = sel && ok with sel the valid byte of axis a;
     c_p_map[a] = the integer, c_p_map[b] = -1 where valid, both 0 elsewhere
  4. s = fw_a * (unw_a / P2), or the anchored coordinate (tests/anchor_reference.py) where that rule applies
  5. t = f * ((s - c) * (1.0 / f)) + c                f, c = Kp[0], Kp[2] (a = 0) or Kp[4], Kp[5] (a = 1)
  6. r0 = Ac[0][:3] - u Ac[2][:3], f0 = Ac[2][3] u - Ac[0][3];  r1, f1 with v and row 1;  r2 = Ap[a][:3] - t Ap[2][:3], f2 = Ap[2][3] t - Ap[a][3]
     c0 = r1 x r2, c1 = r2 x r0, c2 = r0 x r1;  det = r0 . c0;  X = (f0 c0 + f1 c1 + f2 c2) * (1.0 / det), 0 where det == 0
  7. points = (float)X where valid, NaN elsewhere; intersection_points = X where valid, 0 elsewhere

NumPy evaluates each operation as one IEEE double operation; the definition fuses some multiply-adds (fma), so points agree to the
project's 1e-5 bar, not bit for bit.  Validity, c_p_map and the coordinates have no fused step: they are exact."""
import numpy as np

import anchor_reference as AR
import subpixel_reference as SR

P2 = (2.0 * 22.0) / 7.0


def correspond(unw, fw, extent):
    """(ok, integer as float64) of stage 5's test on one absolute-phase plane (float32)."""
    assert unw.dtype == np.float32
    with np.errstate(invalid="ignore"):
        r = np.rint(np.float64(fw) * (unw.astype(np.float64) / P2))
        ok = (r >= 0.0) & (r <= np.float64(extent - 1))
    return ok, r


def stage5(unw, sel, fw, extent, axis):
    """(valid uint8, c_p_map int64 (H, W, 2)) of the one-axis stage 5."""
    ok, r = correspond(unw, fw, extent)
    valid = (sel == 1) & ok
    cp = np.zeros(unw.shape + (2,), np.int64)
    cp[..., axis] = np.where(valid, np.where(ok, r, 0.0), 0.0).astype(np.int64)
    cp[..., 1 - axis] = np.where(valid, -1, 0)
    return valid.astype(np.uint8), cp


def coordinate(w, code, unw, fw, n_fringe, n_gray, axis, origin, full, anchored):
    """s of step 4 on every pixel (float64)."""
    plain = np.float64(fw) * (unw.astype(np.float64) / P2)
    if not anchored:
        return plain
    where = AR.applies(axis, unw.shape, origin, full, n_gray)
    with np.errstate(invalid="ignore", over="ignore"):
        anch = AR.coordinate(w, code.astype(np.int64), fw, n_fringe)
    return np.where(where, anch, plain)


def correspondences(s, sel, axis):
    """(H, W, 2) of sl3d_get_correspondences_subpixel: s in component a, NaN in component b, both NaN where the valid byte of axis a is not 1."""
    xy = np.full(s.shape + (2,), np.nan)
    xy[..., axis] = np.where(sel == 1, s, np.nan)
    return xy


def project(s, Kp, axis):
    K = np.asarray(Kp, np.float64).reshape(3, 3)
    f, c = (K[0, 0], K[0, 2]) if axis == 0 else (K[1, 1], K[1, 2])
    return f * ((s - c) * (1.0 / f)) + c


def rows(A_cam, A_proj, axis, u, v, t):
    """(P (n, 3, 3), F (n, 3)) of step 6."""
    Ac, Ap = np.asarray(A_cam, np.float64).reshape(3, 4), np.asarray(A_proj, np.float64).reshape(3, 4)
    spec = [(Ac, 0, u), (Ac, 1, v), (Ap, axis, t)]
    P = np.stack([np.stack([A[r, j] - x * A[2, j] for j in range(3)], axis=-1) for A, r, x in spec], axis=-2)
    F = np.stack([A[2, 3] * x - A[r, 3] for A, r, x in spec], axis=-1)
    return P, F


def solve(A_cam, A_proj, axis, u, v, t):
    """X (n, 3): adj(P) F / det(P), zero where the determinant is zero."""
    P, F = rows(A_cam, A_proj, axis, u, v, t)
    r0, r1, r2 = P[:, 0], P[:, 1], P[:, 2]
    cross = lambda p, q: np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=-1)
    c0, c1, c2 = cross(r1, r2), cross(r2, r0), cross(r0, r1)
    det = r0[:, 0] * c0[:, 0] + (r0[:, 1] * c0[:, 1] + r0[:, 2] * c0[:, 2])
    with np.errstate(divide="ignore"):
        rdet = np.where(det != 0.0, 1.0 / np.where(det != 0.0, det, 1.0), 0.0)
    n = F[:, 0:1] * c0 + (F[:, 1:2] * c1 + F[:, 2:3] * c2)
    return n * rdet[:, None], det


def scan(w, code, unw, sel, cal, A_cam, A_proj, axis, fw, extent, n_gray, n_fringe=3, origin=(0, 0), full=None, anchored=False):
    """Steps 3-7 over one view from the planes of axis a before stage 5 (w float32, code int, unw float32, sel uint8).  Returns dict(valid,
    c_p_map, xy (the correspondences), s, points float32, ipoints float64, det (H, W; NaN where not valid))."""
    Kc, dc, _, _, Kp, _, _, _ = cal
    H, W = unw.shape
    full = (W, H) if full is None else full
    valid, cp = stage5(unw, sel, fw, extent, axis)
    s = coordinate(w, code, unw, fw, n_fringe, n_gray, axis, origin, full, anchored)
    m = valid == 1
    rws, cols = np.nonzero(m)
    u, v = SR.undistort_reproject(cols.astype(np.float64) + origin[0], rws.astype(np.float64) + origin[1], Kc, dc)
    X, det = solve(A_cam, A_proj, axis, u, v, project(s[m], Kp, axis))
    points = np.full((H, W, 3), np.nan, np.float32)
    ipoints = np.zeros((H, W, 3), np.float64)
    dets = np.full((H, W), np.nan)
    points[rws, cols] = X.astype(np.float32)
    ipoints[rws, cols] = X
    dets[rws, cols] = det
    return dict(valid=valid, c_p_map=cp, xy=correspondences(s, sel, axis), s=s, points=points, ipoints=ipoints, det=dets)
