"""A synthetic capture whose scan reproduces the reference's own point cloud (tests/golden/ply_stage7.npz).

Plain module (not a conftest): imported by tests/test_oracle.py, tests/test_gpu_reference_cloud.py and
tests/golden/make_golden.py, which wrote the fixture.

The reference's configuration: camera 1600x1200, projector 1280x720, fringe width 32, 6 / 5 Gray planes, 3 fringes
(global_cv.h:49-53, common_variables.h:6-9,23-24).  Every pixel's planes are one row of a per-coordinate byte table:
row x of `table_x` is the (fringe triple, Gray planes, inverse Gray planes) on which stages 3-5 decode projector column x,
row y of `table_y` the same for projector row y.  make_golden.py proved every row with the oracle.

  * mask: every pixel but the one-pixel frame border is selected, so stage 3's boundary removal only clears the ring next to the
    border, where no vertex lies;
  * vertex pixels (c, r) of the fixture's tuples decode to their (x, y) (a vertex no tuple reproduces has the tuple -1 and is
    not part of the capture);
  * every other pixel is a FILLER that stays selected but decodes out of range: on even rows the x filler (Gray code 63,
    x >= 2016 > PW - 1), on odd rows the y filler (Gray code 31, y >= 992 > PH - 1), so that both sides of C2's range test
    (5/compute_correspondance.cpp:671) reject about 1.9 M pixels with codes >= n_codes.
"""
import os

import numpy as np

W, H, PW, PH = 1600, 1200, 1280, 720
N_V, N_H, FW, NCODES_V, NCODES_H, F = 6, 5, 32, 40, 23, 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ply_stage7.npz")
X_FILLER, Y_FILLER = PW, PH          # the filler rows of table_x / table_y


def predict_points(tup, Ac, Ap, cal):
    """A compression model of the PLY's floats, not a reference: T1-T3 on the tuples [n, 4] (camera col c, row r, projector x, y)
    with only element-wise IEEE operations (cvUndistortPoints' 5 fixed-point iterations, the normal equations summed in a fixed
    order, Cramer's rule), so that the float32 result is the same bits on every machine.  Ac, Ap: the fixture's 3x4 K [R|t]."""
    f64 = np.float64

    def undist(u, v, K, d):
        K = [float(k) for k in np.ravel(K)]
        k1, k2, p1, p2, k3 = [float(k) for k in d]
        x0 = (u - K[2]) / K[0]
        y0 = (v - K[5]) / K[4]
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            x, y = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * ic, (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * ic
        hw = K[6] * x + K[7] * y + K[8]
        return (K[0] * x + K[1] * y + K[2]) / hw, (K[3] * x + K[4] * y + K[5]) / hw

    uc, vc = undist(tup[:, 0].astype(f64), tup[:, 1].astype(f64), cal["Kc"], cal["dc"])
    up, vp = undist(tup[:, 2].astype(f64), tup[:, 3].astype(f64), cal["Kp"], cal["dp"])
    rows = [(Ac, uc, 0), (Ac, vc, 1), (Ap, up, 0), (Ap, vp, 1)]
    P = [[A[i, q] - u * A[2, q] for q in range(3)] for A, u, i in rows]
    Fv = [A[2, 3] * u - A[i, 3] for A, u, i in rows]
    M = [[P[0][i] * P[0][j] + P[1][i] * P[1][j] + P[2][i] * P[2][j] + P[3][i] * P[3][j] for j in range(3)] for i in range(3)]
    b = [P[0][i] * Fv[0] + P[1][i] * Fv[1] + P[2][i] * Fv[2] + P[3][i] * Fv[3] for i in range(3)]

    def det(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))

    d = det(M)
    out = []
    for k in range(3):
        Mk = [[b[i] if j == k else M[i][j] for j in range(3)] for i in range(3)]
        out.append(det(Mk) / d)
    return np.stack(out, -1).astype(np.float32)


def _ordered(v):
    i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _from_ordered(o):
    o = np.asarray(o, dtype=np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(np.float32)


def encode_fixture(tuples, xyz, cal, Ac, Ap):
    """The stored form of tuples [n, 4] (-1 rows: vertices no tuple reproduces) and the PLY's float32 xyz [n, 3]: tuple deltas in
    file order, and each point as its ulp residual from predict_points (0 or +-1), the unmatched points verbatim, and the SHA-256
    of the xyz bytes, which load_fixture checks -- the decoded floats ARE the PLY's, bit for bit."""
    import hashlib
    tuples = np.asarray(tuples, dtype=np.int64)
    m = tuples[:, 0] >= 0
    res = np.zeros(xyz.shape, dtype=np.int64)
    res[m] = _ordered(xyz[m]) - _ordered(predict_points(tuples[m], Ac, Ap, cal))
    assert np.abs(res).max() <= 127
    enc = {"tuples_delta": np.diff(tuples, axis=0, prepend=0).astype(np.int16), "xyz_residual": res.astype(np.int8),
           "unmatched_xyz": xyz[~m], "A_cam": Ac, "A_proj": Ap,
           "xyz_sha256": np.array(hashlib.sha256(np.ascontiguousarray(xyz, dtype="<f4").tobytes()).hexdigest())}
    assert np.array_equal(np.cumsum(enc["tuples_delta"].astype(np.int64), axis=0), tuples)
    return enc


def load_fixture(path=FIXTURE, cal=None):
    """The fixture with `tuples` [n, 4] int64 and the PLY's `xyz` [n, 3] float32 decoded (see encode_fixture); cal: the calibration
    dict (default: tests/golden/calibration.json)."""
    import hashlib
    import json
    fx = dict(np.load(path))
    if cal is None:
        with open(os.path.join(os.path.dirname(path), "calibration.json")) as f:
            cal = json.load(f)
    tup = np.cumsum(fx["tuples_delta"].astype(np.int64), axis=0)
    m = tup[:, 0] >= 0
    xyz = np.empty(tup[:, :3].shape, dtype=np.float32)
    xyz[m] = _from_ordered(_ordered(predict_points(tup[m], fx["A_cam"], fx["A_proj"], cal)) + fx["xyz_residual"][m].astype(np.int64))
    xyz[~m] = fx["unmatched_xyz"]
    if hashlib.sha256(xyz.astype("<f4").tobytes()).hexdigest() != str(fx["xyz_sha256"]):
        raise ValueError(f"{path}: the decoded points are not the PLY's (SHA-256 of the xyz bytes differs)")
    fx["tuples"], fx["xyz"] = tup, xyz
    return fx


def capture(fx):
    """fx: the fixture (load_fixture()).  -> (mask [H,W] u8, planes_v [F+2N_v,H,W] u8, planes_h [F+2N_h,H,W] u8)."""
    tup = matched_tuples(fx)
    ix = np.empty((H, W), dtype=np.int64)
    iy = np.empty((H, W), dtype=np.int64)
    ix[0::2], iy[0::2] = X_FILLER, 0                  # even rows: x out of range
    ix[1::2], iy[1::2] = 0, Y_FILLER                  # odd rows: y out of range
    ix[tup[:, 1], tup[:, 0]] = tup[:, 2]
    iy[tup[:, 1], tup[:, 0]] = tup[:, 3]
    planes_v = np.ascontiguousarray(np.moveaxis(fx["table_x"][ix], -1, 0))
    planes_h = np.ascontiguousarray(np.moveaxis(fx["table_y"][iy], -1, 0))
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[1:-1, 1:-1] = 1
    return mask, planes_v, planes_h


def matched_tuples(fx):
    """[m, 4] int64 (camera col c, row r, projector x, y) of the vertices a tuple reproduces, in file order (= scan order)."""
    t = fx["tuples"].astype(np.int64)
    return t[t[:, 0] >= 0]


def matched_xyz(fx):
    """The PLY's float32 points of those vertices, in file order: what the scan of capture(fx) must produce."""
    return fx["xyz"][fx["tuples"][:, 0] >= 0]


def vertex_map(fx):
    """[H,W] bool: the pixels that carry a vertex (the valid map stage 5 must leave)."""
    t = matched_tuples(fx)
    v = np.zeros((H, W), dtype=bool)
    v[t[:, 1], t[:, 0]] = True
    return v
