"""The mesh definition of include/sl3d.h restated in NumPy (shared by tests/test_mesh_arith.py and tests/test_gpu_mesh.py), written
from the definition alone:

  vertices   the valid pixels in row-major scan order; vid(r, c) = number of valid pixels before (r, c)
  len2(p,q)  dx = (double)p.x - (double)q.x ...; (dx*dx + dy*dy) + dz*dz in IEEE double (NumPy's ufuncs do not contract);
             short iff len2 <= (double)max_edge * (double)max_edge; NaN is not short
  cell       corners a = (r, c), b = (r, c+1), d = (r+1, c), e = (r+1, c+1)
             4 valid: diagonal a-e iff len2(a, e) <= len2(b, d): (a, d, e) then (a, e, b); else (a, d, b) then (b, d, e)
             3 valid: e missing (a, d, b); a missing (b, d, e); b missing (a, d, e); d missing (a, e, b)
  faces      the candidates with three short edges, cells in row-major order, a cell's faces in the order above
"""
import hashlib

import numpy as np

A, B, D, E = 0, 1, 2, 3
SHAPES = np.array([(A, D, E), (A, E, B), (A, D, B), (B, D, E)], dtype=np.int64)
ADE, AEB, ADB, BDE = 0, 1, 2, 3
# pixel offsets (row, col) of the corners
CORNER_RC = np.array([(0, 0), (0, 1), (1, 0), (1, 1)], dtype=np.int64)


def _len2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def np_mesh(xyz, valid, max_edge, stats=None):
    """(vertices float32 (n, 3), faces int32 (m, 3)) of one view; stats (a dict) receives counts of what occurred."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 3 and xyz.shape[2] == 3
    H, W = xyz.shape[:2]
    v = (np.asarray(valid).reshape(H, W) & 1) == 1
    vid = (np.cumsum(v.ravel()) - 1).reshape(H, W)
    verts = xyz[v]
    thr2 = np.float64(np.float32(max_edge)) * np.float64(np.float32(max_edge))
    if H < 2 or W < 2:
        if stats is not None:
            stats.update(ties=0, at_threshold=0, diag_ae=0, diag_bd=0, three=0, candidates=0, rejected=0, len2=np.zeros(0))
        return verts, np.zeros((0, 3), np.int32)
    P = xyz.astype(np.float64)
    pa, pb, pd, pe = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    va, vb, vd, ve = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    with np.errstate(invalid="ignore", over="ignore"):
        L = {"ab": _len2(pa, pb), "ad": _len2(pa, pd), "ae": _len2(pa, pe), "bd": _len2(pb, pd), "be": _len2(pb, pe), "de": _len2(pd, pe)}
        S = {k: x <= thr2 for k, x in L.items()}                          # NaN compares false
        ae_first = L["ae"] <= L["bd"]                                      # a tie takes a-e, a NaN b-d
    nvalid = va.astype(int) + vb + vd + ve
    four = nvalid == 4
    keep_of = {ADE: S["ad"] & S["de"] & S["ae"], AEB: S["ae"] & S["be"] & S["ab"], ADB: S["ad"] & S["bd"] & S["ab"], BDE: S["bd"] & S["de"] & S["be"]}
    shape = np.full((H - 1, W - 1, 2), -1, dtype=np.int64)
    shape[..., 0][four & ae_first], shape[..., 1][four & ae_first] = ADE, AEB
    shape[..., 0][four & ~ae_first], shape[..., 1][four & ~ae_first] = ADB, BDE
    three = nvalid == 3
    shape[..., 0][three & ~ve] = ADB
    shape[..., 0][three & ~va] = BDE
    shape[..., 0][three & ~vb] = ADE
    shape[..., 0][three & ~vd] = AEB
    keep = np.zeros((H - 1, W - 1, 2), dtype=bool)
    for s, k in keep_of.items():
        keep |= (shape == s) & k[..., None]
    ids = np.stack([vid[:-1, :-1], vid[:-1, 1:], vid[1:, :-1], vid[1:, 1:]], axis=-1)   # a, b, d, e
    sel = np.nonzero(keep)                                                 # C order: cells row-major, slot 0 before slot 1
    corners = SHAPES[shape[sel]]                                           # (m, 3) corner numbers
    faces = ids[sel[0][:, None], sel[1][:, None], corners].astype(np.int32)
    if stats is not None:
        cand = shape >= 0
        edges_of = {ADE: ("ad", "de", "ae"), AEB: ("ae", "be", "ab"), ADB: ("ad", "bd", "ab"), BDE: ("bd", "de", "be")}
        at, lens = 0, []
        for s, names in edges_of.items():
            m = (shape == s).any(axis=-1)
            for nme in names:
                at += int((L[nme][m] == thr2).sum())
                lens.append(L[nme][m])
        stats.update(ties=int((four & (L["ae"] == L["bd"])).sum()), at_threshold=at, diag_ae=int((four & ae_first).sum()),
                     diag_bd=int((four & ~ae_first).sum()), three=int(three.sum()), candidates=int(cand.sum()),
                     rejected=int(cand.sum() - keep.sum()), len2=np.concatenate(lens) if lens else np.zeros(0))
    return verts, faces


def faces_sha256(faces):
    return hashlib.sha256(np.ascontiguousarray(faces, dtype="<i4").tobytes()).hexdigest()


def check_faces(faces, valid, n_vertices):
    """Every face: three distinct ids in [0, n_vertices); its pixels form one of the four shapes of ONE cell; orientation -1; the cells
    are listed in row-major order."""
    faces = np.asarray(faces)
    assert faces.dtype == np.int32 and faces.ndim == 2 and faces.shape[1] == 3
    if not len(faces):
        return
    H, W = valid.shape
    assert faces.min() >= 0 and faces.max() < n_vertices
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    pix = np.flatnonzero((valid.ravel() & 1) == 1)
    assert len(pix) == n_vertices
    r, c = pix[faces] // W, pix[faces] % W                                # (m, 3)
    r0, c0 = r.min(axis=1), c.min(axis=1)
    rel = np.stack([r - r0[:, None], c - c0[:, None]], axis=-1)           # (m, 3, 2)
    assert rel.max() <= 1
    want = CORNER_RC[SHAPES]                                               # (4, 3, 2)
    assert (rel[:, None] == want[None]).all(axis=(2, 3)).any(axis=1).all()
    e1c, e1r = c[:, 1] - c[:, 0], r[:, 1] - r[:, 0]
    e2c, e2r = c[:, 2] - c[:, 1], r[:, 2] - r[:, 1]
    assert (e1c * e2r - e1r * e2c == -1).all()
    cell = r0 * W + c0
    assert (np.diff(cell) >= 0).all()
