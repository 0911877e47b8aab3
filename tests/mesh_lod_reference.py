"""The level-of-detail definition of include/sl3d.h restated in NumPy (shared by tests/test_mesh_lod_arith.py and
tests/test_gpu_mesh_lod.py), written from the definition alone:

  blocks          H' = ceil(H / step), W' = ceil(W / step); block (R, C) = rows [R step, min(R step + step, H)) x the same of the columns
  representative  the candidate with the smallest d = (2(r - R step) + 1 - step)^2 + (2(c - C step) + 1 - step)^2, the first in row-major
                  scan order among equals; no candidate: an invalid coarse pixel
  position        the representative's bits; with the mean: members = the representative and every other candidate q with
                  len2(q, rep) <= (double)lod_edge^2 (NaN: not a member), k of them; k == 1: the representative's bits, else per
                  component s = +0, s += (double)q in scan order, (float)(s / (double)k)

The mesh, the normals and the ids of a level of detail follow with np_mesh / np_normals on what np_lod returns, lod_mesh below.
"""
import numpy as np

from mesh_normals_reference import np_normals
from mesh_reference import np_mesh

MEAN, NORMALS = 1, 2


def np_lod(xyz, candidates, step, lod_edge, mean, stats=None):
    """(coarse xyz float32 (H', W', 3), coarse valid uint8 (H', W'), rep int64 (H', W'): the representative's pixel r * W + c, -1 where
    the coarse pixel is invalid); stats (a dict) receives: ties (blocks whose smallest d more than one candidate has), excluded
    (candidates that are no members; 0 without the mean), clipped (occupied blocks the window clips), k_gt_1 / k_eq_1 (occupied blocks by their
    number of members; without the mean every block counts as k == 1), at_threshold (len2 == lod_edge^2 exactly), nan_len2."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 3 and xyz.shape[2] == 3 and 1 <= step <= 16
    H, W = xyz.shape[:2]
    Hc, Wc = -(-H // step), -(-W // step)
    n = step * step
    cand = np.zeros((Hc * step, Wc * step), bool)
    cand[:H, :W] = (np.asarray(candidates).reshape(H, W) & 1) == 1
    pts = np.zeros((Hc * step, Wc * step, 3), np.float32)
    pts[:H, :W] = xyz
    pix = np.full((Hc * step, Wc * step), -1, np.int64)
    pix[:H, :W] = np.arange(H * W).reshape(H, W)

    def blocks(a):                                                         # (H', W', step * step, ...) in the block's scan order
        tail = a.shape[2:]
        return a.reshape(Hc, step, Wc, step, *tail).swapaxes(1, 2).reshape(Hc, Wc, n, *tail)

    bc, bp, bpix = blocks(cand), blocks(pts), blocks(pix)
    dr, dc = np.divmod(np.arange(n), step)
    d = (2 * dr + 1 - step) ** 2 + (2 * dc + 1 - step) ** 2
    big = np.iinfo(np.int64).max
    dist = np.where(bc, d[None, None, :], big)
    best = dist.min(axis=2)
    valid = best < big
    at = np.argmax(dist == best[..., None], axis=2)                       # the first in scan order among equals
    at = np.where(valid, at, 0)
    take = at[..., None]
    rep_pts = np.take_along_axis(bp, take[..., None], axis=2)[:, :, 0]     # (H', W', 3) float32: copies, bit for bit
    rep = np.where(valid, np.take_along_axis(bpix, take, axis=2)[..., 0], -1)
    out = rep_pts.copy()
    thr2 = np.float64(np.float32(lod_edge)) * np.float64(np.float32(lod_edge))
    is_rep = (np.arange(n)[None, None, :] == take) & valid[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        df = bp.astype(np.float64) - rep_pts.astype(np.float64)[:, :, None, :]
        len2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
        others = bc & ~is_rep & valid[..., None]
        member = is_rep | (others & (len2 <= thr2))                        # NaN compares false
        k = member.sum(axis=2)
        if mean:
            s = np.zeros((Hc, Wc, 3), np.float64)
            for j in range(n):                                             # the ordered sum: one add after the other
                s = np.where(member[:, :, j, None], s + bp[:, :, j].astype(np.float64), s)
            m = (s / np.maximum(k, 1)[..., None].astype(np.float64)).astype(np.float32)
            out = np.where((k > 1)[..., None], m, out)
    out[~valid] = 0.0
    if stats is not None:
        clipped = np.zeros((Hc, Wc), bool)
        if H % step:
            clipped[-1, :] = True
        if W % step:
            clipped[:, -1] = True
        stats.update(ties=int((valid & (((dist == best[..., None]) & bc).sum(axis=2) > 1)).sum()),
                     excluded=int((others & ~member).sum()) if mean else 0, clipped=int((clipped & valid).sum()),
                     k_gt_1=int((valid & (k > 1)).sum()) if mean else 0, k_eq_1=int((valid & (k == 1)).sum()) if mean else int(valid.sum()),
                     at_threshold=int((others & (len2 == thr2)).sum()), nan_len2=int((others & np.isnan(len2)).sum()),
                     occupied=int(valid.sum()))
    return out, valid.astype(np.uint8), rep


def lod_mesh(xyz, valid, candidates, step, lod_edge, flags, stats=None):
    """(vertices, faces, vertex_ids, normals or None) of one view: np_lod, then np_mesh / np_normals over the coarse grid; vertex_ids:
    the representatives' ids in the scan order of `valid` (the view's compacted cloud)."""
    cxyz, cvalid, rep = np_lod(xyz, candidates, step, lod_edge, bool(flags & MEAN), stats)
    cell_stats = {} if stats is not None else None
    verts, faces = np_mesh(cxyz, cvalid, lod_edge, cell_stats)
    if stats is not None:
        stats["cells"] = cell_stats
    v = (np.asarray(valid).ravel() & 1) == 1
    vid = np.cumsum(v) - 1
    reps = rep[cvalid == 1]
    assert v[reps].all()
    ids = vid[reps].astype(np.int32)
    return verts, faces, ids, (np_normals(verts, faces) if flags & NORMALS else None)
