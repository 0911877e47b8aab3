"""The hole-filling definition of include/sl3d.h restated in NumPy (shared by tests/test_mesh_holes_arith.py and
tests/test_gpu_mesh_holes.py), written from the definition alone:

  hole        a 4-connected component of non-candidate pixels of the window without a pixel of row 0, row H-1, column 0 or column W-1 and
              with at most max_hole pixels -- found by a flood fill, pixel by pixel
  rim         L, R, U, D: the nearest candidates to the left, right, above and below of a hole pixel, dl / dr / du / dd pixels away
  usable      the row interpolant iff len2(L, R) <= ((double)fill_edge (dl + dr))^2 (NaN: not usable); the column interpolant likewise
  position    h = (dr L + dl R) / (dl + dr), v = (dd U + du D) / (du + dd) in double; both usable:
              ((du + dd) h + (dl + dr) v) / ((dl + dr) + (du + dd)); one cast to float32

The mesh, the normals and the ids follow with np_mesh / np_normals over the filled grid, fill_mesh below.
"""
import numpy as np

from mesh_normals_reference import np_normals
from mesh_reference import np_mesh

NORMALS = 1


def np_holes(candidates, max_hole):
    """(hole bool (H, W): the pixels of the qualifying components, number of qualifying components).  A flood fill over the
    4-neighbourhood from every non-candidate pixel not seen yet, in scan order."""
    cand = (np.asarray(candidates) & 1) == 1
    H, W = cand.shape
    seen = cand.copy()
    hole = np.zeros((H, W), bool)
    n = 0
    for r0, c0 in zip(*np.nonzero(~cand)):
        if seen[r0, c0]:
            continue
        seen[r0, c0] = True
        stack, comp, border = [(int(r0), int(c0))], [], False
        while stack:
            r, c = stack.pop()
            comp.append((r, c))
            border |= r == 0 or r == H - 1 or c == 0 or c == W - 1
            for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                if 0 <= rr < H and 0 <= cc < W and not seen[rr, cc]:
                    seen[rr, cc] = True
                    stack.append((rr, cc))
        if not border and len(comp) <= max_hole:
            n += 1
            for r, c in comp:
                hole[r, c] = True
    return hole, n


def _len2(p, q):
    with np.errstate(invalid="ignore", over="ignore"):
        d = p.astype(np.float64) - q.astype(np.float64)
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def np_fill(xyz, candidates, max_hole, fill_edge, stats=None):
    """(filled xyz float32 (H, W, 3), filled valid uint8 (H, W), filled bool (H, W)); stats (a dict) receives holes, hole_pixels, both,
    only_h, only_v, none."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 3 and xyz.shape[2] == 3
    cand = (np.asarray(candidates).reshape(xyz.shape[:2]) & 1) == 1
    hole, n_holes = np_holes(cand, max_hole)
    out = np.where(cand[..., None], xyz, np.float32(0.0))
    filled = np.zeros(cand.shape, bool)
    fe = np.float64(np.float32(fill_edge))
    kinds = {3: 0, 1: 0, 2: 0, 0: 0}
    with np.errstate(invalid="ignore", over="ignore"):
        for r, c in zip(*np.nonzero(hole)):
            dl = dr = du = dd = 1
            while not cand[r, c - dl]:
                dl += 1
            while not cand[r, c + dr]:
                dr += 1
            while not cand[r - du, c]:
                du += 1
            while not cand[r + dd, c]:
                dd += 1
            L, R, U, D = xyz[r, c - dl], xyz[r, c + dr], xyz[r - du, c], xyz[r + dd, c]
            th, tv = fe * np.float64(dl + dr), fe * np.float64(du + dd)
            use_h, use_v = bool(_len2(L, R) <= th * th), bool(_len2(U, D) <= tv * tv)          # NaN compares false
            h = (np.float64(dr) * L.astype(np.float64) + np.float64(dl) * R.astype(np.float64)) / np.float64(dl + dr)
            v = (np.float64(dd) * U.astype(np.float64) + np.float64(du) * D.astype(np.float64)) / np.float64(du + dd)
            kinds[int(use_h) | int(use_v) << 1] += 1
            if use_h and use_v:
                p = (np.float64(du + dd) * h + np.float64(dl + dr) * v) / np.float64((dl + dr) + (du + dd))
            elif use_h:
                p = h
            elif use_v:
                p = v
            else:
                continue
            out[r, c] = p.astype(np.float32)
            filled[r, c] = True
    if stats is not None:
        stats.update(holes=n_holes, hole_pixels=int(hole.sum()), both=kinds[3], only_h=kinds[1], only_v=kinds[2], none=kinds[0])
    return out, (cand | filled).astype(np.uint8), filled


def fill_mesh(xyz, valid, candidates, max_edge, max_hole, fill_edge, flags=0, stats=None):
    """(vertices, faces, vertex_ids, normals or None) of one view: np_fill, then np_mesh / np_normals over the filled grid; vertex_ids:
    a candidate's id in the scan order of `valid` (the view's compacted cloud), -1 for a filled vertex."""
    fxyz, fvalid, filled = np_fill(xyz, candidates, max_hole, fill_edge, stats)
    verts, faces = np_mesh(fxyz, fvalid, max_edge)
    v = (np.asarray(valid).reshape(fvalid.shape) & 1) == 1
    vid = (np.cumsum(v.ravel()) - 1).reshape(v.shape)
    ids = np.where(filled, -1, vid)[fvalid == 1].astype(np.int32)
    return verts, faces, ids, (np_normals(verts, faces) if flags & NORMALS else None)


def filtered_candidates(xyz, valid, max_edge, min_vertices):
    """the candidate map of min_vertices > 1: the pixels whose vertex np_filtered keeps, from np_mesh over the view"""
    from mesh_components_reference import np_filtered
    valid = np.asarray(valid)
    if min_vertices <= 1:
        return (valid & 1).astype(np.uint8)
    verts, faces = np_mesh(xyz, valid, max_edge)
    _, _, ids = np_filtered(verts, faces, min_vertices)
    cand = np.zeros(valid.size, np.uint8)
    cand[np.flatnonzero(valid.ravel() == 1)[ids]] = 1
    return cand.reshape(valid.shape)
