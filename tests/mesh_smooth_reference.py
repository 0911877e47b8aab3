"""The smoothing definition of include/sl3d.h (sl3d_mesh_smooth) restated in NumPy on (vertices, faces) alone (shared by
tests/test_mesh_smooth_arith.py and tests/test_gpu_mesh_smooth.py), written from the definition:

  neighbours  two vertices are neighbours iff some face contains both; a vertex's neighbours sorted by id (at most 8)
  boundary    an edge is a boundary edge iff exactly one face contains it (none lies in more than two); a boundary vertex is an endpoint
              of one
  one step    factor f = the float32 argument widened to double; a vertex with k >= 1 neighbours that is not fixed, per component:
              s = +0, then s += (double)neighbour over the neighbour slots 0..7 in sequence; m = s / (double)k;
              p' = (float32)((double)p + f * (m - (double)p)) -- NumPy's ufuncs do not contract; k = 0 or fixed: p' = p bitwise.
              Every vertex reads the positions of the step before
  iterations  one step with lambda, then one with mu if mu != 0
  flags       1: boundary vertices are fixed; 2: normals = np_normals(smoothed, faces) (tests/mesh_normals_reference.py)
"""
import hashlib

import numpy as np

FIX_BOUNDARY, NORMALS = 1, 2


def np_topology(n_vertices, faces):
    """(slots int64 (n, 8): the neighbours of every vertex in ascending id, -1 beyond its degree; boundary bool (n,); stats: a dict with
    the edges, the boundary edges and the largest number of faces on an edge)."""
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    slots = np.full((n_vertices, 8), -1, np.int64)
    boundary = np.zeros(n_vertices, bool)
    if not len(faces):
        return slots, boundary, dict(edges=0, boundary_edges=0, max_faces_per_edge=0)
    pairs = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    assert (lo != hi).all()
    edges, per_edge = np.unique(np.stack([lo, hi], axis=1), axis=0, return_counts=True)
    assert per_edge.max() <= 2                                             # no edge lies in more than two faces
    boundary[edges[per_edge == 1].ravel()] = True
    # both directions of every edge, sorted by vertex, then by neighbour: a vertex's neighbours in ascending id
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rank = np.arange(len(src)) - np.searchsorted(src, src, side="left")
    assert rank.max() <= 7
    slots[src, rank] = dst
    return slots, boundary, dict(edges=len(edges), boundary_edges=int((per_edge == 1).sum()), max_faces_per_edge=int(per_edge.max()))


def np_step(verts, slots, moving, factor):
    """one step: verts float32 (n, 3) -> float32 (n, 3); moving: the vertices that are not fixed (those without a neighbour stay anyway)"""
    assert verts.dtype == np.float32
    f = np.float64(np.float32(factor))
    P = verts.astype(np.float64)
    k = (slots >= 0).sum(axis=1)
    s = np.zeros_like(P)
    with np.errstate(all="ignore"):
        for j in range(8):                                                  # in sequence over the slots: ascending neighbour id
            sel = slots[:, j] >= 0
            s[sel] = s[sel] + P[slots[sel, j]]
        go = moving & (k > 0)
        m = s[go] / k[go].astype(np.float64)[:, None]
        out = verts.copy()
        out[go] = (P[go] + f * (m - P[go])).astype(np.float32)
    return out


def np_smooth(verts, faces, iterations, lam, mu, flags=0, stats=None):
    """The smoothed vertices (float32 (n, 3)) of the mesh (verts float32 (n, 3), faces int (m, 3)); with flags & NORMALS the pair
    (vertices, normals).  stats (a dict) receives degree (n,), boundary (n,), moving (n,) and np_topology's counts."""
    from mesh_normals_reference import np_normals
    verts = np.ascontiguousarray(verts)
    assert verts.dtype == np.float32 and verts.ndim == 2 and verts.shape[1] == 3 and iterations >= 1
    slots, boundary, st = np_topology(len(verts), faces)
    moving = ~boundary if flags & FIX_BOUNDARY else np.ones(len(verts), bool)
    if stats is not None:
        degree = (slots >= 0).sum(axis=1)
        stats.update(st, degree=degree, boundary=boundary, moving=moving & (degree > 0))
    cur = verts
    for _ in range(iterations):
        cur = np_step(cur, slots, moving, lam)
        if np.float32(mu) != 0:
            cur = np_step(cur, slots, moving, mu)
    return (cur, np_normals(cur, faces)) if flags & NORMALS else cur


def positions_sha256(xyz):
    return hashlib.sha256(np.ascontiguousarray(xyz, dtype="<f4").tobytes()).hexdigest()
