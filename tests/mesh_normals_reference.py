"""The vertex-normal definition of include/sl3d.h restated in NumPy (shared by tests/test_mesh_normals_arith.py and
tests/test_gpu_mesh_normals.py), written from the definition alone:

  face vector  face (i, j, k) in the order the face list gives its ids, points p, q, s widened to double: u = q - p, v = s - p,
               fn = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x) -- NumPy's ufuncs do not contract
  vertex sum   acc = +0, then acc += fn for every face that contains the vertex, in face-list order (at most 8 faces)
  normal       ss = (acc.x*acc.x + acc.y*acc.y) + acc.z*acc.z; 0 < ss < +inf: (float32)(acc / sqrt(ss)), else +0
"""
import hashlib

import numpy as np


def np_normals(verts, faces, stats=None):
    """(n, 3) float32 normals of the mesh (verts float32 (n, 3), faces int (m, 3)); stats (a dict) receives max_faces_per_vertex and
    faces_per_vertex."""
    verts, faces = np.asarray(verts), np.asarray(faces)
    assert verts.dtype == np.float32 and verts.ndim == 2 and verts.shape[1] == 3
    assert faces.ndim == 2 and faces.shape[1] == 3
    n, m = len(verts), len(faces)
    P = verts.astype(np.float64)
    acc = np.zeros((n, 3), np.float64)
    with np.errstate(all="ignore"):
        p, q, s = P[faces[:, 0]], P[faces[:, 1]], P[faces[:, 2]]
        u, v = q - p, s - p
        fn = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=-1)
        # (vertex, face index) pairs, sorted by vertex, then by face index: a vertex's faces in face-list order
        vert = faces.astype(np.int64).ravel()
        face = np.repeat(np.arange(m, dtype=np.int64), 3)
        order = np.lexsort((face, vert))
        vert, face = vert[order], face[order]
        first = np.searchsorted(vert, vert, side="left")
        rank = np.arange(len(vert)) - first
        passes = int(rank.max()) + 1 if len(rank) else 0
        assert passes <= 8
        for k in range(passes):                       # sequential by rank: every vertex occurs at most once per pass
            sel = rank == k
            acc[vert[sel]] = acc[vert[sel]] + fn[face[sel]]
        ss = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
        ok = (ss > 0.0) & (ss < np.inf)
        out = np.zeros((n, 3), np.float32)
        out[ok] = (acc[ok] / np.sqrt(ss[ok])[:, None]).astype(np.float32)
    if stats is not None:
        stats.update(max_faces_per_vertex=passes, faces_per_vertex=np.bincount(vert, minlength=n))
    return out


def normals_sha256(normals):
    return hashlib.sha256(np.ascontiguousarray(normals, dtype="<f4").tobytes()).hexdigest()
