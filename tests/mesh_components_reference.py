"""The component definition of include/sl3d.h restated in NumPy (shared by tests/test_mesh_components_arith.py and
tests/test_gpu_mesh_components.py), written from the definition alone, over the faces of mesh_reference.np_mesh:

  component     two vertices are connected iff they share a face; the transitive closure.  A vertex in no face: a component of size 1
  label         the smallest vertex id of the component, int32, in vertex-id order
  filtered      vertices whose component has >= min_vertices vertices, in order, renumbered; the original faces among them, in order,
                with the new ids; ids[i] = original id of new vertex i
"""
import hashlib

import numpy as np


def np_labels(n_vertices, faces):
    """int32 (n_vertices,): every face gives the edges (v0, v1), (v1, v2).  A round: over every edge whose ends still carry different
    labels the larger label -- a vertex of that component -- takes the minimum of itself and the smaller one (np.minimum.at), then
    pointers are jumped (lab = lab[lab]) until every vertex points at a fixed point.  Rounds until no edge is left: a round at least
    halves the number of labels in use per component, O(log n) rounds."""
    lab = np.arange(n_vertices, dtype=np.int64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    s, d = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    while True:
        ls, ld = lab[s], lab[d]
        active = ls != ld
        if not active.any():
            break
        s, d, ls, ld = s[active], d[active], ls[active], ld[active]
        np.minimum.at(lab, np.maximum(ls, ld), np.minimum(ls, ld))
        while True:
            jumped = lab[lab]
            if np.array_equal(jumped, lab):
                break
            lab = jumped
    return lab.astype(np.int32)


def component_sizes(labels):
    """(roots ascending, their sizes)"""
    roots, sizes = np.unique(labels, return_counts=True)
    return roots, sizes


def np_filtered(verts, faces, min_vertices):
    """(verts', faces' int32, ids int32) of the definition"""
    n = len(verts)
    lab = np_labels(n, faces)
    size = np.bincount(lab, minlength=n)
    keep = size[lab] >= min_vertices
    ids = np.flatnonzero(keep).astype(np.int32)
    new_id = np.cumsum(keep) - 1
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fk = keep[f].all(axis=1) if len(f) else np.zeros(0, bool)
    assert np.array_equal(fk, keep[f].any(axis=1) if len(f) else fk)      # a face's vertices share a component
    return np.asarray(verts)[keep], new_id[f[fk]].astype(np.int32).reshape(-1, 3), ids


def labels_sha256(labels):
    return hashlib.sha256(np.ascontiguousarray(labels, dtype="<i4").tobytes()).hexdigest()


def serpentine(H, W, corridor, gap, vertical=False):
    """0/1 mask (H, W): corridors `corridor` pixels high separated by `gap` unselected rows, joined alternately at the right and left
    ends -- one snake the minimum label has to travel from end to end.  vertical: the same along the columns."""
    if vertical:
        return np.ascontiguousarray(serpentine(W, H, corridor, gap).T)
    m = np.zeros((H, W), np.uint8)
    period = corridor + gap
    for i, r0 in enumerate(range(0, H - corridor + 1, period)):
        m[r0:r0 + corridor] = 1
        if r0 + period + corridor <= H:                      # a further corridor follows: the joint
            c = slice(W - corridor, W) if i % 2 == 0 else slice(0, corridor)
            m[r0 + corridor:r0 + period, c] = 1
    return m
