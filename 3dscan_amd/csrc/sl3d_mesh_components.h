// sl3d_mesh_components.h -- the connectivity of the mesh stage (sl3d_mesh_components / sl3d_mesh_views_filtered): the union-find
// that turns what the cells connect into labels, and which faces a filter keeps.  Shared by the kernels of sl3d_mesh_components.hip and by the CPU check the test
// suite runs over whole frames (tests/native/mesh_components_check.cpp): plain C, no HIP types.  The definition (include/sl3d.h):
//
//   two vertices are connected iff they share a face of the mesh sl3d_mesh_views defines; components: the transitive closure
//   label of a vertex = the smallest vertex id of its component; vertex ids follow the pixels' scan order, so the smallest PIXEL index
//   (r * pitch + c) of a component names the same vertex: the union-find runs on pixel indices, ids appear only on the way out
//
// What a cell connects comes from the cell plane (cc_cell_code / cc_code_corners, sl3d_mesh.h).
//
// The union-find: L[x] is x (a root) or a smaller pixel index of the same component.  Labels only ever decrease, every write is an
// atomic minimum, and nobody waits for anybody: a lost race shows as a value that is not the one expected, and the loser goes on with
// what it read.  Every loop carries an iteration bound (the pixels of the view are enough: a path has no more steps, and a union is
// retried only when another union succeeded); on exhaustion *failed is set and the walk ends where it is.
//
// How labels are read and written is the includer's: CC_LABEL_T, CC_LOAD(p), CC_FETCH_MIN(p, v) (returns the old value).  Kernels take
// agent-scope relaxed atomics -- other blocks write labels while they are read, and plain accesses are served by an XCD's own L2 -- the
// CPU check takes std::atomic<int>; left undefined, plain C accesses for one thread.
#pragma once
#include "sl3d_mesh.h"

#ifdef __HIPCC__
#define SL3D_CC_FN __device__ __forceinline__
#else
#define SL3D_CC_FN static inline
#endif

#ifndef CC_LABEL_T
#define CC_LABEL_T int
#ifdef __HIPCC__
#define CC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CC_FETCH_MIN(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
static inline int cc_plain_fetch_min(int *p, int v)
{
    const int old = *p;
    if (v < old) *p = v;
    return old;
}
#define CC_LOAD(p) (*(p))
#define CC_FETCH_MIN(p, v) cc_plain_fetch_min((p), (v))
#endif
#endif

// Does face f (0..1) of a cell survive the filter?  A face's vertices share a component, so one of them decides: its first, which is a
// or b in all four shapes -- a pixel of the cell's upper row.  keep_a / keep_b: whether the components of those corners are kept.
SL3D_CC_FN int cc_face_kept(unsigned cell, int f, int keep_a, int keep_b) { return mesh_corner(cell, f, 0) == MESH_A ? keep_a : keep_b; }

// ---- the union-find ----------------------------------------------------------------------------------------------------------------
// the root of x.  On the way every visited entry is lowered to its grandparent (path halving: an atomic minimum like every other write)
SL3D_CC_FN int cc_find(CC_LABEL_T *L, int x, int bound, int *failed)
{
    int p = CC_LOAD(L + x);
    while (p != x) {
        if (bound-- <= 0) {
            *failed = 1;
            return x;
        }
        const int g = CC_LOAD(L + p);
        if (g != p) CC_FETCH_MIN(L + x, g);
        x = p, p = g;
    }
    return x;
}

// joins the components of a and b: the larger root is hung under the smaller.  If the larger root has found another parent in the
// meantime the minimum may have replaced that parent by b -- so the walk goes on joining THAT parent and b, and no link is lost.
SL3D_CC_FN void cc_union(CC_LABEL_T *L, int a, int b, int bound, int *failed)
{
    for (int tries = bound;;) {
        a = cc_find(L, a, bound, failed);
        b = cc_find(L, b, bound, failed);
        if (*failed || a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = CC_FETCH_MIN(L + a, b);
        if (old == a) return;
        if (tries-- <= 0) {
            *failed = 1;
            return;
        }
        a = old;
    }
}

// the unions of the cell whose corner a is pixel pa (pixel indices: b = pa + 1, d = pa + pitch, e = pa + pitch + 1): every corner the
// faces touch joins the first of them
SL3D_CC_FN void cc_cell_unions(CC_LABEL_T *L, unsigned code, int pa, int pitch, int bound, int *failed)
{
    const unsigned cs = cc_code_corners(code);
    if (!cs) return;
    const int first = (cs & 1u) ? pa : pa + 1;
    if ((cs & 3u) == 3u) cc_union(L, first, pa + 1, bound, failed);
    if (cs & 4u) cc_union(L, first, pa + pitch, bound, failed);
    if (cs & 8u) cc_union(L, first, pa + pitch + 1, bound, failed);
}
