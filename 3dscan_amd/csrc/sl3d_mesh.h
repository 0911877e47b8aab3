// sl3d_mesh.h -- the arithmetic of the mesh stage (sl3d_mesh_views): which triangles one cell of the organized point grid gives.
//
// Shared by k_mesh_count / k_mesh_emit (sl3d_mesh.hip) and by the CPU check the test suite runs over whole frames
// (tests/native/mesh_check.cpp): plain C, no HIP types.  The reference has no mesh stage (its user meshed the PLY of stage 8 in
// MeshLab); the definition is this library's own and every test checks it bit for bit:
//
//   cell (r, c), r in [0, H-1), c in [0, W-1): corners a = (r, c), b = (r, c+1), d = (r+1, c), e = (r+1, c+1)
//   len2(p, q) = (dx*dx + dy*dy) + dz*dz with dx = (double)p.x - (double)q.x ..., IEEE double, no contraction
//   an edge is short iff len2 <= thr2 = (double)max_edge * (double)max_edge   (a NaN len2 is not short)
//   4 valid corners: diagonal a-e iff len2(a, e) <= len2(b, d) (a tie takes a-e, a NaN on either side b-d)
//                    a-e: candidates (a, d, e) then (a, e, b);   b-d: candidates (a, d, b) then (b, d, e)
//   3 valid corners: e missing (a, d, b); a missing (b, d, e); b missing (a, d, e); d missing (a, e, b)
//   a candidate is a face iff its three edges are short.  All four shapes have the same orientation in pixel space.
#pragma once

#ifdef __HIPCC__
#define SL3D_MESH_FN __host__ __device__ __forceinline__
#else
#define SL3D_MESH_FN static inline
#endif

// corner numbers of a cell, also the bit numbers of `vbits`
#define MESH_A 0
#define MESH_B 1
#define MESH_D 2
#define MESH_E 3
#define MESH_TRI(p, q, s) ((unsigned)(p) | (unsigned)(q) << 2 | (unsigned)(s) << 4)

SL3D_MESH_FN double mesh_len2(const float *p, const float *q)
{
    const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

SL3D_MESH_FN int mesh_short(double len2, double thr2) { return len2 <= thr2; }  // false for NaN

SL3D_MESH_FN double mesh_thr2(float max_edge) { return (double)max_edge * (double)max_edge; }

// The faces of one cell.  vbits: bit MESH_A.. set iff that corner is valid; the points of invalid corners are not looked at.
// Returns n | face0 << 2 | face1 << 8: n = number of faces (0..2), face k = MESH_TRI of its three corner numbers, in output order.
SL3D_MESH_FN unsigned mesh_cell(unsigned vbits, const float *a, const float *b, const float *d, const float *e, double thr2)
{
    unsigned t0, t1 = 0;
    int s0, s1 = 0;
    switch (vbits & 15u) {
    case 15u: {
        const double ae = mesh_len2(a, e), bd = mesh_len2(b, d);
        const int ad = mesh_short(mesh_len2(a, d), thr2), de = mesh_short(mesh_len2(d, e), thr2);
        const int ab = mesh_short(mesh_len2(a, b), thr2), be = mesh_short(mesh_len2(b, e), thr2);
        if (ae <= bd) {
            const int dg = mesh_short(ae, thr2);
            t0 = MESH_TRI(MESH_A, MESH_D, MESH_E), s0 = ad & de & dg;
            t1 = MESH_TRI(MESH_A, MESH_E, MESH_B), s1 = dg & be & ab;
        } else {
            const int dg = mesh_short(bd, thr2);
            t0 = MESH_TRI(MESH_A, MESH_D, MESH_B), s0 = ad & dg & ab;
            t1 = MESH_TRI(MESH_B, MESH_D, MESH_E), s1 = dg & de & be;
        }
        break;
    }
    case 7u:  // e missing
        t0 = MESH_TRI(MESH_A, MESH_D, MESH_B);
        s0 = mesh_short(mesh_len2(a, d), thr2) & mesh_short(mesh_len2(d, b), thr2) & mesh_short(mesh_len2(b, a), thr2);
        break;
    case 14u:  // a missing
        t0 = MESH_TRI(MESH_B, MESH_D, MESH_E);
        s0 = mesh_short(mesh_len2(b, d), thr2) & mesh_short(mesh_len2(d, e), thr2) & mesh_short(mesh_len2(e, b), thr2);
        break;
    case 13u:  // b missing
        t0 = MESH_TRI(MESH_A, MESH_D, MESH_E);
        s0 = mesh_short(mesh_len2(a, d), thr2) & mesh_short(mesh_len2(d, e), thr2) & mesh_short(mesh_len2(e, a), thr2);
        break;
    case 11u:  // d missing
        t0 = MESH_TRI(MESH_A, MESH_E, MESH_B);
        s0 = mesh_short(mesh_len2(a, e), thr2) & mesh_short(mesh_len2(e, b), thr2) & mesh_short(mesh_len2(b, a), thr2);
        break;
    default:
        return 0u;
    }
    if (s0) return (unsigned)(1 + s1) | t0 << 2 | t1 << 8;
    return s1 ? (1u | t1 << 2) : 0u;
}

// corner number j (0..2) of face k (0..1) of a mesh_cell result
SL3D_MESH_FN unsigned mesh_corner(unsigned cell, int k, int j) { return (cell >> (2 + 6 * k + 2 * j)) & 3u; }
