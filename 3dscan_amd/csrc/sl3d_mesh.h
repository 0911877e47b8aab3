// sl3d_mesh.h -- the arithmetic of the mesh stage (sl3d_mesh_views): which triangles one cell of the organized point grid gives.
//
// Shared by every mesh kernel (sl3d_mesh.hip, sl3d_mesh_normals.hip, sl3d_mesh_components.hip, sl3d_mesh_smooth.hip) and by the CPU
// checks the test suite runs over whole frames (tests/native/mesh_*_check.cpp): plain C, no HIP types.  The reference has no mesh stage
// (its user meshed the PLY of stage 8 in MeshLab); the definition is this library's own and every test checks it bit for bit:
//
//   cell (r, c), r in [0, H-1), c in [0, W-1): corners a = (r, c), b = (r, c+1), d = (r+1, c), e = (r+1, c+1)
//   len2(p, q) = (dx*dx + dy*dy) + dz*dz with dx = (double)p.x - (double)q.x ..., IEEE double, no contraction
//   an edge is short iff len2 <= thr2 = (double)max_edge * (double)max_edge   (a NaN len2 is not short)
//   4 valid corners: diagonal a-e iff len2(a, e) <= len2(b, d) (a tie takes a-e, a NaN on either side b-d)
//                    a-e: candidates (a, d, e) then (a, e, b);   b-d: candidates (a, d, b) then (b, d, e)
//   3 valid corners: e missing (a, d, b); a missing (b, d, e); b missing (a, d, e); d missing (a, e, b)
//   a candidate is a face iff its three edges are short.  All four shapes have the same orientation in pixel space.
//
// Vertex normals (sl3d_mesh_normals; k_mesh_normals in sl3d_mesh_normals.hip, tests/native/mesh_normals_check.cpp), equally exact:
//   face (i, j, k) with points p, q, s widened to double: u = q - p, v = s - p,
//        fn = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x), every operation one IEEE double operation, no contraction
//   vertex at pixel (r, c): acc = +0, then acc += fn for every face that contains it in face-list order: cells (r-1, c-1), (r-1, c),
//        (r, c-1), (r, c), within a cell the cell's face order -- at most 8 faces
//   ss = (acc.x*acc.x + acc.y*acc.y) + acc.z*acc.z;  0 < ss < +inf: n = (float)(acc / sqrt(ss)) per component (sqrt and division
//        correctly rounded in double, the cast to nearest even), else n = +0 (no face, degenerate faces, overflow, NaN)
//   for points (col, row, f(col, row)) this is (f_x, f_y, -1) / |..|: the orientation follows the faces, nothing is flipped
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define SL3D_MESH_FN __host__ __device__ __forceinline__
#define SL3D_MESH_UNROLL _Pragma("unroll")
#else
#define SL3D_MESH_FN static inline
#define SL3D_MESH_UNROLL
#endif

#define MESH_CHUNK 1024  // pixels of a row per block of the mesh kernels: 256 lanes x one quad

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

// ---- the cell plane ------------------------------------------------------------------------------------------------------------
// mesh_cell has seven outcomes -- no face, one of the four shapes, or one of the two pairs -- so a byte per cell (cc_cell_code) keeps
// everything later passes need: what the cell connects, and its faces in output order (cc_code_cell gives the mesh_cell result back),
// without evaluating the doubles again.  Written by k_mesh_cells (sl3d_mesh.hip) for the components and the smoothing calls.
#define CC_ADE MESH_TRI(MESH_A, MESH_D, MESH_E)
#define CC_AEB MESH_TRI(MESH_A, MESH_E, MESH_B)
#define CC_ADB MESH_TRI(MESH_A, MESH_D, MESH_B)
#define CC_BDE MESH_TRI(MESH_B, MESH_D, MESH_E)

// a mesh_cell result as a code: 0 no face; 1 (a,d,e); 2 (a,e,b); 3 (a,d,b); 4 (b,d,e); 5 (a,d,e)(a,e,b); 6 (a,d,b)(b,d,e)
SL3D_MESH_FN unsigned cc_cell_code(unsigned cell)
{
    const unsigned n = cell & 3u, t0 = cell >> 2 & 63u;
    if (n == 0u) return 0u;
    if (n == 2u) return t0 == CC_ADE ? 5u : 6u;
    return t0 == CC_ADE ? 1u : t0 == CC_AEB ? 2u : t0 == CC_ADB ? 3u : 4u;
}

// ... and back
SL3D_MESH_FN unsigned cc_code_cell(unsigned code)
{
    switch (code & 7u) {
    case 1u: return 1u | CC_ADE << 2;
    case 2u: return 1u | CC_AEB << 2;
    case 3u: return 1u | CC_ADB << 2;
    case 4u: return 1u | CC_BDE << 2;
    case 5u: return 2u | CC_ADE << 2 | CC_AEB << 8;
    case 6u: return 2u | CC_ADB << 2 | CC_BDE << 8;
    default: return 0u;
    }
}

// the corners the faces of a code touch, bit MESH_A.. as in mesh_cell's vbits: these are what the cell connects
SL3D_MESH_FN unsigned cc_code_corners(unsigned code) { return 0x0ffe7bd0u >> (4u * (code & 7u)) & 15u; }

// ---- vertex normals ------------------------------------------------------------------------------------------------------------------
// the area-weighted normal of the face (p, q, s), in the order the face list gives its vertices
SL3D_MESH_FN void mesh_face_vector(const float *p, const float *q, const float *s, double out[3])
{
    const double ux = (double)q[0] - (double)p[0], uy = (double)q[1] - (double)p[1], uz = (double)q[2] - (double)p[2];
    const double vx = (double)s[0] - (double)p[0], vy = (double)s[1] - (double)p[1], vz = (double)s[2] - (double)p[2];
    out[0] = uy * vz - uz * vy;
    out[1] = uz * vx - ux * vz;
    out[2] = ux * vy - uy * vx;
}

SL3D_MESH_FN void mesh_normal_from_sum(const double acc[3], float out[3])
{
    const double ss = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2];
    out[0] = out[1] = out[2] = 0.0f;
    if (ss > 0.0 && ss < (double)INFINITY) {  // (false for NaN)
        const double len = sqrt(ss);
        out[0] = (float)(acc[0] / len), out[1] = (float)(acc[1] / len), out[2] = (float)(acc[2] / len);
    }
}

// one of two points by a flag (selects on values already loaded, no indexed array: the kernel keeps the points in registers)
SL3D_MESH_FN void mesh_pick(int first, const float *x, const float *y, float out[3])
{
    const float x0 = x[0], x1 = x[1], x2 = x[2], y0 = y[0], y1 = y[1], y2 = y[2];
    out[0] = first ? x0 : y0, out[1] = first ? x1 : y1, out[2] = first ? x2 : y2;
}

// The faces of one cell -- `cell`: its mesh_cell result, a / b / d / e: its corners' points -- add their vectors to the sums of the cell's
// corners `left` and `right`.  j (0..4): the column of corner a among a quad's 6 columns; `left` is pixel j - 1 of the quad (none for
// j = 0), `right` pixel j (none for j = 4); acc[3 * k ..]: the sum of pixel k.  Face 0 before face 1, `left` before `right`.
SL3D_MESH_FN void mesh_cell_sums(unsigned cell, const float *a, const float *b, const float *d, const float *e, int j, unsigned left, unsigned right,
                                 double acc[12])
{
    SL3D_MESH_UNROLL
    for (int f = 0; f < 2; f++)
        if ((int)(cell & 3u) > f) {
            const unsigned c0 = mesh_corner(cell, f, 0), c1 = mesh_corner(cell, f, 1), c2 = mesh_corner(cell, f, 2);
            // the four shapes mesh_cell gives -- (a,d,e) (a,e,b) (a,d,b) (b,d,e) -- start at a or b, go on to d or e and end at e or b
            float p[3], q[3], s[3];
            double fn[3];
            mesh_pick(c0 == MESH_A, a, b, p);
            mesh_pick(c1 == MESH_D, d, e, q);
            mesh_pick(c2 == MESH_E, e, b, s);
            mesh_face_vector(p, q, s, fn);
            const unsigned has = 1u << c0 | 1u << c1 | 1u << c2;
            if (j >= 1 && (has >> left & 1u)) acc[3 * j - 3] += fn[0], acc[3 * j - 2] += fn[1], acc[3 * j - 1] += fn[2];
            if (j <= 3 && (has >> right & 1u)) acc[3 * j] += fn[0], acc[3 * j + 1] += fn[1], acc[3 * j + 2] += fn[2];
        }
}

// The cells of one cell row under a quad's 6 columns, left to right: the cell whose corner a is column j (0..4) adds its faces' vectors
// to the sums of its corners `left` (pixel j - 1 of the quad) and `right` (pixel j).  vu / vl: valid bits of the cells' upper / lower
// pixel row, bit j = column j; up / lo: the points of those rows (18 floats each; those of invalid pixels are not looked at).
SL3D_MESH_FN void mesh_cell_row_sums(unsigned vu, unsigned vl, const float *up, const float *lo, unsigned left, unsigned right, double thr2,
                                     double acc[12])
{
    SL3D_MESH_UNROLL
    for (int j = 0; j < 5; j++) {
        const float *a = up + 3 * j, *b = a + 3, *d = lo + 3 * j, *e = d + 3;
        mesh_cell_sums(mesh_cell((vu >> j & 3u) | (vl >> j & 3u) << 2, a, b, d, e, thr2), a, b, d, e, j, left, right, acc);
    }
}

// The face-vector sums of one quad: pixels c0 .. c0 + 3 of row r.  v[t], t = 0..2: the valid bits of row r - 1 + t, bit j = pixel
// c0 - 1 + j (j = 0..5; 0 outside the window); pt / pm / pb: the points of those 6 pixels of rows r - 1 / r / r + 1.  acc[3 * k ..]: the
// sum of pixel c0 + k.  The 5 cells of row r - 1 (the quad's pixels are their corners d / e), then the 5 of row r (corners a / b): for
// every pixel that is the order (r-1, c-1), (r-1, c), (r, c-1), (r, c) of the definition.
SL3D_MESH_FN void mesh_quad_sums(const unsigned v[3], const float *pt, const float *pm, const float *pb, double thr2, double acc[12])
{
    SL3D_MESH_UNROLL
    for (int i = 0; i < 12; i++) acc[i] = 0.0;
    mesh_cell_row_sums(v[0], v[1], pt, pm, MESH_D, MESH_E, thr2, acc);
    mesh_cell_row_sums(v[1], v[2], pm, pb, MESH_A, MESH_B, thr2, acc);
}
