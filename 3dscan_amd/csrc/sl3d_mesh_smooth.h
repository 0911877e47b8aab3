// sl3d_mesh_smooth.h -- the arithmetic of the smoothing stage (sl3d_mesh_smooth; the definition: include/sl3d.h): which of the 8 pixels
// around a vertex are its neighbours, one umbrella step, and the face-vector sums of the smoothed mesh.  Shared by the kernels of
// sl3d_mesh_smooth.hip and by the CPU check the test suite runs over whole frames (tests/native/mesh_smooth_check.cpp): plain C, no HIP
// types.
//
//   neighbours   two vertices are neighbours iff some face of the mesh sl3d_mesh_views defines contains both: the faces of a vertex lie in
//                the four cells around its pixel, so its neighbours are among the 8 pixels around it -- the ring byte, bit j = neighbour j
//                in scan order: (r-1,c-1), (r-1,c), (r-1,c+1), (r,c-1), (r,c+1), (r+1,c-1), (r+1,c), (r+1,c+1)
//   boundary     an edge in exactly one face; a boundary vertex is an endpoint of one.  With SL3D_SMOOTH_FIX_BOUNDARY its ring is 0:
//                "fixed" and "no neighbour" are the same to a step, and a fixed vertex stays in the rings of its neighbours
//   one step     s = +0, then s += (double)neighbour for the ring's bits in ascending order; m = s / (double)k;
//                p' = (float)((double)p + f * (m - (double)p)); every operation one IEEE double operation, nothing contracted;
//                ring 0: p' = p bitwise.  All vertices read the positions of the step before (Jacobi)
//   normals      the definition of sl3d_mesh.h over the smoothed positions with the ORIGINAL connectivity: the cells come from the cell
//                plane (cc_cell_code, sl3d_mesh.h), never from positions that have moved
#pragma once
#include "sl3d_mesh.h"

#define SL3D_SMOOTH_FN SL3D_MESH_FN

// ---- the ring ------------------------------------------------------------------------------------------------------------------------
// what the faces of one cell add to the edge counts of the vertex at corner `me` of that cell: 2 bits per direction (bit pair j =
// neighbour j), the number of faces that contain the edge to that neighbour.  A cell has at most 2 faces and an edge lies in at most 2
// faces of the whole mesh: no pair overflows
SL3D_SMOOTH_FN unsigned smooth_cell_edges(unsigned code, unsigned me)
{
    const unsigned cell = cc_code_cell(code);
    unsigned cnt = 0u;
    SL3D_MESH_UNROLL
    for (int f = 0; f < 2; f++) {
        if ((int)(cell & 3u) <= f) continue;
        const unsigned c0 = mesh_corner(cell, f, 0), c1 = mesh_corner(cell, f, 1), c2 = mesh_corner(cell, f, 2);
        if (c0 != me && c1 != me && c2 != me) continue;
        SL3D_MESH_UNROLL
        for (int j = 0; j < 3; j++) {
            const unsigned x = j == 0 ? c0 : j == 1 ? c1 : c2;
            if (x == me) continue;
            // corner numbers: bit 1 = the lower pixel row, bit 0 = the right pixel column
            const int dr = (int)(x >> 1) - (int)(me >> 1), dc = (int)(x & 1u) - (int)(me & 1u), at = 3 * (dr + 1) + (dc + 1);
            cnt += 1u << (2 * (at - (at > 4)));
        }
    }
    return cnt;
}

// The ring byte of the vertex at pixel (r, c) from the codes of the cells (r-1,c-1), (r-1,c), (r,c-1), (r,c) -- the pixel is their corner
// e, d, b, a; 0 for a cell outside the window.  A pixel that is no vertex of a face (an invalid one among them) gets 0.
SL3D_SMOOTH_FN unsigned smooth_ring(unsigned c00, unsigned c01, unsigned c10, unsigned c11, int fix_boundary)
{
    const unsigned cnt = smooth_cell_edges(c00, MESH_E) + smooth_cell_edges(c01, MESH_D) + smooth_cell_edges(c10, MESH_B) + smooth_cell_edges(c11, MESH_A);
    const unsigned lo = cnt & 0x5555u, hi = cnt >> 1 & 0x5555u;
    if (fix_boundary && (lo & ~hi)) return 0u;  // an edge in exactly one face
    const unsigned any = lo | hi;
    unsigned ring = 0u;
    SL3D_MESH_UNROLL
    for (int j = 0; j < 8; j++) ring |= (any >> (2 * j) & 1u) << j;
    return ring;
}

// the rings of a quad (pixels c0 .. c0 + 3 of row r) as one dword, byte k = pixel c0 + k.  up / mid: the codes of the cells of rows r - 1 /
// r, byte j = cell column c0 - 1 + j (j = 0..4; 0 outside the window)
SL3D_SMOOTH_FN unsigned smooth_quad_rings(unsigned long long up, unsigned long long mid, int fix_boundary)
{
    unsigned rings = 0u;
    SL3D_MESH_UNROLL
    for (int k = 0; k < 4; k++)
        rings |= smooth_ring((unsigned)(up >> (8 * k)) & 255u, (unsigned)(up >> (8 * k + 8)) & 255u, (unsigned)(mid >> (8 * k)) & 255u,
                             (unsigned)(mid >> (8 * k + 8)) & 255u, fix_boundary)
                 << (8 * k);
    return rings;
}

// ---- one step --------------------------------------------------------------------------------------------------------------------------
// One step of a quad.  rings: smooth_quad_rings' dword; pt / pm / pb: the points of pixels c0 - 1 .. c0 + 4 of rows r - 1 / r / r + 1 (18
// floats each; only those a ring bit points at, and the quad's own, are looked at); out: the 4 new positions.  Neighbours are picked by
// selects on values already loaded, no indexed array: the kernel keeps the points in registers
SL3D_SMOOTH_FN void smooth_step(unsigned rings, const float *pt, const float *pm, const float *pb, double f, float out[12])
{
    SL3D_MESH_UNROLL
    for (int k = 0; k < 4; k++) {
        const unsigned ring = rings >> (8 * k) & 255u;
        const double n = (double)(int)__builtin_popcount(ring);
        SL3D_MESH_UNROLL
        for (int i = 0; i < 3; i++) {
            const float nb[8] = {pt[3 * k + i], pt[3 * k + 3 + i], pt[3 * k + 6 + i], pm[3 * k + i], pm[3 * k + 6 + i], pb[3 * k + i], pb[3 * k + 3 + i],
                                 pb[3 * k + 6 + i]};
            double s = 0.0;
            SL3D_MESH_UNROLL
            for (int j = 0; j < 8; j++) {
                const double t = s + (double)nb[j];
                s = (ring >> j & 1u) ? t : s;
            }
            const float p = pm[3 * k + 3 + i];
            const double pd = (double)p, m = s / n;
            const float moved = (float)(pd + f * (m - pd));
            out[3 * k + i] = ring ? moved : p;
        }
    }
}

// ---- normals of the smoothed mesh: mesh_cell_row_sums / mesh_quad_sums (sl3d_mesh.h) with cell codes in place of mesh_cell -------------
// codes: byte j = the code of the cell whose corner a is column j (0..4) of the 6 columns; everything else as in mesh_cell_row_sums
SL3D_SMOOTH_FN void smooth_cell_row_sums(unsigned long long codes, const float *up, const float *lo, unsigned left, unsigned right, double acc[12])
{
    SL3D_MESH_UNROLL
    for (int j = 0; j < 5; j++) {
        const float *a = up + 3 * j, *b = a + 3, *d = lo + 3 * j, *e = d + 3;
        mesh_cell_sums(cc_code_cell((unsigned)(codes >> (8 * j)) & 255u), a, b, d, e, j, left, right, acc);
    }
}

// up / mid: the cell codes of rows r - 1 / r as smooth_quad_rings takes them; pt / pm / pb: the (smoothed) points of the 6 pixels of rows
// r - 1 / r / r + 1; acc[3 * k ..]: the face-vector sum of pixel c0 + k, in the order of the definition
SL3D_SMOOTH_FN void smooth_quad_sums(unsigned long long up, unsigned long long mid, const float *pt, const float *pm, const float *pb, double acc[12])
{
    SL3D_MESH_UNROLL
    for (int i = 0; i < 12; i++) acc[i] = 0.0;
    smooth_cell_row_sums(up, pt, pm, MESH_D, MESH_E, acc);
    smooth_cell_row_sums(mid, pm, pb, MESH_A, MESH_B, acc);
}

// which of the 6 pixels of the cells' upper (low 6 bits) and lower (bits 8..13) row are corners of a face of the 5 cells: the points a
// gather has to load -- all of them vertices, so their positions in a smoothed plane are written
SL3D_SMOOTH_FN unsigned smooth_row_corners(unsigned long long codes)
{
    unsigned v = 0u;
    SL3D_MESH_UNROLL
    for (int j = 0; j < 5; j++) {
        const unsigned cs = cc_code_corners((unsigned)(codes >> (8 * j)) & 255u);
        v |= (cs & 3u) << j | (cs >> 2 & 3u) << (8 + j);
    }
    return v;
}
