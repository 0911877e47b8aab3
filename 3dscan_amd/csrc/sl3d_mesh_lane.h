// sl3d_mesh_lane.h -- what a lane of the mesh kernels loads and decides, each spelled once: the valid (keep, cell-code) bytes and the points
// of its quad and of the pixels around it, the 4 cells of its quad, the faces it stages.  Shared by the kernels of sl3d_mesh.hip,
// sl3d_mesh_normals.hip, sl3d_mesh_components.hip and sl3d_mesh_smooth.hip, inlined into each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_mesh.h"

namespace sl3d {

// the 4 valid (or keep) bits of the lane's quad -- pixels c0 .. c0 + 3 of a 0/1 byte plane row, `quad`: the first of them -- clipped to the
// window; 0 for a quad beyond it
__device__ __forceinline__ unsigned quad_bits(const uint8_t *__restrict__ quad, int W, int c0)
{
    if (c0 >= W) return 0u;
    const unsigned in_w = QUAD_IN_WINDOW(W, c0);
    return valid_nibble(*(const unsigned *)quad) & in_w;
}

// the 5 bits of pixels c0 .. c0 + 4 of a 0/1 byte plane row (bit 4: the pixel right of the quad; 0 beyond the window or without the row)
__device__ __forceinline__ unsigned quad_bits5(const uint8_t *__restrict__ row, int W, int c0, bool have_row)
{
    if (c0 >= W || !have_row) return 0u;
    const unsigned right = c0 + 4 < W ? row[c0 + 4] : 0u;
    return quad_bits(row + c0, W, c0) | (right & 1u) << 4;
}

// the codes of the lane's 4 cells as the dword of the cell plane (byte k = cc_cell_code of cell k)
__device__ __forceinline__ unsigned cell_codes(const unsigned cell[4])
{
    return cc_cell_code(cell[0]) | cc_cell_code(cell[1]) << 8 | cc_cell_code(cell[2]) << 16 | cc_cell_code(cell[3]) << 24;
}

// the codes of the cells of columns c0 - 1 .. c0 + 3 of a cell-plane row, byte j = column c0 - 1 + j; 0 without the row (c0 < W: the dword
// was written whole by k_mesh_cells, cells beyond the window as 0)
__device__ __forceinline__ unsigned long long cell_codes5(const uint8_t *__restrict__ row, int c0, bool have_row)
{
    if (!have_row) return 0ull;
    const unsigned left = c0 > 0 ? row[c0 - 1] : 0u;
    return (unsigned long long)*(const unsigned *)(row + c0) << 8 | left;
}

// the points of a quad -- 4 pixels, 12 floats, 16-byte aligned -- as three 16-byte loads
__device__ __forceinline__ void load_quad(const float *__restrict__ p, float q[12])
{
    const float4 *p4 = (const float4 *)p;
    const float4 a = p4[0], b = p4[1], d = p4[2];
    q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w, q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w, q[8] = d.x, q[9] = d.y, q[10] = d.z, q[11] = d.w;
}

// The points of pixels c0 - 1 .. c0 + 4 of one row of a plane as 18 floats: columns c0 .. c0 + 3 as 16-byte loads if `quad`, the pixels left
// and right of them if asked for (lines the neighbouring lanes request anyway); what is not loaded is 0.  p: the row's pixel c0
__device__ __forceinline__ void load_row6(const float *__restrict__ p, bool quad, bool left, bool right, float q[18])
{
#pragma unroll
    for (int i = 0; i < 12; i++) q[3 + i] = 0.0f;
    if (quad) load_quad(p, q + 3);
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = left ? p[i - 3] : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) q[15 + i] = right ? p[12 + i] : 0.0f;
}

// the lane's 4 cells (a = pixel c0 + k of row r): v0 / v1 = valid bits of pixels c0 .. c0 + 4 of rows r / r + 1 (bit 4: the pixel right
// of the quad; 0 beyond the window), cell[k] = mesh_cell of cell k.  row0 / pts0: row r of the valid / points plane.
__device__ __forceinline__ void mesh_lane(const uint8_t *__restrict__ row0, const float *__restrict__ pts0, int W, int pitch, int c0, bool next_row,
                                          double thr2, unsigned &v0, unsigned &v1, unsigned cell[4])
{
    v0 = v1 = 0u;
    cell[0] = cell[1] = cell[2] = cell[3] = 0u;
    if (c0 >= W) return;
    const unsigned in_w = QUAD_IN_WINDOW(W, c0);
    const bool right = c0 + 4 < W;
    // every valid byte the lane needs, requested before the first is looked at
    const unsigned w0 = *(const unsigned *)(row0 + c0);
    const unsigned w1 = next_row ? *(const unsigned *)(row0 + pitch + c0) : 0u;
    const unsigned r0 = right ? row0[c0 + 4] : 0u;
    const unsigned r1 = right && next_row ? row0[pitch + c0 + 4] : 0u;
    v0 = (valid_nibble(w0) & in_w) | (r0 & 1u) << 4;
    v1 = (valid_nibble(w1) & in_w) | (r1 & 1u) << 4;
    if (!v0 || !v1) return;  // a face has a corner in either row
    const float *p0 = pts0 + 3 * (size_t)c0, *p1 = pts0 + 3 * ((size_t)pitch + c0);
    float q0[15] = {}, q1[15] = {};  // (the pixel right of the quad: 0 unless valid)
    load_quad(p0, q0);
    load_quad(p1, q1);
    if (v0 & 16u) {
        const float *s = pts0 + 3 * (size_t)(c0 + 4);
        q0[12] = s[0], q0[13] = s[1], q0[14] = s[2];
    }
    if (v1 & 16u) {
        const float *s = pts0 + 3 * ((size_t)pitch + c0 + 4);
        q1[12] = s[0], q1[13] = s[1], q1[14] = s[2];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned vb = (v0 >> k & 3u) | (v1 >> k & 3u) << 2;  // a, b, d, e
        cell[k] = mesh_cell(vb, &q0[3 * k], &q0[3 * k + 3], &q1[3 * k], &q1[3 * k + 3], thr2);
    }
}

// The faces of the lane's 4 cells go to s_faces at `rank`, `rank + 1` ...: every face of a cell (ALL; keep is not looked at), or face f of
// cell k iff bit f of keep[k].  id0 / id1: the vertex ids
// of the first valid (kept) pixel at or behind c0 in rows r / r + 1; v0 / v1: the valid (keep) bits of pixels c0 .. c0 + 4 of those rows
template <bool ALL>
__device__ __forceinline__ void stage_faces(int id0, int id1, unsigned v0, unsigned v1, const unsigned cells[4], const unsigned keep[4], unsigned rank,
                                            int *s_faces)
{
    const unsigned cell[4] = {cells[0], cells[1], cells[2], cells[3]};  // (a copy: read through the caller's array the loop below compiles to more)
    int id[2][5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        id[0][j] = id0 + __popc(v0 & ((1u << j) - 1u));
        id[1][j] = id1 + __popc(v1 & ((1u << j) - 1u));
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int f = 0; f < 2; f++)
            if (ALL ? (int)(cell[k] & 3u) > f : (bool)(keep[k] >> f & 1u)) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const unsigned cn = mesh_corner(cell[k], f, j);
                    const int lo = (cn & 2u) ? id[1][k] : id[0][k], hi = (cn & 2u) ? id[1][k + 1] : id[0][k + 1];
                    s_faces[3 * rank + j] = (cn & 1u) ? hi : lo;
                }
                rank++;
            }
}

}  // namespace sl3d
