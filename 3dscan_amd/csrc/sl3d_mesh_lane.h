// sl3d_mesh_lane.h -- what a lane of the mesh kernels loads and decides: the 4 cells of its quad.  Shared by k_mesh_count / k_mesh_emit
// (sl3d_mesh.hip) and k_cc_cells (sl3d_mesh_components.hip), inlined into each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_mesh.h"

namespace sl3d {

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
    const float4 *p0 = (const float4 *)(pts0 + 3 * (size_t)c0);
    const float4 *p1 = (const float4 *)(pts0 + 3 * ((size_t)pitch + c0));
    const float4 a0 = p0[0], a1 = p0[1], a2 = p0[2], b0 = p1[0], b1 = p1[1], b2 = p1[2];
    float q0[15] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, 0.0f, 0.0f, 0.0f};
    float q1[15] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, 0.0f, 0.0f, 0.0f};
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

}  // namespace sl3d
