// sl3d_mesh_smooth.hip -- Taubin / Laplacian smoothing of the mesh sl3d_mesh_views defines, and the normals of the smoothed mesh
// (sl3d_mesh_smooth; the definition, the ring and the step: sl3d_mesh_smooth.h).  The grid gives the adjacency: a vertex's neighbours are
// among the 8 pixels around it, and which of them follows from the faces of the four cells around the pixel.  A fixed sequence of
// launches over the mesh kernels' chunks (1024 pixels of ONE row, a lane owning one quad):
//   k_mesh_cells and k_compact_scan over the count array of every view (launch_mesh_cells, sl3d_mesh.hip): mesh_cell of every cell
//                      ONCE, from the ORIGINAL positions, left as a byte per cell (cc_cell_code); per chunk its valid pixels and their scan
//   k_smooth_ring    : ring byte of every pixel from the four cell bytes around it (smooth_quad_rings): integers only, no points
//   k_smooth_step    : once per step.  A lane loads its ring dword and the points of rows r - 1, r, r + 1, columns c0 - 1 .. c0 + 4 that a
//                      ring bit points at, evaluates smooth_step and stores its quad.  Ping-pong between two planes of the dense layout;
//                      the first step reads the context's own point plane, which is never written.  A vertex with ring 0 (no neighbour, or
//                      fixed) stores its old position: the destination is complete for the next step under every valid pixel.  Positions
//                      under invalid pixels are never looked at -- a ring bit only ever points at a vertex of a face -- so the planes need no
//                      initialisation
//   k_smooth_out     : the final plane compacted into the other one: chunk offset from the scan, wave-prefix rank, LDS staging, one coalesced run per chunk
//   k_smooth_normals : (on request) the gather of k_mesh_normals over the final plane with cell bytes in place of mesh_cell
// No atomics, no block waits for another, nothing depends on the data: the result follows from the planes and the scan alone.
// The block idioms live in sl3d_block.h, a lane's loads (quad_bits, cell_codes5, load_quad, load_row6) in sl3d_mesh_lane.h.  k_smooth_out
// and k_smooth_normals write their ordered output (rank, staging, barrier, flush) out: one helper for it changed their instruction
// histograms and was not measured (profiles/mesh_idioms_identity.txt).
#include <hip/hip_runtime.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh_lane.h"
#include "sl3d_mesh_smooth.h"

namespace sl3d {

// grid (chunks of a row, H, views); rings: [view][view_stride]
__global__ __launch_bounds__(256) void k_smooth_ring(const uint8_t *__restrict__ cells, int W, int pitch, size_t view_stride, int fix_boundary,
                                                     uint8_t *__restrict__ rings)
{
    const int r = blockIdx.y, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    if (c0 >= W) return;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    const unsigned long long mid = cell_codes5(cells + row, c0, true), up = cell_codes5(cells + row - pitch, c0, r > 0);
    *(unsigned *)(rings + row + c0) = (up | mid) ? smooth_quad_rings(up, mid, fix_boundary) : 0u;
}

// grid (chunks of a row, H, views); src / dst: [view][view_stride][3]; f: the step's factor
__global__ __launch_bounds__(256) void k_smooth_step(const uint8_t *__restrict__ valid, const uint8_t *__restrict__ rings, const float *__restrict__ src,
                                                     int W, int pitch, size_t view_stride, double f, float *__restrict__ dst)
{
    const int r = blockIdx.y, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    if (c0 >= W) return;
    const size_t px = (size_t)blockIdx.z * view_stride + (size_t)r * pitch + c0;
    const unsigned own = quad_bits(valid + px, W, c0);
    if (!own) return;
    const unsigned ring = *(const unsigned *)(rings + px);
    // bits 0..2 of a ring byte point into row r - 1, bits 5..7 into row r + 1; bits 0, 3, 5 of pixel 0 at column c0 - 1, bits 2, 4, 7 of
    // pixel 3 at column c0 + 4.  A set bit is a vertex: inside the window, its position written
    const bool top = ring & 0x07070707u, bot = ring & 0xe0e0e0e0u;
    const float *p = src + 3 * px;
    float q[3][18];
    load_row6(p - 3 * (ptrdiff_t)pitch, top, ring & 0x01u, ring & 0x04000000u, q[0]);
    load_row6(p, true, ring & 0x08u, ring & 0x10000000u, q[1]);
    load_row6(p + 3 * (ptrdiff_t)pitch, bot, ring & 0x20u, ring & 0x80000000u, q[2]);
    float o[12];
    smooth_step(ring, q[0], q[1], q[2], f, o);
    float4 *d4 = (float4 *)(dst + 3 * px);
    d4[0] = make_float4(o[0], o[1], o[2], o[3]);
    d4[1] = make_float4(o[4], o[5], o[6], o[7]);
    d4[2] = make_float4(o[8], o[9], o[10], o[11]);
}

// grid (chunks of a row, H, views); counts / offsets: k_mesh_cells' and their scan; out: [view][out_stride][3] in vertex-id order
__global__ __launch_bounds__(256) void k_smooth_out(const uint8_t *__restrict__ valid, const float *__restrict__ plane, int W, int H, int pitch,
                                                    size_t view_stride, const unsigned *__restrict__ counts,
                                                    const unsigned long long *__restrict__ offsets, float *__restrict__ out, size_t out_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t chunk = ((size_t)blockIdx.z * H + r) * nck + blockIdx.x;
    const unsigned block_vertices = counts[chunk];
    if (block_vertices == 0) return;  // (the whole block: nothing to write)
    const size_t px = (size_t)blockIdx.z * view_stride + (size_t)r * pitch + c0;
    __shared__ unsigned s_wave[4];
    __shared__ float s_pts[3 * MESH_CHUNK];  // the block's points in output order
    const unsigned own = quad_bits(valid + px, W, c0);
    float q[12] = {};
    if (own) load_quad(plane + 3 * px, q);
    const unsigned cv = __popc(own);
    unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
    if (own) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (own >> k & 1u) {
                s_pts[3 * rank] = q[3 * k], s_pts[3 * rank + 1] = q[3 * k + 1], s_pts[3 * rank + 2] = q[3 * k + 2];
                rank++;
            }
    }
    __syncthreads();
    block_flush(out + 3 * ((size_t)blockIdx.z * out_stride + offsets[chunk]), s_pts, 3 * block_vertices);
}

// grid (chunks of a row, H, views); plane: the smoothed positions; normals: [view][normal_stride][3]
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_smooth_normals(
    const uint8_t *__restrict__ valid, const uint8_t *__restrict__ cells, const float *__restrict__ plane, int W, int H, int pitch, size_t view_stride,
    const unsigned *__restrict__ counts, const unsigned long long *__restrict__ offsets, float *__restrict__ normals, size_t normal_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t chunk = ((size_t)blockIdx.z * H + r) * nck + blockIdx.x;
    const unsigned block_vertices = counts[chunk];
    if (block_vertices == 0) return;  // (the whole block: nothing to write)
    const size_t px = (size_t)blockIdx.z * view_stride + (size_t)r * pitch + c0;
    __shared__ unsigned s_wave[4];
    __shared__ float s_n[3 * MESH_CHUNK];  // the block's normals in output order
    unsigned own = 0u;
    unsigned long long up = 0ull, mid = 0ull;
    if (c0 < W) {
        own = quad_bits(valid + px, W, c0);
        if (own) mid = cell_codes5(cells + px - c0, c0, true), up = cell_codes5(cells + px - c0 - pitch, c0, r > 0);
    }
    float n[4][3] = {};
    if (up | mid) {
        // the corners of the faces of the 10 cells: the points to load, row by row (a row none of them lies in is not read)
        const unsigned cu = smooth_row_corners(up), cm = smooth_row_corners(mid);
        const unsigned v[3] = {cu & 63u, (cu >> 8 | cm) & 63u, cm >> 8 & 63u};
        const float *p = plane + 3 * px;
        float q[3][18];
#pragma unroll
        for (int t = 0; t < 3; t++) load_row6(p + 3 * (ptrdiff_t)(t - 1) * pitch, v[t] & 30u, v[t] & 1u, v[t] & 32u, q[t]);
        double acc[12];
        smooth_quad_sums(up, mid, q[0], q[1], q[2], acc);
#pragma unroll
        for (int k = 0; k < 4; k++) mesh_normal_from_sum(&acc[3 * k], n[k]);
    }
    const unsigned cv = __popc(own);
    unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
    if (own) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (own >> k & 1u) {
                s_n[3 * rank] = n[k][0], s_n[3 * rank + 1] = n[k][1], s_n[3 * rank + 2] = n[k][2];
                rank++;
            }
    }
    __syncthreads();
    block_flush(normals + 3 * ((size_t)blockIdx.z * normal_stride + offsets[chunk]), s_n, 3 * block_vertices);
}

int launch_mesh_smooth(const KParams &P, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu, bool fix_boundary,
                       const SmoothBuffers &b, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(b.s, 1);
    const size_t v0 = L.v0;
    const unsigned *counts = c.cnt;
    const unsigned long long *offsets = c.off;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_mesh_cells(P, L, max_edge, b.cells, nullptr, nullptr, nullptr, c, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_smooth_ring, L.grid, dim3(256), 0, st, (const uint8_t *)(b.cells + v0), P.W, P.pitch, P.px_view_stride, (int)fix_boundary,
                       b.rings + v0);
    // step s reads what step s - 1 wrote (the first: the context's points) and writes plane s & 1; the plane the last step did not write
    // takes the compacted vertices
    const float *src = L.in.points;
    const int per = mu != 0.0f ? 2 : 1, steps = smooth_steps(iterations, mu);
    for (int s = 0; s < steps; s++) {
        float *dst = b.plane[s & 1] + 3 * v0;
        hipLaunchKernelGGL(k_smooth_step, L.grid, dim3(256), 0, st, L.in.valid, (const uint8_t *)(b.rings + v0), src, P.W, P.pitch, P.px_view_stride,
                           (double)(s % per ? mu : lambda), dst);
        src = dst;
    }
    hipLaunchKernelGGL(k_smooth_out, L.grid, dim3(256), 0, st, L.in.valid, src, P.W, P.H, P.pitch, P.px_view_stride, counts, offsets,
                       b.plane[steps & 1] + 3 * v0, P.px_view_stride);
    if (b.normals)
        hipLaunchKernelGGL(k_smooth_normals, L.grid, dim3(256), 0, st, L.in.valid, (const uint8_t *)(b.cells + v0), src, P.W, P.H, P.pitch,
                           P.px_view_stride, counts, offsets, b.normals + 3 * v0, P.px_view_stride);
    return (int)hipGetLastError();
}

}  // namespace sl3d
