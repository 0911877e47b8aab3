// sl3d_mesh_normals.hip -- vertex normals of the mesh sl3d_mesh_views defines (sl3d_mesh_normals; the definition and its arithmetic:
// sl3d_mesh.h).  A vertex's faces lie in the four cells around its pixel, so the normals are a gather over the organized grid:
//   k_mesh_normals_count : per chunk (1024 pixels of ONE row, the mesh kernels' chunk) its valid pixels
//   (k_compact_scan over the count array of every view: sl3d_clouds.hip)
//   k_mesh_normals       : a lane owns one quad of row r: valid bytes and points of rows r - 1, r, r + 1, columns c0 - 1 .. c0 + 4, the 10
//                          cells that touch its 4 pixels (mesh_quad_sums), 4 normals; the block's normals are contiguous in the output
//                          (vertex offset of the chunk + prefix within the chunk) and leave through LDS as one coalesced run
// No atomics, no adjacency lists, nothing read that sl3d_mesh_views wrote: the result follows from the planes and the scan alone, so it
// does not depend on the launch shape, the batch or the run.
// The scheme is the compaction's; its idioms -- valid-bit unpack, window clip, block sum, wave prefix, the waves in front, LDS flush --
// live in sl3d_block.h, the count kernel's quad_bits in sl3d_mesh_lane.h.  k_mesh_normals keeps its valid bits, its rows and its ordered
// output written out: load_row6, load_quad, a six-bit form of quad_bits and the output helper were each tried alone, each changes its
// instruction histogram, and none was measured (profiles/mesh_idioms_identity.txt).  What a launch starts from: mesh_launch
// (sl3d_internal.h).
#include <hip/hip_runtime.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh_lane.h"

namespace sl3d {

// grid (chunks of a row, H, views); counts: [view][H * chunks]
__global__ __launch_bounds__(256) void k_mesh_normals_count(const uint8_t *__restrict__ valid, int W, int pitch, size_t view_stride,
                                                            unsigned *__restrict__ counts)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    valid += (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    __shared__ unsigned s_cnt[4];
    unsigned c = __popc(quad_bits(valid + c0, W, c0));
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) counts[((size_t)blockIdx.z * gridDim.y + r) * nck + blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
}

// grid (chunks of a row, H, views); offsets: [view][H * chunks] exclusive scan of the counts; normals: [view][normal_stride][3]
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_mesh_normals(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                      size_t view_stride, double thr2, const unsigned *__restrict__ counts,
                                                      const unsigned long long *__restrict__ offsets, float *__restrict__ normals,
                                                      size_t normal_stride)
{
    const int r = blockIdx.y, nck = gridDim.x;
    const size_t chunk = ((size_t)blockIdx.z * H + r) * nck + blockIdx.x;
    const unsigned block_vertices = counts[chunk];
    if (block_vertices == 0) return;  // (the whole block: nothing to write)
    valid += (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    points += 3 * ((size_t)blockIdx.z * view_stride + (size_t)r * pitch);
    __shared__ unsigned s_wave[4];
    __shared__ float s_n[3 * MESH_CHUNK];  // the block's normals in output order
    const int c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const bool row[3] = {r > 0, true, r + 1 < H};
    unsigned v[3] = {0u, 0u, 0u};
    if (c0 < W) {
        const unsigned in_w = QUAD_IN_WINDOW(W, c0);
        const bool left = c0 > 0, right = c0 + 4 < W;
        // every valid byte the lane needs, requested before the first is looked at
        unsigned w[3], l[3], g[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const uint8_t *p = valid + (ptrdiff_t)(t - 1) * pitch + c0;
            w[t] = row[t] ? *(const unsigned *)p : 0u;
            l[t] = row[t] && left ? p[-1] : 0u;
            g[t] = row[t] && right ? p[4] : 0u;
        }
#pragma unroll
        for (int t = 0; t < 3; t++) v[t] = (l[t] & 1u) | (valid_nibble(w[t]) & in_w) << 1 | (g[t] & 1u) << 5;
    }
    const unsigned own = v[1] >> 1 & 15u;
    float n[4][3];
    if (own) {
        // columns c0 .. c0 + 3 of the three rows as 16-byte loads, the pixels left and right of them where they are valid (lines the
        // neighbouring lanes request anyway); a row outside the window or without a valid pixel among the 6 is not read
        float q[3][18];
        float4 f[3][3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const float4 *p = (const float4 *)(points + 3 * ((ptrdiff_t)(t - 1) * pitch + c0));
            f[t][0] = f[t][1] = f[t][2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (v[t]) f[t][0] = p[0], f[t][1] = p[1], f[t][2] = p[2];
        }
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const float *p = points + 3 * ((ptrdiff_t)(t - 1) * pitch + c0);
            const float m[12] = {f[t][0].x, f[t][0].y, f[t][0].z, f[t][0].w, f[t][1].x, f[t][1].y, f[t][1].z, f[t][1].w,
                                 f[t][2].x, f[t][2].y, f[t][2].z, f[t][2].w};
#pragma unroll
            for (int i = 0; i < 3; i++) q[t][i] = (v[t] & 1u) ? p[i - 3] : 0.0f;
#pragma unroll
            for (int i = 0; i < 12; i++) q[t][3 + i] = m[i];
#pragma unroll
            for (int i = 0; i < 3; i++) q[t][15 + i] = (v[t] & 32u) ? p[12 + i] : 0.0f;
        }
        double acc[12];
        mesh_quad_sums(v, q[0], q[1], q[2], thr2, acc);
#pragma unroll
        for (int k = 0; k < 4; k++) mesh_normal_from_sum(&acc[3 * k], n[k]);
    }
    // exclusive prefix of the lane's valid pixels over the block
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
    // the block's normals are contiguous in the output: coalesced dword stores
    block_flush(normals + 3 * ((size_t)blockIdx.z * normal_stride + offsets[chunk]), s_n, 3 * block_vertices);
}

int launch_mesh_normals(const KParams &P, int first_view, int n_views, float max_edge, const CompactScratch &s, float *normals,
                        size_t normal_stride, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(s, 1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mesh_normals_count, L.grid, dim3(256), 0, st, L.in.valid, P.W, P.pitch, P.px_view_stride, c.cnt);
    int rc = launch_compact_scan(c.cnt, c.off, L.n_chunks, n_views, c.tot, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mesh_normals, L.grid, dim3(256), 0, st, L.in.valid, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, mesh_thr2(max_edge),
                       (const unsigned *)c.cnt, (const unsigned long long *)c.off, normals + 3 * (size_t)first_view * normal_stride, normal_stride);
    return (int)hipGetLastError();
}

}  // namespace sl3d
