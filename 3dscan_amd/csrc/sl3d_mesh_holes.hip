// sl3d_mesh_holes.hip -- the small interior holes of a view's mesh, filled from their rims (sl3d_mesh_fill_holes; the definition:
// include/sl3d.h, the arithmetic and the union-find: sl3d_mesh_holes.h).  The filled grid is a dense result of its own -- valid / points
// planes with the geometry of the view's -- so what follows the fill are the launchers of the mesh over a KParams that carries it.  A fixed
// sequence of launches over the mesh kernels' chunks (1024 pixels of ONE row, a lane owning one quad); nothing in it depends on the data,
// no block waits for another, every loop over labels or pixels is bounded (a failure ends as a word the call reads back):
//   k_hole_init    : label of a non-candidate pixel = the first pixel of its row run inside the chunk (block max / min scans over the
//                    quads' candidate bits), or HOLE_OUTSIDE for a run that cannot belong to a hole: rows 0 / H-1, columns 0 / W-1, longer
//                    than max_hole.  Under a lasso the background is OUTSIDE from here on and costs the later passes one load per pixel
//   k_hole_union   : a run joins the run across the chunk seam and the runs it overlaps in the next row: atomic minima only
//   k_hole_flatten : every non-candidate pixel that is not OUTSIDE already looks its root up and stores it; the root's size grows by an
//                    integer atomic add
//   k_hole_fill    : candidates are copied bitwise; a pixel of a qualifying component walks to its rim over the candidate bytes, takes
//                    the four rim points and hole_position; the id plane gets the candidate's id in the view's compacted cloud or -1;
//                    holes (counted at their roots) and filled pixels are counted per chunk, k_compact_scan adds them up (atomic adds to
//                    one word per view cost the first form 150 us at 1080p: 16,000 adds to one address)
//   launch_compact_views, launch_mesh_views over the filled planes, launch_mesh_ids (k_lod_ids), launch_mesh_normals on request
// Between kernels plain loads read what the kernel before wrote; inside k_hole_union and k_hole_flatten, where other blocks write
// labels, every label access is an agent-scope relaxed atomic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh_holes.h"
#include "sl3d_mesh_lane.h"

namespace sl3d {

static_assert(MESH_CHUNK == 1024, "a chunk is one block of 256 quads");

// fail: one word per view, set when an iteration bound ran out
__device__ __forceinline__ void hole_record_failure(unsigned long long *fail)
{
    __hip_atomic_store(fail, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the 4 bytes of a quad of a 0/1 plane from its 4 bits
__device__ __forceinline__ unsigned nibble_bytes(unsigned b) { return (b & 1u) | (b & 2u) << 7 | (b & 4u) << 14 | (b & 8u) << 21; }

// grid (chunks of a row, H, views).  cand: [view][view_stride] 0/1 bytes; labels / sizes: [view][view_stride]
__global__ __launch_bounds__(256) void k_hole_init(const uint8_t *__restrict__ cand, int W, int H, int pitch, size_t view_stride, int max_hole,
                                                   int *__restrict__ labels, int *__restrict__ sizes)
{
    const int r = blockIdx.y, chunk0 = blockIdx.x * MESH_CHUNK, c0 = chunk0 + threadIdx.x * 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    __shared__ int s_max[4], s_min[4];
    // stops: the candidates of the quad and its pixels beyond the window -- what ends a run
    const unsigned in_w = c0 < W ? QUAD_IN_WINDOW(W, c0) : 0u;
    const unsigned stops = (quad_bits(cand + row + c0, W, c0) | ~in_w) & 15u;
    // the column behind the last stop at or in front of the lane's quad (inclusive maximum), the first stop at or behind it (minimum)
    const int own_after = stops ? c0 + 32 - __clz(stops) : chunk0, own_first = stops ? c0 + __ffs(stops) - 1 : chunk0 + MESH_CHUNK;
    int after = own_after, first = own_first;
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(after, off, 64), f = __shfl_down(first, off, 64);
        if (lane >= off) after = max(after, a);
        if (lane + off < 64) first = min(first, f);
    }
    if (lane == 63) s_max[wave] = after;
    if (lane == 0) s_min[wave] = first;
    __syncthreads();
    // exclusive: the lanes in front / behind, without the lane's own quad
    int before = __shfl_up(after, 1, 64), behind = __shfl_down(first, 1, 64);
    if (lane == 0) before = chunk0;
    if (lane == 63) behind = chunk0 + MESH_CHUNK;
    for (int i = 0; i < 4; i++) {
        if (i < wave) before = max(before, s_max[i]);
        if (i > wave) behind = min(behind, s_min[i]);
    }
    if (c0 >= pitch) return;
    int lab[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lab[k] = HOLE_NONE;
        if (stops >> k & 1u) continue;
        const unsigned lo = stops & ((1u << k) - 1u), hi = stops >> (k + 1);
        const int s = lo ? c0 + 32 - __clz(lo) : before, e = hi ? c0 + k + __ffs(hi) : behind;  // the run [s, e) of pixel c0 + k inside the chunk
        lab[k] = hole_run_outside(r, s, e, W, H, max_hole) ? HOLE_OUTSIDE : r * pitch + s;
    }
    *(int4 *)(labels + row + c0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
    *(int4 *)(sizes + row + c0) = make_int4(0, 0, 0, 0);
}

// grid (chunks of a row, H, views); bound: the iteration bound of every label walk
__global__ __launch_bounds__(256) void k_hole_union(const uint8_t *__restrict__ cand, int W, int H, int pitch, size_t view_stride, int bound, int *labels,
                                                    unsigned long long *fail)
{
    const int r = blockIdx.y, chunk0 = blockIdx.x * MESH_CHUNK, c0 = chunk0 + threadIdx.x * 4;
    if (c0 >= W) return;
    const uint8_t *row = cand + (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    const unsigned in_w = QUAD_IN_WINDOW(W, c0);
    const bool next_row = r + 1 < H;
    // non-candidates of pixels c0 - 1 .. c0 + 3 of rows r and r + 1 as bits 0 .. 4 (0 beyond the window)
    unsigned n0 = (~quad_bits(row + c0, W, c0) & in_w) << 1, n1 = next_row ? (~quad_bits(row + pitch + c0, W, c0) & in_w) << 1 : 0u;
    if (!n0) return;
    if (c0 > 0) {
        n0 |= ~row[c0 - 1] & 1u;
        if (next_row) n1 |= ~row[pitch + c0 - 1] & 1u;
    }
    labels += (size_t)blockIdx.z * view_stride;
    int failed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (failed || !(n0 >> (k + 1) & 1u)) continue;
        hole_pixel_unions(labels, r * pitch + c0 + k, pitch, k == 0 && c0 == chunk0 && c0 > 0, n0 >> k & 1u, n1 >> (k + 1) & 1u, n1 >> k & 1u, bound, &failed);
    }
    if (failed) hole_record_failure(fail + blockIdx.z);
}

// grid (chunks of a row, H, views)
__global__ __launch_bounds__(256) void k_hole_flatten(const uint8_t *__restrict__ cand, int W, int pitch, size_t view_stride, int bound, int *labels, int *sizes,
                                                      unsigned long long *fail)
{
    const int r = blockIdx.y, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    if (c0 >= W) return;
    const size_t view = (size_t)blockIdx.z * view_stride;
    const unsigned nc = ~quad_bits(cand + view + (size_t)r * pitch + c0, W, c0) & QUAD_IN_WINDOW(W, c0);
    if (!nc) return;
    labels += view, sizes += view;
    const int p = r * pitch + c0;
    // what the union kernel left (a plain load: whatever another block lowers meanwhile is lowered to an ancestor, and OUTSIDE is final)
    const int4 l = *(const int4 *)(labels + p);
    const int seen[4] = {l.x, l.y, l.z, l.w};
    int failed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (failed || !(nc >> k & 1u) || seen[k] == HOLE_OUTSIDE) continue;  // (the background: nothing to look up, nothing to store)
        const int root = hole_find(labels, p + k, bound, &failed);
        if (failed) break;
        if (root != p + k) CC_FETCH_MIN(labels + p + k, root);
        if (root != HOLE_OUTSIDE) atomicAdd(sizes + root, 1);
    }
    if (failed) hole_record_failure(fail + blockIdx.z);
}

// grid (chunks of a row, H, views).  offsets: [view][H * chunks] exclusive scan of the valid pixels per chunk (the candidates are the
// valid pixels), or NULL: vid, [view][view_stride], holds the id of every candidate.  walk: the bound of a rim walk.  valid_f / ids_f [view][view_stride], points_f
// [view][view_stride][3]: the filled grid; counts: [view][2][H * chunks]: holes (counted at their roots), filled pixels
__global__ __launch_bounds__(256) void k_hole_fill(const uint8_t *__restrict__ cand, const float *__restrict__ points, int W, int H, int pitch,
                                                   size_t view_stride, int max_hole, int walk, float fill_edge, const int *__restrict__ labels,
                                                   const int *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                   const int *__restrict__ vid, uint8_t *__restrict__ valid_f, float *__restrict__ points_f,
                                                   int *__restrict__ ids_f, unsigned *__restrict__ counts, unsigned long long *fail)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t view = (size_t)blockIdx.z * view_stride, row = view + (size_t)r * pitch;
    __shared__ unsigned s_wave[4], s_cnt[4];
    const unsigned in_w = c0 < W ? QUAD_IN_WINDOW(W, c0) : 0u;
    const unsigned cb = quad_bits(cand + row + c0, W, c0), nc = ~cb & in_w;
    // the candidates of the chunk in front of the quad: their ids follow from the chunk's offset
    const unsigned cv = __popc(cb);
    const unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
    float q[12] = {};
    int id[4] = {-1, -1, -1, -1};
    if (cb) {
        load_quad(points + 3 * (row + c0), q);
        if (offsets) {
            const int id0 = (int)offsets[((size_t)blockIdx.z * H + r) * nck + blockIdx.x] + (int)rank;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (cb >> k & 1u) id[k] = id0 + (int)__popc(cb & ((1u << k) - 1u));
        } else {
            const int4 o = *(const int4 *)(vid + row + c0);
            const int orig[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (cb >> k & 1u) id[k] = orig[k];
        }
    }
    unsigned fb = 0u, holes = 0u;
    if (nc) {
        const int4 l = *(const int4 *)(labels + row + c0);
        const int root[4] = {l.x, l.y, l.z, l.w};
        int failed = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!(nc >> k & 1u) || root[k] == HOLE_OUTSIDE) continue;
            if (!hole_qualifies(root[k], sizes[view + root[k]], max_hole)) continue;
            holes += root[k] == r * pitch + c0 + k;
            float o[3] = {0.0f, 0.0f, 0.0f};
            if (hole_fill_pixel(cand + view, points + 3 * view, r, c0 + k, W, H, pitch, walk, fill_edge, o, &failed)) {
                fb |= 1u << k;
                q[3 * k] = o[0], q[3 * k + 1] = o[1], q[3 * k + 2] = o[2];
            }
        }
        if (failed) hole_record_failure(fail + blockIdx.z);
    }
    if (c0 < pitch) {  // (the quad lies inside the pitch: a multiple of 16; a point under an invalid pixel of the filled grid is 0)
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (!((cb | fb) >> k & 1u)) q[3 * k] = q[3 * k + 1] = q[3 * k + 2] = 0.0f;
        *(unsigned *)(valid_f + row + c0) = nibble_bytes(cb | fb);
        float4 *o4 = (float4 *)(points_f + 3 * (row + c0));
        o4[0] = make_float4(q[0], q[1], q[2], q[3]), o4[1] = make_float4(q[4], q[5], q[6], q[7]), o4[2] = make_float4(q[8], q[9], q[10], q[11]);
        *(int4 *)(ids_f + row + c0) = make_int4(id[0], id[1], id[2], id[3]);
    }
    // holes and filled pixels of the chunk in one word: at most 1024 of either
    unsigned c = holes | (unsigned)__popc(fb) << 16;
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) {
        const unsigned t = BLOCK_SUM_TOTAL(s_cnt);
        const int n_chunks = H * nck, chunk = r * nck + blockIdx.x;
        counts += (size_t)blockIdx.z * 2 * n_chunks;
        counts[chunk] = t & 0xffffu;
        counts[n_chunks + chunk] = t >> 16;
    }
}

int launch_mesh_holes(const KParams &P, const KParams &F, int first_view, int n_views, float max_edge, int max_hole, float fill_edge, const LodSource &src,
                      const HoleBuffers &b, bool normals, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const size_t v0 = L.v0;
    const int bound = (int)P.px_view_stride;
    const int walk = std::min(max_hole, std::max(P.W, P.H));
    unsigned long long *fail = b.failed + first_view;
    const CompactScratch hc = L.sliced(b.hol, 2);
    hipStream_t st = (hipStream_t)stream;
    int rc = (int)hipMemsetAsync(fail, 0, sizeof(unsigned long long) * (size_t)n_views, st);
    if (rc) return rc;
    const uint8_t *cand = src.cand + v0;
    hipLaunchKernelGGL(k_hole_init, L.grid, dim3(256), 0, st, cand, P.W, P.H, P.pitch, P.px_view_stride, max_hole, b.labels + v0, b.sizes + v0);
    hipLaunchKernelGGL(k_hole_union, L.grid, dim3(256), 0, st, cand, P.W, P.H, P.pitch, P.px_view_stride, bound, b.labels + v0, fail);
    hipLaunchKernelGGL(k_hole_flatten, L.grid, dim3(256), 0, st, cand, P.W, P.pitch, P.px_view_stride, bound, b.labels + v0, b.sizes + v0, fail);
    hipLaunchKernelGGL(k_hole_fill, L.grid, dim3(256), 0, st, cand, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, max_hole, walk, fill_edge,
                       (const int *)(b.labels + v0), (const int *)(b.sizes + v0), src.offsets, src.vid ? src.vid + v0 : nullptr, F.valid + v0,
                       F.points + 3 * v0, b.ids + v0, hc.cnt, fail);
    rc = launch_compact_scan(hc.cnt, hc.off, L.n_chunks, 2 * n_views, hc.tot, stream);
    if (!rc) rc = launch_compact_views(F, first_view, n_views, b.blk, b.xyz + 3 * v0, nullptr, nullptr, stream);
    if (!rc) rc = launch_mesh_views(F, first_view, n_views, max_edge, b.chk, b.faces, b.face_stride, stream);
    if (!rc) rc = launch_mesh_ids(F, first_view, n_views, b.chk, b.ids, b.vertex_ids, stream);
    if (!rc && normals) rc = launch_mesh_normals(F, first_view, n_views, max_edge, b.nrm, b.normals, F.px_view_stride, stream);
    return rc;
}

}  // namespace sl3d
