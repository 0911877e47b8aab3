// sl3d_mesh_components.hip -- the connected components of the mesh sl3d_mesh_views defines, and that mesh without its small components
// (sl3d_mesh_components / sl3d_mesh_views_filtered; the definition and the union-find: sl3d_mesh_components.h; the cell plane: sl3d_mesh.h).
// A fixed sequence of launches over the mesh kernels' chunks (1024 pixels of ONE row, a lane owning one quad); nothing in it depends on
// the data, no block waits for another, and every loop over labels is bounded (a failure ends as a word the call reads back):
//   k_mesh_cells_uf and k_compact_scan over the count array of every view (launch_mesh_cells, sl3d_mesh.hip): the cell plane; label of a
//                  pixel = its own index, size = 0; per chunk its valid pixels and their scan
//   k_cc_union   : every cell with a face joins its corners -- a lock-free union-find on the label plane, atomic minima only
//   k_cc_flatten : every valid pixel looks its root up and stores it; vertex id of the pixel (chunk offset + prefix) into the id plane;
//                  the roots are counted and every root's size summed, both by integer atomic adds aggregated per wave first
//   k_cc_labels  : label of a vertex = the vertex id of its root, staged per chunk and written as one coalesced run
// and for the filtered mesh, behind k_cc_flatten:
//   k_cc_keep    : keep byte of a pixel = its root's size >= min_vertices; per chunk the kept vertices and the kept faces (a face goes
//                  with its first corner, cc_face_kept)
//   (k_compact_scan over the 2 count arrays of every view)
//   k_cc_emit    : kept points, their original ids and the kept faces with the new ids, ranked by wave prefixes, staged in LDS in output
//                  order and flushed -- k_mesh_emit's scheme with keep bytes for valid bytes and the cell plane for the doubles
// Between kernels plain loads read what the kernel before wrote; inside k_cc_union and k_cc_flatten, where other blocks write labels,
// every label access is an agent-scope relaxed atomic (CC_LOAD / CC_FETCH_MIN).  What a caller sees -- labels, counts, kept ids, faces --
// is fixed by the definition: the atomics only decide who does which part of the work.
// The block idioms live in sl3d_block.h, a lane's loads, cells and staged faces in sl3d_mesh_lane.h.
#include <hip/hip_runtime.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh_components.h"
#include "sl3d_mesh_lane.h"

namespace sl3d {

__device__ __forceinline__ void cc_record_failure(unsigned long long *stat)
{
    __hip_atomic_store(stat + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (chunks of a row, H - 1, views); bound: the iteration bound of every label walk
__global__ __launch_bounds__(256) void k_cc_union(const uint8_t *__restrict__ cells, int W, int pitch, size_t view_stride, int bound, int *labels,
                                                  unsigned long long *stat)
{
    const int r = blockIdx.y, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    if (c0 >= W) return;
    const unsigned codes = *(const unsigned *)(cells + (size_t)blockIdx.z * view_stride + (size_t)r * pitch + c0);
    if (!codes) return;
    labels += (size_t)blockIdx.z * view_stride;
    int failed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (failed) break;
        cc_cell_unions(labels, codes >> (8 * k) & 255u, r * pitch + c0 + k, pitch, bound, &failed);
    }
    if (failed) cc_record_failure(stat + 2 * blockIdx.z);
}

// grid (chunks of a row, H, views); offsets: [view][H * chunks] exclusive scan of k_mesh_cells' counts; vid: [view][view_stride] vertex ids
// (-1 under an invalid pixel)
__global__ __launch_bounds__(256) void k_cc_flatten(const uint8_t *__restrict__ valid, int W, int H, int pitch, size_t view_stride, int bound,
                                                    const unsigned long long *__restrict__ offsets, int *labels, int *__restrict__ vid, int *sizes,
                                                    unsigned long long *stat)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    labels += (size_t)blockIdx.z * view_stride;
    sizes += (size_t)blockIdx.z * view_stride;
    stat += 2 * blockIdx.z;
    __shared__ unsigned s_wave[4];
    const unsigned own = quad_bits(valid + row + c0, W, c0);
    const int p = r * pitch + c0;
    // the roots of the lane's pixels, stored (a minimum like every other write: the root is not above what stands there)
    int root[4] = {-1, -1, -1, -1}, failed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((own >> k & 1u) && !failed) {
            root[k] = cc_find(labels, p + k, bound, &failed);
            if (!failed && root[k] != p + k) CC_FETCH_MIN(labels + p + k, root[k]);
        }
    if (failed) cc_record_failure(stat);
    // vertex ids: the chunk's offset + the valid pixels of the chunk in front
    const unsigned cv = __popc(own);
    const unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
    if (c0 < W) {
        const int id0 = (int)offsets[((size_t)blockIdx.z * H + r) * nck + blockIdx.x] + (int)rank;
        int id[4];
#pragma unroll
        for (int k = 0; k < 4; k++) id[k] = (own >> k & 1u) ? id0 + (int)__popc(own & ((1u << k) - 1u)) : -1;
        *(int4 *)(vid + row + c0) = make_int4(id[0], id[1], id[2], id[3]);
    }
    // roots and sizes: integer adds, aggregated per wave first.  Pixel k of every lane in turn: the lanes whose root is that of the
    // first lane with a pixel go out as ONE add (a large component: all of them), whoever differs adds for itself
    unsigned roots = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool has = root[k] >= 0 && !failed;
        roots += has && root[k] == p + k;
        const unsigned long long m = __ballot(has);
        if (!m) continue;  // (wave-uniform)
        const int lead = __ffsll((long long)m) - 1, r0 = __shfl(root[k], lead, 64);
        const unsigned n = (unsigned)__popcll(__ballot(has && root[k] == r0));
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(sizes + r0, (int)n);
        else if (has && root[k] != r0) atomicAdd(sizes + root[k], 1);
    }
    roots = wave_sum(roots);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(stat, (unsigned long long)roots);
}

// grid (chunks of a row, H, views); counts / offsets: k_mesh_cells' and their scan; out: [view][out_stride] labels in vertex-id order
__global__ __launch_bounds__(256) void k_cc_labels(const uint8_t *__restrict__ valid, int W, int H, int pitch, size_t view_stride,
                                                   const unsigned *__restrict__ counts, const unsigned long long *__restrict__ offsets,
                                                   const int *__restrict__ labels, const int *__restrict__ vid, int *__restrict__ out, size_t out_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t chunk = ((size_t)blockIdx.z * H + r) * nck + blockIdx.x;
    const unsigned block_vertices = counts[chunk];
    if (block_vertices == 0) return;  // (the whole block: nothing to write)
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    vid += (size_t)blockIdx.z * view_stride;
    __shared__ unsigned s_wave[4];
    __shared__ int s_lab[MESH_CHUNK];  // the block's labels in output order
    const unsigned own = quad_bits(valid + row + c0, W, c0);
    int lab[4] = {0, 0, 0, 0};
    if (own) {
        const int4 l = *(const int4 *)(labels + row + c0);
        const int root[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (own >> k & 1u) lab[k] = vid[root[k]];
    }
    const unsigned cv = __popc(own);
    unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (own >> k & 1u) s_lab[rank++] = lab[k];
    __syncthreads();
    block_flush(out + (size_t)blockIdx.z * out_stride + offsets[chunk], s_lab, block_vertices);
}

// the faces of the lane's 4 cells that survive: kb = keep bits of pixels c0 .. c0 + 4 of the cells' upper row; n[k] = kept faces of cell k
// (bit f of keep[k]: face f is kept)
__device__ __forceinline__ unsigned cc_kept_faces(unsigned codes, unsigned kb, unsigned cell[4], unsigned keep[4])
{
    unsigned n = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cell[k] = cc_code_cell(codes >> (8 * k) & 255u);
        keep[k] = 0u;
#pragma unroll
        for (int f = 0; f < 2; f++)
            if ((int)(cell[k] & 3u) > f && cc_face_kept(cell[k], f, kb >> k & 1u, kb >> (k + 1) & 1u)) keep[k] |= 1u << f, n++;
    }
    return n;
}

// grid (chunks of a row, H, views); keep: [view][view_stride] 0/1 bytes; counts: [view][2][H * chunks]: kept vertices, kept faces
__global__ __launch_bounds__(256) void k_cc_keep(const uint8_t *__restrict__ valid, const uint8_t *__restrict__ cells, int W, int H, int pitch,
                                                 size_t view_stride, const int *__restrict__ labels, const int *__restrict__ sizes, int min_vertices,
                                                 uint8_t *__restrict__ keep, unsigned *__restrict__ counts)
{
    const int r = blockIdx.y, nck = gridDim.x, chunk = r * nck + blockIdx.x, n_chunks = H * nck, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    sizes += (size_t)blockIdx.z * view_stride;
    counts += (size_t)blockIdx.z * 2 * n_chunks;
    __shared__ unsigned s_cnt[4];
    const unsigned own = quad_bits(valid + row + c0, W, c0);
    unsigned kb = 0u, nf = 0u;
    if (c0 < W) {
        const unsigned codes = *(const unsigned *)(cells + row + c0);
        if (own) {
            const int4 l = *(const int4 *)(labels + row + c0);
            const int root[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((own >> k & 1u) && sizes[root[k]] >= min_vertices) kb |= 1u << k;
        }
        *(unsigned *)(keep + row + c0) = (kb & 1u) | (kb & 2u) << 7 | (kb & 4u) << 14 | (kb & 8u) << 21;
        // the last cell's faces that start at b go with the pixel right of the quad (valid: it is a corner of a face)
        const unsigned last = codes >> 24;
        if (last == 4u || last == 6u) kb |= (unsigned)(sizes[labels[row + c0 + 4]] >= min_vertices) << 4;
        unsigned cell[4], fk[4];
        nf = cc_kept_faces(codes, kb, cell, fk);
    }
    // both counts in one word: at most 1024 pixels and 2048 faces per chunk
    unsigned c = __popc(kb & 15u) | nf << 16;
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) {
        const unsigned t = BLOCK_SUM_TOTAL(s_cnt);
        counts[chunk] = t & 0xffffu;
        counts[n_chunks + chunk] = t >> 16;
    }
}

// grid (chunks of a row, H, views); counts / offsets: k_cc_keep's and their scan; xyz: [view][point_stride][3], ids: [view][point_stride],
// faces: [view][face_stride][3]
__global__ __launch_bounds__(256) void k_cc_emit(const uint8_t *__restrict__ keep, const uint8_t *__restrict__ cells, const float *__restrict__ points,
                                                 const int *__restrict__ vid, int W, int H, int pitch, size_t view_stride,
                                                 const unsigned *__restrict__ counts, const unsigned long long *__restrict__ offsets,
                                                 float *__restrict__ xyz, int *__restrict__ ids, size_t point_stride, int *__restrict__ faces,
                                                 size_t face_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, chunk = r * nck + blockIdx.x, n_chunks = H * nck, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    counts += (size_t)blockIdx.z * 2 * n_chunks;
    const unsigned block_vertices = counts[chunk], block_faces = counts[n_chunks + chunk];
    if (block_vertices == 0 && block_faces == 0) return;  // (the whole block; a face may hang on the next chunk's first pixel alone)
    offsets += (size_t)blockIdx.z * 2 * n_chunks;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    __shared__ unsigned s_wave_v[4], s_wave_f[4];
    __shared__ float s_pts[3 * MESH_CHUNK];      // the block's kept points,
    __shared__ int s_ids[MESH_CHUNK];            // their original ids
    __shared__ int s_faces[2 * MESH_CHUNK * 3];  // and its kept faces, all in output order
    const bool next_row = r + 1 < H;
    const unsigned k0 = quad_bits5(keep + row, W, c0, true), k1 = quad_bits5(keep + row + pitch, W, c0, next_row);
    unsigned cell[4] = {0u, 0u, 0u, 0u}, fk[4] = {0u, 0u, 0u, 0u}, cf = 0u;
    if (c0 < W && block_faces) cf = cc_kept_faces(*(const unsigned *)(cells + row + c0), k0, cell, fk);
    // exclusive prefixes over the block: kept pixels of row r (low half) and of row r + 1 (high half) in one word, faces in another
    const unsigned cv = __popc(k0 & 15u) | __popc(k1 & 15u) << 16;
    const unsigned ev = waves_before(s_wave_v, wave_prefix(cv, s_wave_v) - cv);
    unsigned rank_f = waves_before(s_wave_f, wave_prefix(cf, s_wave_f) - cf);
    if (k0 & 15u) {
        float q[12];
        load_quad(points + 3 * (row + c0), q);
        const int4 o = *(const int4 *)(vid + row + c0);
        const int orig[4] = {o.x, o.y, o.z, o.w};
        unsigned rank_v = ev & 0xffffu;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k0 >> k & 1u) {
                s_pts[3 * rank_v] = q[3 * k], s_pts[3 * rank_v + 1] = q[3 * k + 1], s_pts[3 * rank_v + 2] = q[3 * k + 2];
                s_ids[rank_v] = orig[k];
                rank_v++;
            }
    }
    // new ids of pixels c0 .. c0 + 4 of both rows: the chunk's offset + the kept pixels of the chunk in front (the pixel right of the
    // block's last quad is the next chunk's first: the same expression)
    if (cf) stage_faces<false>((int)offsets[chunk] + (int)(ev & 0xffffu), (int)offsets[chunk + nck] + (int)(ev >> 16), k0, k1, cell, fk, rank_f, s_faces);
    __syncthreads();
    // the block's points, ids and faces are contiguous in the output: coalesced dword stores
    const size_t at = (size_t)blockIdx.z * point_stride + offsets[chunk];
    block_flush(xyz + 3 * at, s_pts, 3 * block_vertices);
    block_flush(ids + at, s_ids, block_vertices);
    block_flush(faces + 3 * ((size_t)blockIdx.z * face_stride + offsets[n_chunks + chunk]), s_faces, 3 * block_faces);
}

// labels (buffers.labels_out != nullptr) or the state the filter starts from
int launch_mesh_components(const KParams &P, int first_view, int n_views, float max_edge, const CcBuffers &b, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(b.s, 1);
    const int bound = (int)P.px_view_stride;
    const size_t v0 = L.v0;
    unsigned long long *stat = b.stat + 2 * (size_t)first_view;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_mesh_cells(P, L, max_edge, b.cells, b.labels, b.sizes, stat, c, stream);
    if (rc) return rc;
    if (P.H > 1)
        hipLaunchKernelGGL(k_cc_union, dim3(L.nck, P.H - 1, n_views), dim3(256), 0, st, (const uint8_t *)(b.cells + v0), P.W, P.pitch, P.px_view_stride, bound,
                           b.labels + v0, stat);
    hipLaunchKernelGGL(k_cc_flatten, L.grid, dim3(256), 0, st, L.in.valid, P.W, P.H, P.pitch, P.px_view_stride, bound, (const unsigned long long *)c.off,
                       b.labels + v0, b.vid + v0, b.sizes + v0, stat);
    if (b.labels_out)
        hipLaunchKernelGGL(k_cc_labels, L.grid, dim3(256), 0, st, L.in.valid, P.W, P.H, P.pitch, P.px_view_stride, (const unsigned *)c.cnt,
                           (const unsigned long long *)c.off, (const int *)(b.labels + v0), (const int *)(b.vid + v0), b.labels_out + v0, P.px_view_stride);
    return (int)hipGetLastError();
}

// behind launch_mesh_components over the same views: the keep bytes and their counts (all the level-of-detail call wants of the filter)
int launch_mesh_keep(const KParams &P, int first_view, int n_views, int min_vertices, const CcBuffers &b, const CcFiltered &f, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(f.s, 2);
    const size_t v0 = L.v0;
    hipLaunchKernelGGL(k_cc_keep, L.grid, dim3(256), 0, (hipStream_t)stream, L.in.valid, (const uint8_t *)(b.cells + v0), P.W, P.H, P.pitch,
                       P.px_view_stride, (const int *)(b.labels + v0), (const int *)(b.sizes + v0), min_vertices, f.keep + v0, c.cnt);
    return (int)hipGetLastError();
}

// behind launch_mesh_components over the same views
int launch_mesh_filter(const KParams &P, int first_view, int n_views, int min_vertices, const CcBuffers &b, const CcFiltered &f, void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(f.s, 2);
    const size_t v0 = L.v0;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_mesh_keep(P, first_view, n_views, min_vertices, b, f, stream);
    if (!rc) rc = launch_compact_scan(c.cnt, c.off, L.n_chunks, 2 * n_views, c.tot, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cc_emit, L.grid, dim3(256), 0, st, (const uint8_t *)(f.keep + v0), (const uint8_t *)(b.cells + v0), L.in.points, (const int *)(b.vid + v0),
                       P.W, P.H, P.pitch, P.px_view_stride, (const unsigned *)c.cnt, (const unsigned long long *)c.off, f.xyz + 3 * v0, f.ids + v0,
                       P.px_view_stride, f.faces + 3 * (size_t)first_view * f.face_stride, f.face_stride);
    return (int)hipGetLastError();
}

}  // namespace sl3d
