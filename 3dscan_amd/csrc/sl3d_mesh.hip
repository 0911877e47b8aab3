// sl3d_mesh.hip -- the mesh stage: ordered triangles over the organized point grid of a dense result (sl3d_mesh_views; the
// definition and its arithmetic: sl3d_mesh.h).  The vertices are the compacted cloud launch_compact_views writes; this unit adds
//   k_mesh_count : per chunk (1024 pixels of ONE row) the valid pixels of the chunk and the faces of the cells whose corner a lies in it
//   (k_compact_scan over the 2 count arrays of every view: sl3d_clouds.hip)
//   k_mesh_emit  : the same cells again, every face ranked by wave prefixes and written at face_offset[chunk] + rank
// A lane owns one quad of row r -- 4 cells: its own 4 pixels of rows r and r + 1 (one dword of valid bytes and three 16-byte loads of
// points per row) and the pixel right of them (the corners b / e of its last cell), which the neighbouring lane has requested too: those
// loads hit the cache the neighbour's lines are in.  No index plane: the vertex id of a pixel is its chunk's offset plus the valid
// pixels of the chunk in front of it, for row r + 1 from ITS chunk's offset -- both are prefixes over bytes the block holds anyway.
// No atomics: every output position follows from the scans, so the result does not depend on the launch shape, the batch or the run.
// The scheme is the compaction's; its idioms -- valid-bit unpack, window clip, block sum, LDS flush -- live in sl3d_block.h.  Written
// out here: the two-word wave prefix of k_mesh_emit (vertices and faces in one shuffle loop).  A lane's loads, cells and staged faces:
// mesh_lane, stage_faces (sl3d_mesh_lane.h).  Chunks per row: mesh_row_chunks; what a launch starts from: mesh_launch (sl3d_internal.h).
// Also here, with mesh_lane's other users: k_mesh_cells / k_mesh_cells_uf, the cell pass the components and the smoothing calls start with
// (launch_mesh_cells) -- mesh_cell of every cell ONCE, left as a byte per cell (cc_cell_code, sl3d_mesh.h), and per chunk its valid pixels.
#include <hip/hip_runtime.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh.h"
#include "sl3d_mesh_lane.h"

namespace sl3d {

// grid (chunks of a row, H, views); counts: [view][2][H * chunks]: valid pixels, faces
__global__ __launch_bounds__(256) void k_mesh_count(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                    size_t view_stride, double thr2, unsigned *__restrict__ counts)
{
    const int r = blockIdx.y, nck = gridDim.x, chunk = r * nck + blockIdx.x, n_chunks = H * nck;
    valid += (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    points += 3 * ((size_t)blockIdx.z * view_stride + (size_t)r * pitch);
    counts += (size_t)blockIdx.z * 2 * n_chunks;
    __shared__ unsigned s_cnt[4];
    unsigned v0, v1, cell[4];
    mesh_lane(valid, points, W, pitch, blockIdx.x * MESH_CHUNK + threadIdx.x * 4, r + 1 < H, thr2, v0, v1, cell);
    // both counts in one word: at most 1024 pixels and 2048 faces per chunk
    unsigned c = __popc(v0 & 15u) | ((cell[0] & 3u) + (cell[1] & 3u) + (cell[2] & 3u) + (cell[3] & 3u)) << 16;
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) {
        const unsigned t = BLOCK_SUM_TOTAL(s_cnt);
        counts[chunk] = t & 0xffffu;
        counts[n_chunks + chunk] = t >> 16;
    }
}

// grid (chunks of a row, H - 1, views); offsets: [view][2][H * chunks] exclusive scans of the counts; faces: [view][face_stride][3]
__global__ __launch_bounds__(256) void k_mesh_emit(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                   size_t view_stride, double thr2, const unsigned *__restrict__ counts,
                                                   const unsigned long long *__restrict__ offsets, int *__restrict__ faces, size_t face_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, chunk = r * nck + blockIdx.x, n_chunks = H * nck;
    counts += (size_t)blockIdx.z * 2 * n_chunks;
    if (counts[n_chunks + chunk] == 0) return;  // (the whole block: nothing to write)
    valid += (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    points += 3 * ((size_t)blockIdx.z * view_stride + (size_t)r * pitch);
    offsets += (size_t)blockIdx.z * 2 * n_chunks;
    faces += 3 * (size_t)blockIdx.z * face_stride;
    __shared__ unsigned s_wave_v[4], s_wave_f[4];
    __shared__ int s_faces[2 * MESH_CHUNK * 3];  // the block's faces in output order
    unsigned v0, v1, cell[4];
    mesh_lane(valid, points, W, pitch, blockIdx.x * MESH_CHUNK + threadIdx.x * 4, true, thr2, v0, v1, cell);
    // exclusive prefixes over the block: valid pixels of row r (low half) and of row r + 1 (high half) in one word, faces in another
    const unsigned cv = __popc(v0 & 15u) | __popc(v1 & 15u) << 16;
    const unsigned cf = (cell[0] & 3u) + (cell[1] & 3u) + (cell[2] & 3u) + (cell[3] & 3u);
    unsigned iv = cv, jf = cf;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned tv = __shfl_up(iv, off, 64), tf = __shfl_up(jf, off, 64);
        if ((threadIdx.x & 63) >= off) iv += tv, jf += tf;
    }
    if ((threadIdx.x & 63) == 63) s_wave_v[threadIdx.x >> 6] = iv, s_wave_f[threadIdx.x >> 6] = jf;
    __syncthreads();
    unsigned base_v = 0, base_f = 0;
    for (int i = 0; i < (int)(threadIdx.x >> 6); i++) base_v += s_wave_v[i], base_f += s_wave_f[i];
    const unsigned block_faces = BLOCK_SUM_TOTAL(s_wave_f);
    if (cf) {
        const unsigned ev = base_v + (iv - cv);
        // vertex ids of pixels c0 .. c0 + 4 of both rows; the pixel right of the block's last quad is the next chunk's first, whose
        // offset is this chunk's offset plus this chunk's count: the same expression
        stage_faces<true>((int)offsets[chunk] + (int)(ev & 0xffffu), (int)offsets[chunk + nck] + (int)(ev >> 16), v0, v1, cell, nullptr, base_f + (jf - cf), s_faces);
    }
    __syncthreads();
    // the block's faces are contiguous in the output: coalesced dword stores
    block_flush(faces + 3 * offsets[n_chunks + chunk], s_faces, 3 * block_faces);
}

// The cell pass.  grid (chunks of a row, H, views); cells: [view][view_stride]; counts: [view][H * chunks].  UNION_FIND: also labels / sizes,
// [view][view_stride] planes, initialised here, and stat, [view][2] {roots, failure}, zeroed here for the kernels behind
template <bool UNION_FIND>
__device__ __forceinline__ void mesh_cells(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch, size_t view_stride,
                                           double thr2, uint8_t *__restrict__ cells, int *__restrict__ labels, int *__restrict__ sizes,
                                           unsigned *__restrict__ counts, unsigned long long *__restrict__ stat)
{
    const int r = blockIdx.y, nck = gridDim.x, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    const size_t row = (size_t)blockIdx.z * view_stride + (size_t)r * pitch;
    __shared__ unsigned s_cnt[4];
    unsigned v0, v1, cell[4];
    mesh_lane(valid + row, points + 3 * row, W, pitch, c0, r + 1 < H, thr2, v0, v1, cell);
    if (c0 < W) {  // (the quad lies inside the pitch: a multiple of 16)
        *(unsigned *)(cells + row + c0) = cell_codes(cell);
        if (UNION_FIND) {
            const int p = r * pitch + c0;
            *(int4 *)(labels + row + c0) = make_int4(p, p + 1, p + 2, p + 3);
            *(int4 *)(sizes + row + c0) = make_int4(0, 0, 0, 0);
        }
    }
    if (UNION_FIND && blockIdx.x == 0 && r == 0 && threadIdx.x == 0) stat[2 * blockIdx.z] = stat[2 * blockIdx.z + 1] = 0ull;
    unsigned c = __popc(v0 & 15u);
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) counts[((size_t)blockIdx.z * H + r) * nck + blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
}
// (two argument lists over one body: with the union-find's three pointers in its list the plain kernel loads its arguments differently)
__global__ __launch_bounds__(256) void k_mesh_cells(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                    size_t view_stride, double thr2, uint8_t *__restrict__ cells, unsigned *__restrict__ counts)
{
    mesh_cells<false>(valid, points, W, H, pitch, view_stride, thr2, cells, nullptr, nullptr, counts, nullptr);
}
__global__ __launch_bounds__(256) void k_mesh_cells_uf(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                       size_t view_stride, double thr2, uint8_t *__restrict__ cells, int *__restrict__ labels,
                                                       int *__restrict__ sizes, unsigned *__restrict__ counts, unsigned long long *__restrict__ stat)
{
    mesh_cells<true>(valid, points, W, H, pitch, view_stride, thr2, cells, labels, sizes, counts, stat);
}

int mesh_row_chunks(const KParams &P) { return (P.W + MESH_CHUNK - 1) / MESH_CHUNK; }
int mesh_chunks(const KParams &P) { return P.H * mesh_row_chunks(P); }

int launch_mesh_cells(const KParams &P, const MeshLaunch &L, float max_edge, uint8_t *cells, int *labels, int *sizes, unsigned long long *stat,
                      const CompactScratch &c, void *stream)
{
    const double thr2 = mesh_thr2(max_edge);
    hipStream_t st = (hipStream_t)stream;
    if (labels)
        hipLaunchKernelGGL(k_mesh_cells_uf, L.grid, dim3(256), 0, st, L.in.valid, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, thr2, cells + L.v0,
                           labels + L.v0, sizes + L.v0, c.cnt, stat);
    else
        hipLaunchKernelGGL(k_mesh_cells, L.grid, dim3(256), 0, st, L.in.valid, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, thr2, cells + L.v0, c.cnt);
    return launch_compact_scan(c.cnt, c.off, L.n_chunks, L.n_views, c.tot, stream);
}

int launch_mesh_views(const KParams &P, int first_view, int n_views, float max_edge, const CompactScratch &s, int *faces, size_t face_stride,
                      void *stream)
{
    const MeshLaunch L = mesh_launch(P, first_view, n_views);
    const CompactScratch c = L.sliced(s, 2);
    const double thr2 = mesh_thr2(max_edge);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mesh_count, L.grid, dim3(256), 0, st, L.in.valid, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, thr2, c.cnt);
    int rc = launch_compact_scan(c.cnt, c.off, L.n_chunks, 2 * n_views, c.tot, stream);
    if (rc) return rc;
    if (P.H > 1)
        hipLaunchKernelGGL(k_mesh_emit, dim3(L.nck, P.H - 1, n_views), dim3(256), 0, st, L.in.valid, L.in.points, P.W, P.H, P.pitch, P.px_view_stride, thr2,
                           (const unsigned *)c.cnt, (const unsigned long long *)c.off, faces + 3 * (size_t)first_view * face_stride, face_stride);
    return (int)hipGetLastError();
}

}  // namespace sl3d
