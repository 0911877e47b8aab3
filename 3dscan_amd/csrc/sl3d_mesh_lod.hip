// sl3d_mesh_lod.hip -- the level-of-detail mesh: one vertex per step x step pixel block, meshed with the rules of the fine mesh
// (sl3d_mesh_views_lod; the definition: include/sl3d.h, its arithmetic: sl3d_mesh_lod.h).  The new work is the block pass; what follows it
// are the launchers of the fine mesh over a KParams that describes the coarse grid (lod_params, sl3d_internal.h):
//   k_lod_blocks : grid (tiles of a coarse row, H', views).  A block stages ONE coarse row of a tile -- up to 16 fine rows of up to 256
//                  columns -- in LDS (sized per step: 3.5 KB per fine row): wave w takes rows w, w + 4, ..., lane l the row's quad l: one
//                  dword of candidate bytes and three 16-byte loads of points, 3 KB contiguous per wave and row, every fine byte read
//                  once (13 B per pixel).  The wave's prefix over the quads' candidates and -- where the ids come from the chunk offsets
//                  -- the candidates between the chunk's start and the tile (at most 1 KB of valid bytes per row more, lines the
//                  neighbouring tiles load anyway) go along.  Then three passes over the tile, none with a branch on loaded data: a thread
//                  per block ROW takes the minimum of the row's packed keys and a thread per block the minimum of those (no atomics);
//                  with the mean a thread per PIXEL tests its membership and sets a bit in the pixel's byte; a thread per block adds the
//                  members up (the ordered sum is a serial chain by definition: its parallelism is across coarse pixels, rows and
//                  views) and stores the coarse valid byte, point and id
//   launch_compact_views, launch_mesh_views over the coarse planes: vertices and faces in output order
//   k_lod_ids    : the representatives' ids in the order of the vertices: the chunk offsets launch_mesh_views left, wave-prefix rank, LDS
//                  staging, one coalesced run per chunk (k_cc_labels' scheme)
//   launch_mesh_normals over the coarse planes (on request)
// Nothing in the sequence depends on the data, no block waits for another, every output position follows from a scan.
#include <hip/hip_runtime.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_mesh_lane.h"
#include "sl3d_mesh_lod.h"

namespace sl3d {

// cand: the fine views' candidate bytes, [view][view_stride]; offsets: [view][H * nck] exclusive scan of the valid pixels per chunk (the
// candidates are the valid pixels), or NULL: vid, [view][view_stride], holds the id of every candidate.  Coarse planes: valid_c / ids_c
// [view][stride_c], points_c [view][stride_c][3], rows pitch_c apart
__global__ __launch_bounds__(256) void k_lod_blocks(const uint8_t *__restrict__ cand, const float *__restrict__ points, int W, int H, int pitch,
                                                    size_t view_stride, int step, int tc, int mean, double thr2,
                                                    const unsigned long long *__restrict__ offsets, int nck, const int *__restrict__ vid, int Wc,
                                                    int pitch_c, size_t stride_c, uint8_t *__restrict__ valid_c, float *__restrict__ points_c,
                                                    int *__restrict__ ids_c)
{
    // the tile, sized by the launch for its step (lod_tile_bytes): step rows of tw points, of tw / 4 candidate dwords and quad prefixes, step
    // words, (step + 1) * tc keys
    extern __shared__ __attribute__((aligned(16))) float s_pts[];
    const int tw = tc * step, nq = tw >> 2, col0 = blockIdx.x * tw, r0 = blockIdx.y * step, rows = min(step, H - r0);
    unsigned *s_cand = (unsigned *)(s_pts + 3 * step * tw), *s_qpre = s_cand + step * nq, *s_front = s_qpre + step * nq;
    unsigned *s_key = s_front + step, *s_rep = s_key + step * tc;  // a key per block row, per block
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t view = (size_t)blockIdx.z * view_stride;
    for (int i = wave; i < rows; i += 4) {  // (wave-uniform)
        const size_t row = view + (size_t)(r0 + i) * pitch;
        const int c = col0 + 4 * lane;
        unsigned w = 0u;
        if (lane < nq && c < W) {  // (the quad lies inside the pitch: a multiple of 16)
            const unsigned in_w = QUAD_IN_WINDOW(W, c);
            w = *(const unsigned *)(cand + row + c) & ((in_w & 1u) | (in_w & 2u) << 7 | (in_w & 4u) << 14 | (in_w & 8u) << 21);
            const float4 *p4 = (const float4 *)(points + 3 * (row + c));
            float4 *s4 = (float4 *)(s_pts + 3 * (i * tw + 4 * lane));
            const float4 a = p4[0], b = p4[1], d = p4[2];
            s4[0] = a, s4[1] = b, s4[2] = d;
        }
        if (lane < nq) s_cand[i * nq + lane] = w;
        unsigned incl = (unsigned)__popc(w);
        const unsigned own = incl;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane < nq) s_qpre[i * nq + lane] = incl - own;
        if (offsets) {  // (uniform) the chunk's columns in front of the tile: all inside the window
            unsigned n = 0u;
            for (int c1 = (col0 & ~(MESH_CHUNK - 1)) + 4 * lane; c1 < col0; c1 += 256) n += (unsigned)__popc(*(const unsigned *)(cand + row + c1) & 0x01010101u);
            n = wave_sum(n);
            if (lane == 0) s_front[i] = n;
        }
    }
    __syncthreads();
    // the representatives: a thread per block row, then a thread per block
    uint8_t *tile = (uint8_t *)s_cand;
    for (int u = threadIdx.x; u < rows * tc; u += 256) s_key[u] = lod_row_key(tile, tw, (u % tc) * step, u / tc, step);
    __syncthreads();
    if ((int)threadIdx.x < tc) {
        unsigned key = LOD_NONE;
        for (int dr = 0; dr < rows; dr++) key = lod_key_min(key, s_key[dr * tc + threadIdx.x]);
        s_rep[threadIdx.x] = key;
    }
    if (mean) {  // (uniform) the members: a thread per pixel, each its own byte
        __syncthreads();
        for (int p = threadIdx.x; p < rows * tw; p += 256) {
            const int dr = p / tw, col = p - dr * tw, t = col / step;
            tile[p] |= (uint8_t)lod_member_bit(tile, s_pts, tw, t * step, dr, col - t * step, step, s_rep[t], thr2);
        }
    }
    __syncthreads();
    const int t = threadIdx.x, C = blockIdx.x * tc + t;
    if (t >= tc || C >= Wc) return;
    const unsigned key = s_rep[t];
    float o[3] = {0.0f, 0.0f, 0.0f};
    int id = -1;
    if (key != LOD_NONE) {
        lod_block_position(tile, s_pts, tw, t * step, rows, step, key, mean, o);
        const int at = (int)(key & 255u), dr = at / step, c = t * step + (at - dr * step), r = r0 + dr;
        if (offsets)
            id = (int)offsets[((size_t)blockIdx.z * H + r) * nck + ((col0 + c) >> 10)] +
                 (int)lod_rank_in_chunk(tile + dr * tw, s_qpre + dr * nq, s_front[dr], col0, c);
        else
            id = vid[view + (size_t)r * pitch + col0 + c];
    }
    const size_t px = (size_t)blockIdx.z * stride_c + (size_t)blockIdx.y * pitch_c + C;
    valid_c[px] = key != LOD_NONE;
    points_c[3 * px] = o[0], points_c[3 * px + 1] = o[1], points_c[3 * px + 2] = o[2];
    ids_c[px] = id;
}
// the LDS of a block: at most 16 * 256 * 14 + 64 + 2 * 1024 = 59456 bytes, within the 64 KB a block may ask for without opting in
static size_t lod_tile_bytes(int step, int tc) { return (size_t)step * (size_t)(tc * step) * 14 + (size_t)step * 4 + (size_t)(step + 1) * tc * 4; }
static_assert(MESH_CHUNK == 1 << 10 && LOD_TILE_W <= MESH_CHUNK && LOD_TILE_W == 4 * 64, "a chunk is 1024 columns, a tile row one wave of quads");

// grid (chunks of a coarse row, H', views); counts / offsets: launch_mesh_views' over the coarse planes, [view][2][H' * chunks]; ids: the
// coarse id plane; out: [view][out_stride] in vertex order
__global__ __launch_bounds__(256) void k_lod_ids(const uint8_t *__restrict__ valid, const int *__restrict__ ids, int W, int H, int pitch, size_t view_stride,
                                                 const unsigned *__restrict__ counts, const unsigned long long *__restrict__ offsets,
                                                 int *__restrict__ out, size_t out_stride)
{
    const int r = blockIdx.y, nck = gridDim.x, chunk = r * nck + blockIdx.x, n_chunks = H * nck, c0 = blockIdx.x * MESH_CHUNK + threadIdx.x * 4;
    counts += (size_t)blockIdx.z * 2 * n_chunks;
    const unsigned block_vertices = counts[chunk];
    if (block_vertices == 0) return;  // (the whole block: nothing to write)
    offsets += (size_t)blockIdx.z * 2 * n_chunks;
    const size_t px = (size_t)blockIdx.z * view_stride + (size_t)r * pitch + c0;
    __shared__ unsigned s_wave[4];
    __shared__ int s_ids[MESH_CHUNK];  // the block's ids in output order
    const unsigned own = quad_bits(valid + px, W, c0);
    int4 v = make_int4(0, 0, 0, 0);
    if (own) v = *(const int4 *)(ids + px);
    const int id[4] = {v.x, v.y, v.z, v.w};
    const unsigned cv = __popc(own);
    unsigned rank = waves_before(s_wave, wave_prefix(cv, s_wave) - cv);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (own >> k & 1u) s_ids[rank++] = id[k];
    __syncthreads();
    block_flush(out + (size_t)blockIdx.z * out_stride + offsets[chunk], s_ids, block_vertices);
}

int launch_mesh_ids(const KParams &Pc, int first_view, int n_views, const CompactScratch &chk, const int *ids, int *vertex_ids, void *stream)
{
    const MeshLaunch L = mesh_launch(Pc, first_view, n_views);
    const CompactScratch c = L.sliced(chk, 2);
    hipLaunchKernelGGL(k_lod_ids, L.grid, dim3(256), 0, (hipStream_t)stream, L.in.valid, ids + L.v0, Pc.W, Pc.H, Pc.pitch, Pc.px_view_stride,
                       (const unsigned *)c.cnt, (const unsigned long long *)c.off, vertex_ids + L.v0, Pc.px_view_stride);
    return (int)hipGetLastError();
}

int launch_mesh_lod(const KParams &P, const KParams &Pc, int first_view, int n_views, int step, float lod_edge, bool mean, const LodSource &src,
                    const LodBuffers &b, bool normals, void *stream)
{
    const int tc = lod_tile_cols(step, LOD_TILE_W), tiles = (Pc.W + tc - 1) / tc;
    const size_t v0 = (size_t)first_view * P.px_view_stride, c0 = (size_t)first_view * Pc.px_view_stride;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lod_blocks, dim3(tiles, Pc.H, n_views), dim3(256), lod_tile_bytes(step, tc), st, src.cand + v0, (const float *)(P.points + 3 * v0), P.W, P.H, P.pitch,
                       P.px_view_stride, step, tc, (int)mean, mesh_thr2(lod_edge), src.offsets, mesh_row_chunks(P), src.vid ? src.vid + v0 : nullptr, Pc.W,
                       Pc.pitch, Pc.px_view_stride, Pc.valid + c0, Pc.points + 3 * c0, b.ids + c0);
    int rc = (int)hipGetLastError();
    if (!rc) rc = launch_compact_views(Pc, first_view, n_views, b.blk, b.xyz + 3 * c0, nullptr, nullptr, stream);
    if (!rc) rc = launch_mesh_views(Pc, first_view, n_views, lod_edge, b.chk, b.faces, b.face_stride, stream);
    if (rc) return rc;
    rc = launch_mesh_ids(Pc, first_view, n_views, b.chk, b.ids, b.vertex_ids, stream);
    if (!rc && normals) rc = launch_mesh_normals(Pc, first_view, n_views, lod_edge, b.nrm, b.normals, Pc.px_view_stride, stream);
    return rc;
}

}  // namespace sl3d
