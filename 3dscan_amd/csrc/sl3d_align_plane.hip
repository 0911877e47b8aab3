// sl3d_align_plane.hip -- gfx950 (MI355X, wave64) kernels of the point-to-plane turntable refinement (sl3d_align_normals /
// sl3d_align_plane_sums / sl3d_refine_turntable_plane; the rule: include/sl3d_align_plane.h, its arithmetic: sl3d_align_plane.h):
//   k_align_normals            : the normal of every pixel of the views' frame windows from its four neighbours -- three floats per pixel,
//                                NaN where there is none -- into planes laid out like points.  blockIdx.y is the view.  A lane per pixel,
//                                direct loads: the five valid bytes first, the points behind five 1s.  A row's neighbours are the next
//                                lanes' own pixels and the rows above and below are read by the waves above and below: L2 serves the reuse,
//                                no tile is staged in LDS.
//   k_align_plane_pass<WINDOW> : one correspondence pass.  Tiling, pairing and the search are k_align_pass's (sl3d_align.hip): a block of 256
//                                threads owns 64 x 32 window pixels of the source view, a wave the tile rows wave, wave + 4, ..., blockIdx.y
//                                is the pair.  The search also remembers the best candidate's pixel; its normal is read once, behind the
//                                distance test.  An accepted pair adds the 15 products of its five fixed-point features.
// The words: three counts in an int per lane, the products in an int64; wave sums by shuffles, the four waves through LDS, then one 64-bit
// integer atomicAdd per non-zero word and block into the record the launcher cleared on the stream.  Integer atomics only, no float
// atomics.  Every loop has a compile-time bound.  Compiled with -ffp-contract=off.
// The tile walk, the search, the tail behind the waves' words and the dispatch over the window are sl3d_align_lane.h's, shared by the two forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_align_lane.h"
#include "sl3d_align_plane.h"

namespace sl3d {

#define ALIGN_PLANE_PRODUCTS 15

// valid / points / normals: the planes of the launch's first view, views px_view_stride pixels apart
__global__ __launch_bounds__(256) void k_align_normals(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                       size_t px_view_stride, double edge2, float *__restrict__ normals)
{
    const size_t v0 = (size_t)blockIdx.y * px_view_stride;
    valid += v0, points += 3 * v0, normals += 3 * v0;
    const AlignLane lane = align_lane(W);
    const int c = lane.c;
#pragma unroll 1
    for (int k = 0; k < ALIGN_TILE_ROWS / 4; k++) {
        const int r = align_row(lane.tile_r, k);
        if (r >= H || c >= W) continue;
        const size_t px = (size_t)r * pitch + c;
        float n[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        if (c >= 1 && c + 1 < W && r >= 1 && r + 1 < H && valid[px] == 1 && valid[px - 1] == 1 && valid[px + 1] == 1 && valid[px - pitch] == 1 &&
            valid[px + pitch] == 1) {
            float q[3], l[3], rt[3], u[3], d[3];
            load3(points, px, q), load3(points, px - 1, l), load3(points, px + 1, rt), load3(points, px - pitch, u), load3(points, px + pitch, d);
            align_normal(q, l, rt, u, d, edge2, n);
        }
        normals[3 * px] = n[0], normals[3 * px + 1] = n[1], normals[3 * px + 2] = n[2];
    }
}

// valid / points: the planes of the launch's first view (the target of pair 0); normals: that view's normal plane; record: [pairs][ALIGN_PLANE_WORDS]
template <int WINDOW>
__global__ __launch_bounds__(256) void k_align_plane_pass(const uint8_t *__restrict__ valid, const float *__restrict__ points,
                                                          const float *__restrict__ normals, int W, int H, int pitch, size_t px_view_stride, int col0,
                                                          int row0, AlignCam cam, AlignPass a, unsigned long long *__restrict__ record)
{
    __shared__ long long s_words[4][ALIGN_PLANE_WORDS];
    const size_t t0 = (size_t)blockIdx.y * px_view_stride, s0 = t0 + px_view_stride;
    const uint8_t *tvalid = valid + t0, *svalid = valid + s0;
    const float *tpoints = points + 3 * t0, *spoints = points + 3 * s0, *tnormals = normals + 3 * t0;
    const AlignLane lane = align_lane(W);
    const int c = lane.c;
    int cnt[3] = {0, 0, 0};  // words 0, 16, 17: accepted, sources, lost to a missing normal
    long long prod[ALIGN_PLANE_PRODUCTS];
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_PRODUCTS; k++) prod[k] = 0;
#pragma unroll 1
    for (int k = 0; k < ALIGN_TILE_ROWS / 4; k++) {
        const int r = align_row(lane.tile_r, k);
        if (r >= H || c >= W) continue;
        const size_t px = (size_t)r * pitch + c;
        if (svalid[px] != 1) continue;
        float p[3];
        load3(spoints, px, p);
        if (!align_finite(p)) continue;
        cnt[1]++;
        double ph[3], dcc, drr;
        align_step(p, &a, ph);
        if (!align_centre(ph, &cam, col0, row0, &dcc, &drr)) continue;
        const int cc = (int)dcc, rr = (int)drr;  // below 2^30 in magnitude
        double best = (double)__builtin_inff();
        float q[3] = {0.0f, 0.0f, 0.0f};
        size_t bpx = 0;
        ALIGN_SEARCH(WINDOW, cc, rr, W, H, pitch, tvalid, tpoints, ph, best, q, bpx = tpx)
        int64_t f[ALIGN_PLANE_FEATURES];
        const int verdict = align_plane_accept(p, q, tnormals + 3 * bpx, best, &a, f);  // (the normal is read behind a finite best: bpx is a pixel of the window)
        cnt[2] += verdict == 2;
        if (verdict != 1) continue;
        cnt[0]++;
        int w = 0;
#pragma unroll
        for (int i = 0; i < ALIGN_PLANE_FEATURES; i++)
#pragma unroll
            for (int j = i; j < ALIGN_PLANE_FEATURES; j++) prod[w++] += (long long)f[i] * (long long)f[j];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cnt[k] = (int)wave_sum((unsigned)cnt[k]);
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_PRODUCTS; k++) prod[k] = wave_sum64(prod[k]);
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_words[threadIdx.x >> 6];
        w[0] = cnt[0], w[16] = cnt[1], w[17] = cnt[2];
#pragma unroll
        for (int k = 0; k < ALIGN_PLANE_PRODUCTS; k++) w[1 + k] = prod[k];
    }
    align_words_add<ALIGN_PLANE_WORDS>(s_words, record + (size_t)blockIdx.y * ALIGN_PLANE_WORDS);
}

int launch_align_normals(const KParams &P, int first_view, int n_views, float normal_edge, float *normals, void *stream)
{
    (void)hipGetLastError();
    const ViewPlanes in = view_planes(P, first_view);
    hipLaunchKernelGGL(k_align_normals, dim3(align_tiles(P), n_views), dim3(256), 0, (hipStream_t)stream, in.valid, in.points, P.W, P.H, P.pitch,
                       P.px_view_stride, align_thr2(normal_edge), normals);
    return (int)hipGetLastError();
}

// the memset of the n_pairs records and the pass over views [first_view, first_view + n_pairs]
int launch_align_plane_pass(const KParams &P, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, const float *normals,
                            unsigned long long *record, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const ViewPlanes in = view_planes(P, first_view);
    return align_dispatch(record, n_pairs, ALIGN_PLANE_WORDS, window, st, [&](auto w) {
        hipLaunchKernelGGL(k_align_plane_pass<decltype(w)::value>, dim3(align_tiles(P), n_pairs), dim3(256), 0, st, in.valid, in.points, normals, P.W, P.H,
                           P.pitch, P.px_view_stride, P.col0, P.row0, cam, a, record);
    });
}

}  // namespace sl3d
