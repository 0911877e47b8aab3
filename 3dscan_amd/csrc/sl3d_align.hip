// sl3d_align.hip -- gfx950 (MI355X, wave64) kernel of the turntable refinement (sl3d_align_sums / sl3d_refine_turntable; the rule:
// include/sl3d_align.h, its arithmetic: sl3d_align.h):
//   k_align_pass<WINDOW> : one correspondence pass of ICP with projective data association.  Pair j = blockIdx.y is (source view j + 1,
//                          target view j) of the launch.  A source pixel is turned by the estimate into the target's frame, projected
//                          into the camera, and the nearest target point among the (2 * WINDOW + 1)^2 pixels around its projection
//                          is its correspondence; the accepted pairs' fixed-point moments are added into the pair's 12 words.
// A block of 256 threads owns a tile of 64 x ALIGN_TILE_ROWS window pixels of the source view (blockIdx.x counts the tiles row-major); a wave
// takes the tile rows wave, wave + 4, ..., a lane one pixel of each: at any time the 64 lanes of a wave are 64 consecutive pixels of one
// row, so their footprints land on neighbouring target pixels.  Several rows per block because of the words: the 12 words of a pair share
// one 128-byte line and the atomics on it are served one after the other (DESIGN 4u measured ~5 ns each); with 32 rows a 1080p pair ends
// in 1020 x 12 of them at the most.
// For a candidate the valid byte is read first, the 12-byte point only behind a 1.  The window is clipped to the window's W x H, never to
// the pitch.  Lanes outside the view, lanes whose pixel is no source and sources without an accepted candidate contribute zeros.
// The words: the linear ones are summed in an int per lane and wave (sl3d_align.h: they fit), the products in an int64; wave sums by
// shuffles, the four waves through LDS, then one 64-bit integer atomicAdd per non-zero word and block into the record the host cleared
// on the stream.  Integer atomics only: the result does not depend on the order of arrival.  Every loop has a compile-time bound.
// Compiled with -ffp-contract=off.
// The tile walk, the search, the tail behind the waves' words and the dispatch over the window are sl3d_align_lane.h's, shared by the two forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_align_lane.h"

namespace sl3d {

// valid / points: the planes of the launch's first view (the target of pair 0), views px_view_stride pixels apart; record: [pairs][ALIGN_WORDS]
template <int WINDOW>
__global__ __launch_bounds__(256) void k_align_pass(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                    size_t px_view_stride, int col0, int row0, AlignCam cam, AlignPass a,
                                                    unsigned long long *__restrict__ record)
{
    __shared__ long long s_words[4][ALIGN_WORDS];
    const size_t t0 = (size_t)blockIdx.y * px_view_stride, s0 = t0 + px_view_stride;
    const uint8_t *tvalid = valid + t0, *svalid = valid + s0;
    const float *tpoints = points + 3 * t0, *spoints = points + 3 * s0;
    const AlignLane lane = align_lane(W);
    const int c = lane.c;
    // words 0 - 4, 9, 11 (n, ax, az, bx, bz, dy, sources) and words 5 - 8, 10 (the products)
    int lin[7] = {0, 0, 0, 0, 0, 0, 0};
    long long prod[5] = {0, 0, 0, 0, 0};
#pragma unroll 1
    for (int k = 0; k < ALIGN_TILE_ROWS / 4; k++) {
        const int r = align_row(lane.tile_r, k);
        if (r >= H || c >= W) continue;
        const size_t px = (size_t)r * pitch + c;
        if (svalid[px] != 1) continue;
        float p[3];
        load3(spoints, px, p);
        if (!align_finite(p)) continue;
        lin[6]++;
        double ph[3], dcc, drr;
        align_step(p, &a, ph);
        if (!align_centre(ph, &cam, col0, row0, &dcc, &drr)) continue;
        const int cc = (int)dcc, rr = (int)drr;  // below 2^30 in magnitude
        double best = (double)__builtin_inff();
        float q[3] = {0.0f, 0.0f, 0.0f};
        ALIGN_SEARCH(WINDOW, cc, rr, W, H, pitch, tvalid, tpoints, ph, best, q, (void)0)
        int64_t t[5];
        if (!align_accept(p, q, best, &a, t)) continue;
        const long long ax = t[0], az = t[1], bx = t[2], bz = t[3], dy = t[4];
        lin[0]++, lin[1] += (int)ax, lin[2] += (int)az, lin[3] += (int)bx, lin[4] += (int)bz, lin[5] += (int)dy;
        prod[0] += ax * bx + az * bz;
        prod[1] += ax * bz - az * bx;
        prod[2] += ax * ax + az * az;
        prod[3] += bx * bx + bz * bz;
        prod[4] += dy * dy;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) lin[k] = (int)wave_sum((unsigned)lin[k]);
#pragma unroll
    for (int k = 0; k < 5; k++) prod[k] = wave_sum64(prod[k]);
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_words[threadIdx.x >> 6];
        w[0] = lin[0], w[1] = lin[1], w[2] = lin[2], w[3] = lin[3], w[4] = lin[4];
        w[5] = prod[0], w[6] = prod[1], w[7] = prod[2], w[8] = prod[3];
        w[9] = lin[5], w[10] = prod[4], w[11] = lin[6];
    }
    align_words_add<ALIGN_WORDS>(s_words, record + (size_t)blockIdx.y * ALIGN_WORDS);
}

// the memset of the n_pairs records and the pass over views [first_view, first_view + n_pairs]
int launch_align_pass(const KParams &P, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, unsigned long long *record,
                      void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const ViewPlanes in = view_planes(P, first_view);
    return align_dispatch(record, n_pairs, ALIGN_WORDS, window, st, [&](auto w) {
        hipLaunchKernelGGL(k_align_pass<decltype(w)::value>, dim3(align_tiles(P), n_pairs), dim3(256), 0, st, in.valid, in.points, P.W, P.H, P.pitch,
                           P.px_view_stride, P.col0, P.row0, cam, a, record);
    });
}

}  // namespace sl3d
