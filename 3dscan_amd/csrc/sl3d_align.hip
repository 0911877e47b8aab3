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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_align.h"
#include "sl3d_block.h"
#include "sl3d_internal.h"

namespace sl3d {

#define ALIGN_TILE_W 64
#define ALIGN_TILE_ROWS 32

__device__ __forceinline__ long long wave_sum64(long long n)
{
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

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
    const int tiles_x = (W + ALIGN_TILE_W - 1) / ALIGN_TILE_W;
    const int tile_r = (int)(blockIdx.x / (unsigned)tiles_x), tile_c = (int)(blockIdx.x - (unsigned)tile_r * (unsigned)tiles_x);
    const int c = tile_c * ALIGN_TILE_W + (int)(threadIdx.x & 63);
    // words 0 - 4, 9, 11 (n, ax, az, bx, bz, dy, sources) and words 5 - 8, 10 (the products)
    int lin[7] = {0, 0, 0, 0, 0, 0, 0};
    long long prod[5] = {0, 0, 0, 0, 0};
#pragma unroll 1
    for (int k = 0; k < ALIGN_TILE_ROWS / 4; k++) {
        const int r = tile_r * ALIGN_TILE_ROWS + 4 * k + (int)(threadIdx.x >> 6);
        if (r >= H || c >= W) continue;
        const size_t px = (size_t)r * pitch + c;
        if (svalid[px] != 1) continue;
        const float p[3] = {spoints[3 * px], spoints[3 * px + 1], spoints[3 * px + 2]};
        if (!align_finite(p)) continue;
        lin[6]++;
        double ph[3], dcc, drr;
        align_step(p, &a, ph);
        if (!align_centre(ph, &cam, col0, row0, &dcc, &drr)) continue;
        const int cc = (int)dcc, rr = (int)drr;  // below 2^30 in magnitude
        double best = (double)__builtin_inff();
        float q[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int dy = -WINDOW; dy <= WINDOW; dy++) {
            const int tr = rr + dy;
            if (tr < 0 || tr >= H) continue;
#pragma unroll
            for (int dx = -WINDOW; dx <= WINDOW; dx++) {
                const int tc = cc + dx;
                if (tc < 0 || tc >= W) continue;
                const size_t tpx = (size_t)tr * pitch + tc;
                if (tvalid[tpx] != 1) continue;
                const float cand[3] = {tpoints[3 * tpx], tpoints[3 * tpx + 1], tpoints[3 * tpx + 2]};
                const double d2 = align_d2(cand, ph);
                if (d2 < best) best = d2, q[0] = cand[0], q[1] = cand[1], q[2] = cand[2];
            }
        }
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
    __syncthreads();
    if (threadIdx.x < ALIGN_WORDS) {
        const long long v = (s_words[0][threadIdx.x] + s_words[1][threadIdx.x]) + (s_words[2][threadIdx.x] + s_words[3][threadIdx.x]);
        if (v) atomicAdd(record + (size_t)blockIdx.y * ALIGN_WORDS + threadIdx.x, (unsigned long long)v);
    }
}

template <int WINDOW>
static void launch_pass(const KParams &P, int first_view, int n_pairs, const AlignCam &cam, const AlignPass &a, unsigned long long *record, hipStream_t st)
{
    const unsigned tiles = (unsigned)((P.W + ALIGN_TILE_W - 1) / ALIGN_TILE_W) * (unsigned)((P.H + ALIGN_TILE_ROWS - 1) / ALIGN_TILE_ROWS);
    const ViewPlanes in = view_planes(P, first_view);
    hipLaunchKernelGGL(k_align_pass<WINDOW>, dim3(tiles, n_pairs), dim3(256), 0, st, in.valid, in.points, P.W, P.H, P.pitch, P.px_view_stride, P.col0,
                       P.row0, cam, a, record);
}

// the memset of the n_pairs records and the pass over views [first_view, first_view + n_pairs]
int launch_align_pass(const KParams &P, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, unsigned long long *record,
                      void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(record, 0, (size_t)n_pairs * ALIGN_WORDS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    (void)hipGetLastError();
    switch (window) {
    case 0: launch_pass<0>(P, first_view, n_pairs, cam, a, record, st); break;
    case 1: launch_pass<1>(P, first_view, n_pairs, cam, a, record, st); break;
    case 2: launch_pass<2>(P, first_view, n_pairs, cam, a, record, st); break;
    case 3: launch_pass<3>(P, first_view, n_pairs, cam, a, record, st); break;
    case 4: launch_pass<4>(P, first_view, n_pairs, cam, a, record, st); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace sl3d
