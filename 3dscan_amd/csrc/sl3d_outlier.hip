// sl3d_outlier.hip -- gfx950 (MI355X, wave64) kernels of the radius outlier filter (sl3d_filter_outliers; the rule: include/sl3d_filter.h, its
// arithmetic: sl3d_outlier.h):
//   k_outlier_support<RADIUS> : per window pixel the number of samples of its (2 * RADIUS + 1)^2 neighbourhood within max_dist, one byte
//                               (SL3D_OUTLIER_NO_SAMPLE where the pixel is no sample) into the support plane
//   k_outlier_apply           : the samples whose support is below min_neighbours lose their valid byte, their point becomes the NaN of
//                               the dense kernels, their intersection_points entry 0; the two counts per view
// Two launches, because a pixel decides from its neighbours as they were when the call was enqueued (the Jacobi form of
// sl3d_repair_periods): the second launch writes the planes only after every block of the first has read them.
//
// k_outlier_support: a block of 256 threads owns a tile of 64 x 8 window pixels, a wave two tile rows (w and w + 4); grid z is the view.  The tile and a
// halo of RADIUS pixels are staged in LDS as three float planes, so the 64 lanes of a wave read 64 consecutive dwords for every (dr, dc):
// no bank conflict.  A staged pixel outside the window, or whose valid byte is not 1, is stored as NaN: "a NaN length is not in range"
// then is the validity test and the clipping, and the window loop -- its columns unrolled, RADIUS is a template parameter -- holds no branch.  Whether
// the pixel itself is a sample is decided by its valid byte, read again from memory, not by its staged point.  At RADIUS 4 the tile is 72 x
// 16 x 12 B = 13.8 KB.  No scratch, no atomics.  The support bytes of 4 lanes go out as one dword (rows are a multiple of 16 bytes long
// and a tile starts on a multiple of 64, so the dword of a window pixel lies inside the row).
// k_outlier_apply: a lane owns 4 consecutive pixels of one row (sl3d_block.h) in each of its block's runs; stores only where it rejects; the counts through wave_sum,
// one LDS word per count and wave, one integer atomic add per non-zero count and block into words the host zeroed on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_outlier.h"

namespace sl3d {

#define OUTLIER_TILE_W 64
#define OUTLIER_TILE_H 8

// valid / points: the planes of the launch's first view; support: its support plane; views px_view_stride pixels apart
template <int RADIUS>
__global__ __launch_bounds__(256) void k_outlier_support(const uint8_t *__restrict__ valid, const float *__restrict__ points, int W, int H, int pitch,
                                                         size_t px_view_stride, double thr2, uint8_t *__restrict__ support)
{
    constexpr int TW = OUTLIER_TILE_W + 2 * RADIUS, TH = OUTLIER_TILE_H + 2 * RADIUS;
    __shared__ float s_x[TH * TW], s_y[TH * TW], s_z[TH * TW];
    const size_t v0 = (size_t)blockIdx.z * px_view_stride;
    valid += v0, points += 3 * v0, support += v0;
    const int c0 = (int)blockIdx.x * OUTLIER_TILE_W, r0 = (int)blockIdx.y * OUTLIER_TILE_H;
    for (int i = (int)threadIdx.x; i < TH * TW; i += 256) {
        const int tr = i / TW, tc = i - tr * TW;
        const int r = r0 - RADIUS + tr, c = c0 - RADIUS + tc;
        float x = __builtin_nanf(""), y = x, z = x;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            const size_t px = (size_t)r * pitch + c;
            if (valid[px] == 1) x = points[3 * px], y = points[3 * px + 1], z = points[3 * px + 2];
        }
        s_x[i] = x, s_y[i] = y, s_z[i] = z;
    }
    __syncthreads();
    // a wave owns the tile rows wave, wave + 4: a lane two pixels of one column, one after the other
    const int lx = (int)(threadIdx.x & 63), c = c0 + lx;
#pragma unroll 1
    for (int ly = (int)(threadIdx.x >> 6); ly < OUTLIER_TILE_H; ly += 4) {
        const int r = r0 + ly;
        const bool inside = r < H && c < W;
        const int at = (ly + RADIUS) * TW + lx + RADIUS;
        const float p[3] = {s_x[at], s_y[at], s_z[at]};
        unsigned n = 0;
        // a row of the neighbourhood per trip, its 2 * RADIUS + 1 columns unrolled: unrolled over the rows too, RADIUS 3 and 4 hold every
        // staged point of the neighbourhood in registers at once (198 and 256 VGPRs).  The pixel itself is masked out, not branched around
#pragma unroll 1
        for (int dr = -RADIUS; dr <= RADIUS; dr++) {
            const int row = at + dr * TW;
#pragma unroll
            for (int dc = -RADIUS; dc <= RADIUS; dc++) {
                const float q[3] = {s_x[row + dc], s_y[row + dc], s_z[row + dc]};
                n += (unsigned)outlier_in_range(p, q, thr2) & (unsigned)((dr | dc) != 0);
            }
        }
        const size_t px = (size_t)r * pitch + c;
        const unsigned b = inside && valid[px] == 1 ? n : SL3D_OUTLIER_NO_SAMPLE;
        // the bytes of lanes 4k .. 4k + 3 as one dword of lane 4k (every lane of the wave takes part in the shuffles)
        const unsigned w = b | __shfl_down(b, 1, 64) << 8 | __shfl_down(b, 2, 64) << 16 | __shfl_down(b, 3, 64) << 24;
        if (inside && (lx & 3) == 0) *(unsigned *)(support + px) = w;
    }
}

// Quad t of a view is quad (t mod lpr) of window row (t / lpr), lpr = quads that hold window pixels; a block owns OUTLIER_APPLY_RUNS runs
// of 256 consecutive quads, a lane one quad of each; grid y is the view.  valid / points / ipoints (NULL without the stage planes) /
// support: of the launch's first view; counts: [n_views][2] words the launch ADDS the views' samples and rejected samples to.
// min_neighbours == 0: nothing is rejected, the launch only counts.  Several runs per block because of the counts: the words of 16 views
// share one 128-byte line, and the atomics on it are served one after the other.  With one run per block -- 2 x 2025 atomics per 1080p
// view -- this launch took 305 us over 16 views whatever it rejected, about 5 ns per atomic; with 8 runs it takes 56 to 135 us, by
// the share it rejects.
#define OUTLIER_APPLY_RUNS 8
__global__ __launch_bounds__(256) void k_outlier_apply(uint8_t *__restrict__ valid, float *__restrict__ points, double *__restrict__ ipoints,
                                                       const uint8_t *__restrict__ support, int W, int H, int pitch, size_t px_view_stride,
                                                       int min_neighbours, unsigned *__restrict__ counts)
{
    __shared__ unsigned s_cnt[2][4];
    const size_t v0 = (size_t)blockIdx.y * px_view_stride;
    const int lpr = (W + 3) / 4;
    unsigned samples = 0, rejected = 0;
    for (int run = 0; run < OUTLIER_APPLY_RUNS; run++) {
        const unsigned t = (blockIdx.x * OUTLIER_APPLY_RUNS + run) * 256u + threadIdx.x;
        const int row = (int)(t / (unsigned)lpr), c0 = 4 * (int)(t - (unsigned)row * (unsigned)lpr);
        if (row >= H) break;
        const size_t px = v0 + (size_t)row * pitch + c0;
        const unsigned vw = *(const unsigned *)(valid + px), sw = *(const unsigned *)(support + px);
        const unsigned in_window = QUAD_IN_WINDOW(W, c0);
        unsigned keep = ~0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool sample = (in_window >> k & 1u) && (vw >> (8 * k) & 0xffu) == 1u;
            const bool reject = sample && outlier_rejected(sw >> (8 * k) & 0xffu, min_neighbours);
            samples += sample, rejected += reject;
            if (reject) {
                keep &= ~(0xffu << (8 * k));
                float *p = points + 3 * (px + k);
                p[0] = p[1] = p[2] = __builtin_nanf("");
                if (ipoints) {
                    double *ip = ipoints + 3 * (px + k);
                    ip[0] = ip[1] = ip[2] = 0.0;
                }
            }
        }
        if (keep != ~0u) *(unsigned *)(valid + px) = vw & keep;
    }
    samples = wave_sum(samples), rejected = wave_sum(rejected);
    if ((threadIdx.x & 63) == 0) s_cnt[0][threadIdx.x >> 6] = samples, s_cnt[1][threadIdx.x >> 6] = rejected;
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned c = BLOCK_SUM_TOTAL(s_cnt[threadIdx.x]);
        if (c) atomicAdd(counts + 2 * blockIdx.y + threadIdx.x, c);
    }
}

template <int RADIUS>
static void launch_support(const KParams &P, int first_view, int n_views, double thr2, uint8_t *support, hipStream_t st)
{
    const dim3 grid((P.W + OUTLIER_TILE_W - 1) / OUTLIER_TILE_W, (P.H + OUTLIER_TILE_H - 1) / OUTLIER_TILE_H, n_views);
    const ViewPlanes in = view_planes(P, first_view);
    hipLaunchKernelGGL(k_outlier_support<RADIUS>, grid, dim3(256), 0, st, in.valid, in.points, P.W, P.H, P.pitch, P.px_view_stride, thr2,
                       support + (size_t)first_view * P.px_view_stride);
}

int launch_outlier_support(const KParams &P, int first_view, int n_views, int radius, float max_dist, uint8_t *support, void *stream)
{
    const double thr2 = mesh_thr2(max_dist);
    (void)hipGetLastError();
    switch (radius) {
    case 1: launch_support<1>(P, first_view, n_views, thr2, support, (hipStream_t)stream); break;
    case 2: launch_support<2>(P, first_view, n_views, thr2, support, (hipStream_t)stream); break;
    case 3: launch_support<3>(P, first_view, n_views, thr2, support, (hipStream_t)stream); break;
    case 4: launch_support<4>(P, first_view, n_views, thr2, support, (hipStream_t)stream); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

int launch_outlier_apply(const KParams &P, int first_view, int n_views, int min_neighbours, const uint8_t *support, unsigned *counts, void *stream)
{
    const unsigned blocks = (unsigned)(((long)((P.W + 3) / 4) * P.H + 256 * OUTLIER_APPLY_RUNS - 1) / (256 * OUTLIER_APPLY_RUNS));
    const size_t v0 = (size_t)first_view * P.px_view_stride;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_outlier_apply, dim3(blocks, n_views), dim3(256), 0, (hipStream_t)stream, P.valid + v0, P.points + 3 * v0,
                       P.ipoints ? P.ipoints + 3 * v0 : nullptr, support + v0, P.W, P.H, P.pitch, P.px_view_stride, min_neighbours, counts);
    return (int)hipGetLastError();
}

}  // namespace sl3d
