// sl3d_align_lane.h -- what the kernels of the two turntable refinements share, each spelled once: the tile of 64 x 32 window pixels a block
// of 256 threads owns and a lane's walk over it, the load of a point, the candidate search around a projection, the way a wave's words
// reach the pair's record, and the launcher's memset and dispatch over the window.  Used by k_align_pass (sl3d_align.hip) and by
// k_align_normals / k_align_plane_pass (sl3d_align_plane.hip), inlined into each: the kernels' instruction streams are those of the
// written-out forms (profiles/align_shared_isa_identity.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sl3d_align.h"
#include "sl3d_block.h"
#include "sl3d_internal.h"

namespace sl3d {

#define ALIGN_TILE_W 64
#define ALIGN_TILE_ROWS 32

// blockIdx.x counts the tiles row-major: the tile row of the block and the column of the lane.  A wave takes the tile rows wave, wave + 4,
// ...: align_row is the lane's row in round k of ALIGN_TILE_ROWS / 4.  The caller skips r >= H and c >= W
struct AlignLane {
    int tile_r, c;
};
__device__ __forceinline__ AlignLane align_lane(int W)
{
    const int tiles_x = (W + ALIGN_TILE_W - 1) / ALIGN_TILE_W;
    const int tile_r = (int)(blockIdx.x / (unsigned)tiles_x), tile_c = (int)(blockIdx.x - (unsigned)tile_r * (unsigned)tiles_x);
    return {tile_r, tile_c * ALIGN_TILE_W + (int)(threadIdx.x & 63)};
}
__device__ __forceinline__ int align_row(int tile_r, int k) { return tile_r * ALIGN_TILE_ROWS + 4 * k + (int)(threadIdx.x >> 6); }

// the tiles of a view: gridDim.x of every launch here
inline unsigned align_tiles(const KParams &P)
{
    return (unsigned)((P.W + ALIGN_TILE_W - 1) / ALIGN_TILE_W) * (unsigned)((P.H + ALIGN_TILE_ROWS - 1) / ALIGN_TILE_ROWS);
}

__device__ __forceinline__ void load3(const float *__restrict__ points, size_t px, float *p)
{
    p[0] = points[3 * px], p[1] = points[3 * px + 1], p[2] = points[3 * px + 2];
}

// The candidate search: the nearest target point to ph among the (2 * WINDOW + 1)^2 pixels around (cc, rr), clipped to the window's W x H
// (never to the pitch); the valid byte is read first, the 12-byte point only behind a 1.  A strict comparison: of equal distances the first
// in row-major order stays.  best (double, +inf going in) and q (float[3]) are the caller's; WON is one more statement run when the
// candidate at pixel tpx wins (the plane form remembers the pixel), or nothing.  A macro: as a __forceinline__ function -- pointer outputs,
// or references and a functor -- the selects of every pass kernel become moves under branches and the VGPR counts move.
#define ALIGN_SEARCH(WINDOW, cc, rr, W, H, pitch, tvalid, tpoints, ph, best, q, WON)     \
    _Pragma("unroll 1") for (int dy = -(WINDOW); dy <= (WINDOW); dy++)                   \
    {                                                                                    \
        const int tr = (rr) + dy;                                                        \
        if (tr < 0 || tr >= (H)) continue;                                               \
        _Pragma("unroll") for (int dx = -(WINDOW); dx <= (WINDOW); dx++)                 \
        {                                                                                \
            const int tc = (cc) + dx;                                                    \
            if (tc < 0 || tc >= (W)) continue;                                           \
            const size_t tpx = (size_t)tr * (pitch) + tc;                                \
            if ((tvalid)[tpx] != 1) continue;                                            \
            float cand[3];                                                               \
            load3(tpoints, tpx, cand);                                                   \
            const double d2 = align_d2(cand, ph);                                        \
            if (d2 < best) {                                                             \
                best = d2, q[0] = cand[0], q[1] = cand[1], q[2] = cand[2];               \
                WON;                                                                     \
            }                                                                            \
        }                                                                                \
    }

// The tail of a pass.  Lane 0 of every wave has written the wave's WORDS sums to s_words[wave] (the kernel's own statements: which sum is
// which word is the form's business, and with the row handed over as an array the int sums are widened in another order and the plane form
// schedules differently).  Here the barrier, the four waves added, then one 64-bit integer atomicAdd per non-zero word into the pair's
// record, which the launcher cleared on the stream
template <int WORDS>
__device__ __forceinline__ void align_words_add(const long long (*s_words)[WORDS], unsigned long long *__restrict__ pair_record)
{
    __syncthreads();
    if (threadIdx.x < WORDS) {
        const long long v = (s_words[0][threadIdx.x] + s_words[1][threadIdx.x]) + (s_words[2][threadIdx.x] + s_words[3][threadIdx.x]);
        if (v) atomicAdd(pair_record + threadIdx.x, (unsigned long long)v);
    }
}

// The memset of the n_pairs records of `words` words and the launch of the pass's instantiation for `window`: launch(w) is called with an
// std::integral_constant whose value is the window
template <typename Launch>
inline int align_dispatch(unsigned long long *record, int n_pairs, int words, int window, hipStream_t st, Launch launch)
{
    const hipError_t e = hipMemsetAsync(record, 0, (size_t)n_pairs * words * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    (void)hipGetLastError();
    switch (window) {
    case 0: launch(std::integral_constant<int, 0>()); break;
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 3: launch(std::integral_constant<int, 3>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
static_assert(ALIGN_MAX_WINDOW == 4, "align_dispatch names every window");

}  // namespace sl3d
