// sl3d_block.h -- the block idioms of the kernels that turn a dense result into an ordered output (sl3d_clouds.hip: k_compact_count /
// k_compact_scatter; the mesh kernels of sl3d_mesh.hip, sl3d_mesh_normals.hip, sl3d_mesh_components.hip and sl3d_mesh_smooth.hip), each
// spelled once.  All of them run the same scheme over blocks of 256 threads (4 waves of 64), a lane owning 4 consecutive pixels: count per
// 1024-pixel block, scan the counts (k_compact_scan), walk the block again, rank every output by wave prefixes, stage the block's
// outputs in LDS in output order, flush them as one coalesced run.  (k_seg_scan / k_seg_close work on 16 waves and a 64-bit carry:
// their own text, sl3d_clouds.hip.)  Every helper is inlined into its kernel: the kernels' instruction streams are those of the
// written-out forms, identical or in another order with equal resource figures (profiles/r09_block_idioms_identity.txt,
// profiles/mesh_idioms_identity.txt).
#pragma once
#include <hip/hip_runtime.h>

namespace sl3d {

// the 4 valid bits of a dword of 0/1 valid bytes
__device__ __forceinline__ unsigned valid_nibble(unsigned w) { return (w & 1u) | (w >> 7 & 2u) | (w >> 14 & 4u) | (w >> 21 & 8u); }

// which of the quad's pixels c0 .. c0 + 3 lie inside a window of W columns, as bits (c0 < W; W and c0 plain ints, named twice).  A macro:
// as a function it moves the address arithmetic of k_mesh_normals_count
#define QUAD_IN_WINDOW(W, c0) ((W) - (c0) >= 4 ? 15u : (1u << ((W) - (c0))) - 1u)

// Sum of c over the block's 256 threads, through one word per wave: expands to the statements that leave the 4 wave sums in s_cnt
// (__shared__ unsigned [4]) behind a barrier; thread 0 -- and nobody else: the add stays under the caller's `threadIdx.x == 0` --
// then takes BLOCK_SUM_TOTAL(s_cnt), the four-word add (of any such array: the wave totals of a prefix too).  c is left holding the
// lane's partial sum.  A macro: in a function -- even the shuffle loop alone -- the same statements are scheduled differently in the count
// kernels.
#define BLOCK_SUM(c, s_cnt)                                                 \
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);    \
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;               \
    __syncthreads()
#define BLOCK_SUM_TOTAL(s_cnt) (s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3])

// the wave's sum of n over its lanes, in every lane
__device__ __forceinline__ unsigned wave_sum(unsigned n)
{
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}
__device__ __forceinline__ long long wave_sum64(long long n)
{
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

// inclusive prefix of c over the lane's wave; the wave's total goes to s_wave[wave] (__shared__ unsigned [4]), valid behind the barrier
// this ends in
__device__ __forceinline__ unsigned wave_prefix(unsigned c, unsigned *s_wave)
{
    unsigned incl = c;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off, 64);
        if ((threadIdx.x & 63) >= off) incl += t;
    }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    return incl;
}

// start + the totals of the waves in front of the lane's, added in this order.  k_mesh_normals starts from the lane's exclusive prefix
// within its wave, k_compact_scatter from 0 and adds that prefix to the result: each sum associated as its kernel had it
__device__ __forceinline__ unsigned waves_before(const unsigned *s_wave, unsigned start)
{
    for (int i = 0; i < (int)(threadIdx.x >> 6); i++) start += s_wave[i];
    return start;
}

// the block's n staged dwords go out as one contiguous run: coalesced dword stores
template <typename T>
__device__ __forceinline__ void block_flush(T *dst, const T *s, unsigned n)
{
    for (unsigned i = threadIdx.x; i < n; i += 256) dst[i] = s[i];
}

}  // namespace sl3d
