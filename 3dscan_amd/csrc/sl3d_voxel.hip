// sl3d_voxel.hip -- gfx950 (MI355X, wave64) kernels of the voxel grid over an unorganised cloud (sl3d_voxel_grid; the rule:
// include/sl3d_voxel.h, its arithmetic: sl3d_voxel.h):
//   k_voxel_insert<CENTROID, COLLAPSE> : a lane per point; the point's cell is claimed or found in a lock-free hash table over 64-bit keys
//                                        (linear probing, 64-bit atomicCAS), the cell's first index, count and -- CENTROID -- its three
//                                        fixed-point sums are accumulated with integer atomics; slot_of[i] = the slot, for run heads
//   k_voxel_count                      : per 1024-point block the cells that emit there (point i emits iff it is the first of its cell and
//                                        the cell holds min_points points), and the occupied cells
//   k_compact_scan (sl3d_clouds.hip)   : the blocks' offsets and the total
//   k_voxel_scatter<CENTROID>          : xyz, first and count of the emitting cells in output order, staged in LDS, flushed coalesced
// The run collapse (COLLAPSE): neighbouring pixels of an organised scan fall into the same cell, so consecutive lanes of a wave often hold
// one key.  Each such run is collapsed onto its head lane -- the heads by a ballot, the run's q sums by a segmented shuffle reduction every
// lane takes part in -- and only the head touches the table.  A cell's first point is the head of its run, so only heads store a slot.
// -DSL3D_VOXEL_NO_COLLAPSE (measurement builds, tools/voxel_timing.py) instantiates the form in which every lane is its own head.
// Everything the kernels add up is an integer at device scope on memory the stream initialised: the result does not depend on the order
// of arrival.  The probe loop is bounded by the capacity; at a load factor <= 0.5 it never runs out, and if it did the lane sets the
// error word and leaves.  No loop here can spin without bound.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_voxel.h"

namespace sl3d {

#ifdef SL3D_VOXEL_NO_COLLAPSE
#define VOXEL_COLLAPSE false
#else
#define VOXEL_COLLAPSE true
#endif

#ifdef SL3D_VOXEL_TIMING
// Measurement builds (tools/voxel_timing.py): an event between the launches of a grid call -- in front of the memsets, behind them, behind
// k_voxel_insert, k_voxel_count, k_compact_scan and k_voxel_scatter -- and the call that reads the five times of the last one
static hipEvent_t g_stamp[6];
static bool g_stamps_made = false;
#define VOXEL_STAMP(k, st) (void)hipEventRecord(g_stamp[k], st)
extern "C" int sl3d_voxel_launch_times(float ms[5])
{
    if (!g_stamps_made || hipEventSynchronize(g_stamp[5]) != hipSuccess) return -1;
    for (int k = 0; k < 5; k++)
        if (hipEventElapsedTime(&ms[k], g_stamp[k], g_stamp[k + 1]) != hipSuccess) return -1;
    return 0;
}
#else
#define VOXEL_STAMP(k, st) (void)0
#endif

// Lane t of block b takes point i = 256 b + t; the grid covers the 1024-point blocks of the emission whole, so every word of slot_of is
// written (VOXEL_NONE behind the cloud's end).  n < 2^31: i fits an unsigned.
template <bool CENTROID, bool COLLAPSE>
__global__ __launch_bounds__(256) void k_voxel_insert(const float *__restrict__ cloud, unsigned n, double L, VoxelTable T, unsigned *__restrict__ slot_of,
                                                      unsigned long long *__restrict__ words)
{
    __shared__ unsigned s_cnt[4];
    const unsigned i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    unsigned long long key = VOXEL_EMPTY;  // of a dropped point and behind the end: a run of its own kind, whose head does nothing
    int q[3] = {0, 0, 0};
    unsigned dropped = 0;
    if (i < n) {
        const float *p = cloud + 3 * (size_t)i;
        const float x[3] = {p[0], p[1], p[2]};
        double c[3];
        const int ok = voxel_cell(x[0], L, &c[0]) & voxel_cell(x[1], L, &c[1]) & voxel_cell(x[2], L, &c[2]);
        if (ok) {
            key = voxel_key(c[0], c[1], c[2]);
            if (CENTROID)
                for (int k = 0; k < 3; k++) q[k] = (int)voxel_q(x[k], c[k], L);  // in [-1, 2^24]: 64 of them sum inside an int
        } else
            dropped = 1;
    }
    // dropped points: one atomic per block
    BLOCK_SUM(dropped, s_cnt);
    if (threadIdx.x == 0) {
        const unsigned d = BLOCK_SUM_TOTAL(s_cnt);
        if (d) atomicAdd(words + VOXEL_WORD_DROPPED, (unsigned long long)d);
    }
    bool head = true;
    unsigned len = 1;
    if (COLLAPSE) {
        const unsigned long long before = __shfl_up(key, 1, 64);
        head = lane == 0 || before != key;
        // the run of a lane ends in front of the next head; a head's run is [lane, end)
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const unsigned end = above ? lane + (unsigned)__ffsll((long long)above) : 64u;
        len = end - lane;
        if (CENTROID)
            for (unsigned off = 1; off < 64; off <<= 1)
                for (int k = 0; k < 3; k++) {
                    const int t = __shfl_down(q[k], off, 64);
                    if (lane + off < end) q[k] += t;
                }
    }
    unsigned slot = VOXEL_NONE;
    if (head && key != VOXEL_EMPTY) {
        const unsigned long long mask = T.capacity - 1;
        unsigned long long s = voxel_hash(key) & mask, probes = 0;
        for (; probes < T.capacity; probes++) {
            const unsigned long long was = atomicCAS(T.key + s, VOXEL_EMPTY, key);
            if (was == VOXEL_EMPTY || was == key) break;
            s = (s + 1) & mask;
        }
        if (probes == T.capacity)
            atomicAdd(words + VOXEL_WORD_ERROR, 1ull);
        else {
            atomicMin(T.first + s, i);
            atomicAdd(T.count + s, len);
            if (CENTROID)
                for (int k = 0; k < 3; k++) atomicAdd((unsigned long long *)T.sums + k * T.capacity + s, (unsigned long long)(long long)q[k]);
            slot = (unsigned)s;
        }
    }
    slot_of[i] = slot;
}

// Which of the lane's 4 points i0 .. i0 + 3 emit (bits 0-3) and which are the first of an occupied cell (bits 4-7).  w: their slot_of words.
// A word is a slot iff it is below the capacity -- VOXEL_NONE is not, but for a table of 2^32 slots, where it names the last one: there,
// as everywhere, `first[slot] == i` decides, and only the head that claimed a cell ever stored its index into first
__device__ __forceinline__ unsigned voxel_emits(const uint4 w, unsigned i0, const VoxelTable &T, unsigned long long min_points)
{
    const unsigned s[4] = {w.x, w.y, w.z, w.w};
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (s[k] < T.capacity && T.first[s[k]] == i0 + k) bits |= (16u | (unsigned)(T.count[s[k]] >= min_points)) << k;
    return bits;
}

// a block of 256 lanes owns 1024 consecutive points, a lane 4 (sl3d_block.h)
__global__ __launch_bounds__(256) void k_voxel_count(const unsigned *__restrict__ slot_of, VoxelTable T, unsigned long long min_points,
                                                     unsigned *__restrict__ block_counts, unsigned long long *__restrict__ words)
{
    __shared__ unsigned s_cnt[4], s_occ[4];
    const unsigned i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    const unsigned bits = voxel_emits(*(const uint4 *)(slot_of + i0), i0, T, min_points);
    unsigned c = __popc(bits & 15u), o = __popc(bits >> 4);
    BLOCK_SUM(c, s_cnt);
    BLOCK_SUM(o, s_occ);
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
        const unsigned occupied = BLOCK_SUM_TOTAL(s_occ);
        if (occupied) atomicAdd(words + VOXEL_WORD_OCCUPIED, (unsigned long long)occupied);
    }
}

template <bool CENTROID>
__global__ __launch_bounds__(256) void k_voxel_scatter(const float *__restrict__ cloud, double L, const unsigned *__restrict__ slot_of, VoxelTable T,
                                                       unsigned long long min_points, const unsigned long long *__restrict__ block_offsets, VoxelOut out)
{
    __shared__ unsigned s_wave[4];
    __shared__ float s_xyz[1024 * 3];
    __shared__ int s_first[1024];
    __shared__ unsigned s_count[1024];
    const unsigned i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    const uint4 w = *(const uint4 *)(slot_of + i0);
    const unsigned bits = voxel_emits(w, i0, T, min_points) & 15u;
    const unsigned c = __popc(bits);
    const unsigned incl = wave_prefix(c, s_wave);
    unsigned local = waves_before(s_wave, 0u) + (incl - c);
    const unsigned block_total = BLOCK_SUM_TOTAL(s_wave);
    const unsigned long long block_off = block_offsets[blockIdx.x];
    const unsigned s[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (bits >> k & 1u) {
            const unsigned i = i0 + k, n = T.count[s[k]];
            const float *p = cloud + 3 * (size_t)i;
            float x[3] = {p[0], p[1], p[2]};
            if (CENTROID && n > 1)  // (a one-point cell's fixed-point centroid may differ from its point by an ulp: it gives the point)
                for (int j = 0; j < 3; j++) {
                    double cell;
                    (void)voxel_cell(x[j], L, &cell);
                    x[j] = voxel_centroid(cell, L, T.sums[j * T.capacity + s[k]], n);
                }
            s_xyz[3 * local + 0] = x[0];
            s_xyz[3 * local + 1] = x[1];
            s_xyz[3 * local + 2] = x[2];
            s_first[local] = (int)i;
            s_count[local] = n;
            local++;
        }
    __syncthreads();
    block_flush(out.xyz + 3 * block_off, s_xyz, 3 * block_total);
    block_flush(out.first + block_off, s_first, block_total);
    block_flush(out.count + block_off, s_count, block_total);
}

template <bool CENTROID>
static void launch_voxel_kernels(const float *cloud, unsigned n, unsigned nb, double L, unsigned long long min_points, const VoxelTable &T, unsigned *slot_of,
                                 const CompactScratch &s, unsigned long long *words, const VoxelOut &out, hipStream_t st)
{
    hipLaunchKernelGGL((k_voxel_insert<CENTROID, VOXEL_COLLAPSE>), dim3(4 * nb), dim3(256), 0, st, cloud, n, L, T, slot_of, words);
    VOXEL_STAMP(2, st);
    hipLaunchKernelGGL(k_voxel_count, dim3(nb), dim3(256), 0, st, slot_of, T, min_points, s.cnt, words);
    VOXEL_STAMP(3, st);
    (void)launch_compact_scan(s.cnt, s.off, (int)nb, 1, words + VOXEL_WORD_KEPT, st);
    VOXEL_STAMP(4, st);
    hipLaunchKernelGGL(k_voxel_scatter<CENTROID>, dim3(nb), dim3(256), 0, st, cloud, L, slot_of, T, min_points, s.off, out);
    VOXEL_STAMP(5, st);
}

// T: ONE allocation, key / first / count / sums in this order (16 bytes a slot, 40 with the sums), so that two memsets initialise it
int launch_voxel_grid(const float *cloud, long long n, float leaf, long long min_points, bool centroid, const VoxelTable &T, unsigned *slot_of,
                      const CompactScratch &s, unsigned long long *words, const VoxelOut &out, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n + 1023) / 1024);
#ifdef SL3D_VOXEL_TIMING
    for (int k = 0; k < 6 && !g_stamps_made; k++) (void)hipEventCreate(&g_stamp[k]);
    g_stamps_made = true;
#endif
    VOXEL_STAMP(0, st);
    hipError_t e = hipMemsetAsync(T.key, 0xFF, (size_t)T.capacity * 12, st);
    if (e == hipSuccess) e = hipMemsetAsync(T.count, 0, (size_t)T.capacity * (centroid ? 28 : 4), st);
    if (e == hipSuccess) e = hipMemsetAsync(words, 0, VOXEL_WORDS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    VOXEL_STAMP(1, st);
    (void)hipGetLastError();
    if (centroid)
        launch_voxel_kernels<true>(cloud, (unsigned)n, nb, (double)leaf, (unsigned long long)min_points, T, slot_of, s, words, out, st);
    else
        launch_voxel_kernels<false>(cloud, (unsigned)n, nb, (double)leaf, (unsigned long long)min_points, T, slot_of, s, words, out, st);
    return (int)hipGetLastError();
}

}  // namespace sl3d
