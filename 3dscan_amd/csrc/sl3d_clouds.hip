// sl3d_clouds.hip -- gfx950 (MI355X, wave64) kernels that CONSUME a result, and their launchers (each kernel's launch is spelled once):
//   k_compact_count / k_compact_scan / k_compact_scatter : O1 / N2, the ordered cloud of a dense result (launch_compact_views; the scan
//                                                          alone for sl3d_mesh.hip: launch_compact_scan)
//   k_seg_scan / k_seg_close                             : the segmented clouds the fused kernel writes -> offsets, totals, contiguous
//                                                          clouds, rotated on the way if asked (launch_seg_scan, launch_seg_close)
//   k_register                                           : N3 over a contiguous cloud (launch_register)
// The block idioms of the compaction kernels -- block sum, wave prefix, the waves in front, LDS flush -- live in sl3d_block.h, shared with
// sl3d_mesh.hip and sl3d_mesh_normals.hip; the planes of a launch's first view: view_planes, blocks per view: compact_blocks
// (sl3d_internal.h).  k_seg_scan / k_seg_close keep their own 16-wave, 64-bit forms here.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"

namespace sl3d {

// ------------------------------------------------------------------------------------------------
// O1 / N2: compaction of the dense cloud in the reference's row-major scan order
// (8/save_point_cloud.cpp:33-37 counts the valid pixels, :85-104 appends them).  Three launches on the
// context's stream: per-block counts (wave ballots), an exclusive scan of the block counts by one block,
// and the scatter.  A block covers 1024 consecutive pixels of the pitch-padded plane; the padding columns
// [W, pitch) of a row are clipped away like the mesh kernels clip them (QUAD_IN_WINDOW), whatever their valid
// bytes hold, so the scan order of the valid pixels is exactly the reference's.
// ------------------------------------------------------------------------------------------------
// The lane's 4 valid bytes (0/1, bit 0 of every byte) with those beyond the window cleared.  base: the lane's first pixel in the plane, a
// multiple of 4 -- the pitch is a multiple of 16, so the quad lies in one row; a plane stays below 2^32 pixels (sl3d_create)
__device__ __forceinline__ unsigned quad_valid_bytes(const uint8_t *valid, size_t base, size_t n_px, int W, int pitch)
{
    if (base >= n_px) return 0u;
    const int col = (int)((unsigned)base % (unsigned)pitch);
    if (col >= W) return 0u;
    const unsigned in_w = QUAD_IN_WINDOW(W, col);
    return *(const unsigned *)(valid + base) & ((in_w & 1u) | (in_w & 2u) << 7 | (in_w & 4u) << 14 | (in_w & 8u) << 21);
}

// blockIdx.y = view of a batch (strides in elements)
__global__ __launch_bounds__(256) void k_compact_count(const uint8_t *valid, size_t n_px, unsigned *block_counts, size_t valid_stride, int nb, int W,
                                                       int pitch)
{
    valid += (size_t)blockIdx.y * valid_stride;
    block_counts += (size_t)blockIdx.y * nb;
    __shared__ unsigned s_cnt[4];
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned c = __popc(quad_valid_bytes(valid, base, n_px, W, pitch));
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
}

// exclusive scan of n counts by a single 1024-thread block (n is a few thousand .. tens of thousands)
__global__ __launch_bounds__(1024) void k_compact_scan(const unsigned *counts, unsigned long long *offsets, int n, unsigned long long *total)
{
    counts += (size_t)blockIdx.x * n;   // one block per view of a batch
    offsets += (size_t)blockIdx.x * n;
    total += blockIdx.x;
    __shared__ unsigned long long s_part[1024];
    const int per = (n + 1023) / 1024, lo = threadIdx.x * per, hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (int i = lo; i < hi; i++) sum += counts[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
        unsigned long long v = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = threadIdx.x == 0 ? 0 : s_part[threadIdx.x - 1];
    for (int i = lo; i < hi; i++) { offsets[i] = run; run += counts[i]; }
    if (threadIdx.x == 1023) *total = s_part[1023];
}

// texture (may be NULL): the BGR camera image save_point_cloud() colours the cloud with (8/save_point_cloud.cpp:46-52,
// 70-72), [row][pitch][3] bytes; rgb_out receives r,g,b per compacted point
__global__ __launch_bounds__(256) void k_compact_scatter(const uint8_t *valid, const float *points, size_t n_px,
                                                         const unsigned long long *block_offsets, float *cloud, const uint8_t *texture,
                                                         uint8_t *rgb_out, size_t view_stride, int nb, int W, int pitch)
{
    valid += (size_t)blockIdx.y * view_stride;
    points += 3 * (size_t)blockIdx.y * view_stride;
    cloud += 3 * (size_t)blockIdx.y * view_stride;
    block_offsets += (size_t)blockIdx.y * nb;
    __shared__ unsigned s_wave[4];
    __shared__ __attribute__((aligned(16))) float s_pts[1024 * 3];  // the block's valid points, compacted
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    const unsigned w = quad_valid_bytes(valid, base, n_px, W, pitch);
    const unsigned c = __popc(w);
    // exclusive prefix of c over the block: wave scan by shuffles, then the 4 wave totals
    const unsigned incl = wave_prefix(c, s_wave);
    const unsigned wave_base = waves_before(s_wave, 0u), block_total = BLOCK_SUM_TOTAL(s_wave);
    unsigned local = wave_base + (incl - c);
    const unsigned long long block_off = block_offsets[blockIdx.x];
    if (w) {
        // the 4 pixels of a lane are 48 contiguous bytes: three 16-B loads, then the valid ones go to LDS in scan order
        const float4 *p4 = (const float4 *)(points + 3 * base);
        const float4 a = p4[0], b = p4[1], d = p4[2];
        const float q[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((w >> (8 * k)) & 1u) {
                s_pts[3 * local + 0] = q[3 * k + 0];
                s_pts[3 * local + 1] = q[3 * k + 1];
                s_pts[3 * local + 2] = q[3 * k + 2];
                if (texture) {
                    const uint8_t *t = texture + 3 * (base + k);  // b, g, r
                    uint8_t *o = rgb_out + 3 * (block_off + local);
                    o[0] = t[2]; o[1] = t[1]; o[2] = t[0];
                }
                local++;
            }
    }
    __syncthreads();
    // the block's segment of the cloud is contiguous: coalesced dword stores
    block_flush(cloud + 3 * block_off, s_pts, 3 * block_total);
}

// views [first_view, first_view + n_views): view first_view + k's compacted cloud goes to clouds + 3 * k * px_view_stride, its total to
// s.tot[first_view + k]; its block counts and their scan are slot k of s.cnt / s.off.  texture / rgb_out: one view (n_views == 1) only --
// that view's BGR image and the r,g,b of its cloud; NULL otherwise
int launch_compact_views(const KParams &P, int first_view, int n_views, const CompactScratch &s, float *clouds, const uint8_t *texture,
                         uint8_t *rgb_out, void *stream)
{
    const size_t n_px = P.px_view_stride;
    const int nb = (int)compact_blocks(P);
    const ViewPlanes in = view_planes(P, first_view);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_compact_count, dim3(nb, n_views), dim3(256), 0, st, in.valid, n_px, s.cnt, n_px, nb, P.W, P.pitch);
    hipLaunchKernelGGL(k_compact_scan, dim3(n_views), dim3(1024), 0, st, s.cnt, s.off, nb, s.tot + first_view);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb, n_views), dim3(256), 0, st, in.valid, in.points, n_px, s.off, clouds, texture, rgb_out, n_px, nb, P.W,
                       P.pitch);
    return (int)hipGetLastError();
}

// k_compact_scan for another unit (sl3d_mesh.hip): n_arrays independent arrays of n counts each, back to back
int launch_compact_scan(const unsigned *counts, unsigned long long *offsets, int n, int n_arrays, unsigned long long *totals, void *stream)
{
    hipLaunchKernelGGL(k_compact_scan, dim3(n_arrays), dim3(1024), 0, (hipStream_t)stream, counts, offsets, n, totals);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Consumers of the SEGMENTED clouds the fused kernel writes (k_fused<..., CMODE = 2>): a view's cloud is the concatenation of
// its segments' first `count` points.  One wave per segment, one point (12 bytes) per lane and step.
// ------------------------------------------------------------------------------------------------
// Exclusive scan of one view's segment counts (1024-thread blocks), behind every segmented launch: it is on the critical path of
// sl3d_run_clouds, so it is written for latency.  A view's segments are scanned by SL3D_SCAN_PARTS blocks (one block per view was a
// latency chain of ~10 us on a 256-CU machine): block (view, part) SUMS the counts of the parts in front of it -- the same
// coalesced reads every one of them does anyway, at most n dwords from the L2 -- and scans its own part from that carry; no block
// waits for another.  The last part's block leaves the view's total in the mapped host word sl3d_get_cloud_counts reads.
// ONE memory round trip per block (round 4): it requests its own counts -- 4 consecutive ones per thread, one 16-byte load, a wave
// reads 1 KB contiguous -- AND the counts in front of its part in the same breath, sums the latter, scans the former in registers
// (the 4 entries, 6 wave shuffles, the 16 wave totals through LDS: one block barrier per chunk) and writes 4 offsets per thread
// (32 contiguous bytes); the next chunk of a long part travels while the current one is scanned.  (Until then: the carry first,
// then the chunk through a padded LDS array with five barriers -- 6.1 us for the 8,100 counts of one 1080p view;
// profiles/r04_seg_scan_ab.txt.  Rounds 2-3: k_compact_scan, 32 strided dwords per thread, 14.3 us for 16 x 32,400 counts; one
// block per view with runs of 32: 10.2 us.)
#define SL3D_SCAN_RUN 4
#define SL3D_SCAN_PARTS 8
__global__ __launch_bounds__(1024) void k_seg_scan(const unsigned *__restrict__ counts, unsigned long long *__restrict__ offsets, int n,
                                                   unsigned long long *total)
{
    const int view = (int)blockIdx.y, part = (int)blockIdx.x;
    counts += (size_t)view * n;   // (n = 4 * tiles: every row of counts is 16-byte aligned, every row of offsets 32-byte aligned)
    offsets += (size_t)view * n;
    constexpr int CHUNK = 1024 * SL3D_SCAN_RUN;
    // parts are whole chunks, so that every chunk of a part is scanned by the same code path
    const int part_len = (((n + SL3D_SCAN_PARTS - 1) / SL3D_SCAN_PARTS + CHUNK - 1) / CHUNK) * CHUNK;
    const int begin = min(part * part_len, n), end = min(begin + part_len, n);
    __shared__ unsigned long long s_part[16];
    __shared__ unsigned s_wave[2][16];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint4 zero = {0u, 0u, 0u, 0u};
    auto mine = [&](int base) { return base + SL3D_SCAN_RUN * t < end ? *(const uint4 *)(counts + base + SL3D_SCAN_RUN * t) : zero; };
    uint4 c = mine(begin);
    unsigned long long carry;
    {   // the carry into this part: the sum of everything in front of it (requested together with the part's first chunk)
        unsigned long long acc = 0ull;
        for (int i = SL3D_SCAN_RUN * t; i < begin; i += CHUNK) {
            const uint4 f = *(const uint4 *)(counts + i);
            acc += (unsigned long long)f.x + f.y + f.z + f.w;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) s_part[wave] = acc;
        __syncthreads();
        carry = 0ull;
#pragma unroll
        for (int w = 0; w < 16; w++) carry += s_part[w];
    }
    int buf = 0;
    for (int base = begin;; base += CHUNK, buf ^= 1) {
        const uint4 next = base + CHUNK < end ? mine(base + CHUNK) : zero;  // (the next chunk travels while this one is scanned)
        const unsigned e1 = c.x, e2 = e1 + c.y, e3 = e2 + c.z, run = e3 + c.w;
        unsigned incl = run;  // inclusive scan of the run totals over the wave, then over the 16 waves
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) s_wave[buf][wave] = incl;
        __syncthreads();  // (two buffers: the next chunk's totals do not overwrite what a slower wave still reads)
        unsigned wbase = 0, chunk_total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const unsigned v = s_wave[buf][w];
            wbase += w < wave ? v : 0u;
            chunk_total += v;
        }
        if (base + SL3D_SCAN_RUN * t < end) {
            const unsigned long long o = carry + (unsigned long long)(wbase + (incl - run));
            ulonglong2 *dst = (ulonglong2 *)(offsets + base + SL3D_SCAN_RUN * t);
            dst[0] = make_ulonglong2(o, o + e1);
            dst[1] = make_ulonglong2(o + e2, o + e3);
        }
        carry += (unsigned long long)chunk_total;
        if (base + CHUNK >= end) break;
        c = next;
    }
    if (t == 0 && part == SL3D_SCAN_PARTS - 1) total[view] = carry;
}

int launch_seg_scan(const KParams &P, int first_view, int n_views, void *stream)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_seg_scan, dim3(SL3D_SCAN_PARTS, (unsigned)n_views), dim3(1024), 0, (hipStream_t)stream,
                       P.seg_counts + (size_t)first_view * P.n_segs, P.seg_offsets + (size_t)first_view * P.n_segs, P.n_segs,
                       P.cloud_totals + first_view);
    return (int)hipGetLastError();
}

// N3's transform of one point, 9/register_point_clouds.cpp:109-117, in the reference's types: p -= t (float, :109-111), p = R * p with the
// float GEMM of cvMatMul (:113: double accumulator, k ascending, rounded to float on store), then p += t (float, :115-117) -- which
// the CALLER adds at its store (with the sum in here k_register's registers are numbered differently: profiles/r08_cloud_consumers_identity.txt).
// R = rotation about Y: rows (r00, 0, r02, 0), (0, 1, 0, 0), (r20, 0, r22, 0); the products with exact zeros add nothing
__device__ __forceinline__ float3 rotated_about(float px, float py, float pz, float r00, float r02, float r20, float r22, float tx, float ty, float tz)
{
    const float x = px - tx, y = py - ty, z = pz - tz;
    const float X = (float)(((double)r00 * (double)x + 0.0 * (double)y) + (double)r02 * (double)z);
    const float Y = (float)((0.0 * (double)x + 1.0 * (double)y) + 0.0 * (double)z);
    const float Z = (float)(((double)r20 * (double)x + 0.0 * (double)y) + (double)r22 * (double)z);
    return make_float3(X, Y, Z);
}

// REG = false: plain copy (closing the gaps); true: the rigid transform of k_register on the way (9/register_point_clouds.cpp:109-117)
// SCAN = false: the segments' offsets come from k_seg_scan.  true: the consumer scans on entry -- a block (4 segments) adds up the
// counts in front of it itself (at most n_segs dwords from the L2, 16 bytes per lane and step: what every part of k_seg_scan does
// for its carry), so a launch of a few views needs NO scan launch between the fused kernel and its consumer; the last block leaves
// the view's total in total_out[view] (host memory mapped into the device: sl3d_get_cloud_counts' word).  Points whose index in the
// closed cloud is >= capacity are not written (a destination smaller than the cloud takes its first `capacity` points).
template <bool REG, bool SCAN>
__global__ __launch_bounds__(256) void k_seg_close(const float *__restrict__ seg_xyz, const unsigned *__restrict__ counts,
                                                   const unsigned long long *__restrict__ offsets, int n_segs, size_t src_view_stride, float *dst,
                                                   size_t dst_view_stride, float r00, float r02, float r20, float r22, float tx, float ty, float tz,
                                                   unsigned long long *total_out, unsigned long long capacity)
{
    typedef float f32x3 __attribute__((ext_vector_type(3), aligned(4)));
    const int wave = (int)(threadIdx.x >> 6);
    const int seg = blockIdx.x * 4 + wave, lane = (int)(threadIdx.x & 63u), v = blockIdx.y;
    const unsigned cnt = seg < n_segs ? counts[(size_t)v * n_segs + seg] : 0u;
    unsigned long long off;
    if (SCAN) {
        __shared__ unsigned long long s_front[4];
        __shared__ unsigned s_cnt[4];
        const unsigned *cv = counts + (size_t)v * n_segs;
        const int n_front = (int)blockIdx.x * 4;  // (whole 16-byte groups: n_segs = 4 * tiles, every row of counts is 16-byte aligned)
        unsigned long long acc = 0ull;
        for (int i = 4 * (int)threadIdx.x; i < n_front; i += 1024) {
            const uint4 f = *(const uint4 *)(cv + i);
            acc += (unsigned long long)f.x + f.y + f.z + f.w;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) {
            s_front[wave] = acc;
            s_cnt[wave] = cnt;
        }
        __syncthreads();
        off = s_front[0] + s_front[1] + s_front[2] + s_front[3];
#pragma unroll
        for (int w = 0; w < 4; w++) off += w < wave ? s_cnt[w] : 0u;
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 192) total_out[v] = off + cnt;  // (wave 3 of the last block: everything in front + its own)
    } else {
        if (seg >= n_segs) return;
        off = offsets[(size_t)v * n_segs + seg];
    }
    // (a 3-float vector type is PADDED to 16 bytes: points are addressed through float pointers, 12 bytes apart)
    const float *src = seg_xyz + 3 * ((size_t)v * src_view_stride + (size_t)seg * SL3D_SEG_POINTS);
    float *out = dst + 3 * ((size_t)v * dst_view_stride + (size_t)off);
    const unsigned long long room = off < capacity ? capacity - off : 0ull;
    const unsigned n = SCAN ? (unsigned)(room < cnt ? room : cnt) : cnt;
    for (unsigned i = (unsigned)lane; i < n; i += 64u) {
        f32x3 p = *(const f32x3 *)(src + 3 * (size_t)i);
        if (REG) {
            const float3 q = rotated_about(p.x, p.y, p.z, r00, r02, r20, r22, tx, ty, tz);
            p.x = q.x + tx; p.y = q.y + ty; p.z = q.z + tz;
        }
        *(f32x3 *)(out + 3 * (size_t)i) = p;
    }
}

// views [first_view, first_view + n_views) of the segmented clouds, as SegClose (sl3d_internal.h) says.  Both at once -- a scan on entry
// and a rotation -- is not a kernel of the library (k_seg_close<true, true> is not instantiated)
int launch_seg_close(const KParams &P, int first_view, int n_views, const SegClose &c, void *stream)
{
    (void)hipGetLastError();
    if (c.scan && c.R4) return (int)hipErrorInvalidValue;
    const auto kernel = c.R4 ? k_seg_close<true, false> : c.scan ? k_seg_close<false, true> : k_seg_close<false, false>;
    const float none[4] = {0.f, 0.f, 0.f, 0.f}, *R4 = c.R4 ? c.R4 : none;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((P.n_segs + 3) / 4), (unsigned)n_views), dim3(256), 0, (hipStream_t)stream,
                       P.clouds + 3 * (size_t)first_view * P.px_view_stride, P.seg_counts + (size_t)first_view * P.n_segs,
                       c.scan ? (const unsigned long long *)nullptr : P.seg_offsets + (size_t)first_view * P.n_segs, P.n_segs, P.px_view_stride, c.dst,
                       c.dst_view_stride_points, R4[0], R4[1], R4[2], R4[3], c.tx, c.ty, c.tz,
                       c.scan ? P.cloud_totals + first_view : (unsigned long long *)nullptr, c.scan ? c.capacity_points : ~0ull);
    return (int)hipGetLastError();
}

// N3: turntable registration of a contiguous cloud, 9/register_point_clouds.cpp:83-128 (rotated_about: the arithmetic per point)
__global__ __launch_bounds__(256) void k_register(const float *in, float *out, long n, float r00, float r02, float r20, float r22,
                                                  float tx, float ty, float tz)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float3 q = rotated_about(in[3 * i + 0], in[3 * i + 1], in[3 * i + 2], r00, r02, r20, r22, tx, ty, tz);
    out[3 * i + 0] = q.x + tx;
    out[3 * i + 1] = q.y + ty;
    out[3 * i + 2] = q.z + tz;
}

int launch_register(const float *in, float *out, long n, const float R4[4], float tx, float ty, float tz, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_register, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, R4[0], R4[1], R4[2], R4[3], tx, ty, tz);
    return (int)hipGetLastError();
}

}  // namespace sl3d
