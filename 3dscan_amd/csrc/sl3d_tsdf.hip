// sl3d_tsdf.hip -- gfx950 (MI355X, wave64) kernels of the TSDF volume (sl3d_tsdf_integrate / sl3d_tsdf_extract; the rule:
// include/sl3d_tsdf.h, its arithmetic: sl3d_tsdf.h):
//   k_tsdf_depth     : the pre-pass of an integration: per view of the call and pixel of the window the camera depth of the pixel's
//                      point as a double, NaN where the pixel is not usable -- a sample then costs four 8-byte gathers instead of four
//                      of a byte and four of 12 bytes
//   k_tsdf_integrate : a lane per voxel, v = 256 b + t, so that i runs along the wave and neighbouring lanes project to neighbouring
//                      pixels.  The loop over the call's views is inside the kernel: sum and weight are read once, live in registers
//                      across the views and are written once.  The views' (c_m, s_m) come from a small table indexed by the loop
//                      counter alone (uniform loads), the camera and the volume from the kernel arguments.  Each sample gathers four
//                      doubles from the view's depth plane.  No atomics on the volume, no LDS but the block sums.
//   k_tsdf_count     : per 1024-voxel block (a lane 4 consecutive voxels, sl3d_block.h) the crossings on the three + edges of its
//                      known voxels, and the known voxels
//   k_compact_scan (sl3d_clouds.hip) : the blocks' offsets and the total
//   k_tsdf_scatter   : walks the block again, ranks every crossing by wave prefixes and writes xyz, normal and edge at its rank: the
//                      output is in ascending (v0, axis)
// The counts -- samples taken, voxels with weight > 0, known voxels -- are integer sums: a wave reduction, the four waves through LDS,
// then one 64-bit atomicAdd per block and word into words the launcher cleared on the stream.  Integer atomics only: the result does
// not depend on the order of arrival.  Every loop is bounded by an argument.
// -DSL3D_TSDF_GATHER (measurement builds, tools/tsdf_timing.py) takes the other route of the depth lookup: the pre-pass is skipped and a
// sample gathers four valid bytes and four points itself.  The same bits, 1.05 to 2.3 times the time; no runtime path of the
// library.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_tsdf.h"

namespace sl3d {

// (i, j, k) of voxel v (below 2^28)
__device__ __forceinline__ void tsdf_ijk(unsigned v, const int *n, int *ijk)
{
    const unsigned nx = (unsigned)n[0], ny = (unsigned)n[1], row = v / nx;
    ijk[0] = (int)(v - row * nx);
    ijk[2] = (int)(row / ny);
    ijk[1] = (int)(row - (unsigned)ijk[2] * ny);
}

// the depth planes of the call's views: z[view][row][pitch], the window's pixels only (a sample reads no other)
__global__ __launch_bounds__(256) void k_tsdf_depth(TsdfFrame frame, size_t px_view_stride, AlignCam cam, double *__restrict__ z)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x), r = (int)blockIdx.y;
    if (c >= frame.W) return;
    const size_t px = (size_t)blockIdx.z * px_view_stride + (size_t)r * (size_t)frame.pitch + (size_t)c;
    z[px] = tsdf_pixel_depth(&frame, px, &cam);
}

#ifdef SL3D_TSDF_GATHER
#define TSDF_SAMPLE(X, a, cam, f, m, T, q) tsdf_sample(X, a, cam, f, T, q)
#else
#define TSDF_SAMPLE(X, a, cam, f, m, T, q) tsdf_sample_plane(X, a, cam, f, zplane + (size_t)(m) * px_view_stride, T, q)
#endif

// frame: the planes of the call's first view, the views px_view_stride pixels apart; turns: [n_views]; n_vox = nx * ny * nz
__global__ __launch_bounds__(256) void k_tsdf_integrate(TsdfFrame frame, size_t px_view_stride, AlignCam cam, TsdfVolume vol, double tx, double tz,
                                                        const TsdfTurn *__restrict__ turns, int n_views, int32_t *__restrict__ sum,
                                                        uint32_t *__restrict__ weight, unsigned n_vox, unsigned long long *__restrict__ words, const double *__restrict__ zplane)
{
    __shared__ unsigned s_taken[4], s_occ[4];
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    unsigned taken = 0, occupied = 0;
    if (v < n_vox) {
        int ijk[3];
        tsdf_ijk(v, vol.n, ijk);
        const double X[3] = {tsdf_centre(ijk[0], vol.L, vol.o[0]), tsdf_centre(ijk[1], vol.L, vol.o[1]), tsdf_centre(ijk[2], vol.L, vol.o[2])};
        int32_t s = sum[v];
        uint32_t w = weight[v];
#pragma unroll 1
        for (int m = 0; m < n_views; m++) {
            const TsdfTurn t = turns[m];
            const AlignPass a = {t.c, -t.s, tx, tz, 0.0, 0.0, 0.0, 0.0};
            TsdfFrame f = frame;
            f.valid += (size_t)m * px_view_stride;
            f.points += 3 * (size_t)m * px_view_stride;
            int32_t q;
            if (TSDF_SAMPLE(X, &a, &cam, &f, m, vol.T, &q)) s += q, w++, taken++;
        }
        sum[v] = s;
        weight[v] = w;
        occupied = w > 0;
    }
    BLOCK_SUM(taken, s_taken);
    BLOCK_SUM(occupied, s_occ);
    if (threadIdx.x == 0) {
        const unsigned n = BLOCK_SUM_TOTAL(s_taken), o = BLOCK_SUM_TOTAL(s_occ);
        if (n) atomicAdd(words + TSDF_WORD_SAMPLES, (unsigned long long)n);
        if (o) atomicAdd(words + TSDF_WORD_OCCUPIED, (unsigned long long)o);
    }
}

// Which of the three + edges of voxel v carry a crossing (bits 0-2), and is v known (bit 3).  t[axis]: the crossing's parameter
__device__ __forceinline__ unsigned tsdf_edges(const TsdfPlanes &P, const int *n, unsigned v, unsigned n_vox, int *ijk, double *t)
{
    if (v >= n_vox || !tsdf_known(&P, v)) return 0u;
    tsdf_ijk(v, n, ijk);
    unsigned bits = 8u;
#pragma unroll
    for (int axis = 0; axis < 3; axis++)
        if (tsdf_crossing(&P, n, v, ijk, axis, &t[axis])) bits |= 1u << axis;
    return bits;
}

// a block of 256 lanes owns 1024 consecutive voxels, a lane 4 (sl3d_block.h)
__global__ __launch_bounds__(256) void k_tsdf_count(TsdfPlanes P, TsdfVolume vol, unsigned n_vox, unsigned *__restrict__ block_counts,
                                                    unsigned long long *__restrict__ words)
{
    __shared__ unsigned s_cnt[4], s_known[4];
    const unsigned v0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    unsigned c = 0, known = 0;
#pragma unroll 1
    for (unsigned k = 0; k < 4; k++) {
        int ijk[3];
        double t[3];
        const unsigned bits = tsdf_edges(P, vol.n, v0 + k, n_vox, ijk, t);
        c += __popc(bits & 7u);
        known += bits >> 3;
    }
    BLOCK_SUM(c, s_cnt);
    BLOCK_SUM(known, s_known);
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
        const unsigned kn = BLOCK_SUM_TOTAL(s_known);
        if (kn) atomicAdd(words + TSDF_WORD_KNOWN, (unsigned long long)kn);
    }
}

__global__ __launch_bounds__(256) void k_tsdf_scatter(TsdfPlanes P, TsdfVolume vol, unsigned n_vox, const unsigned long long *__restrict__ block_offsets,
                                                      float *__restrict__ xyz, float *__restrict__ normals, int32_t *__restrict__ edge)
{
    __shared__ unsigned s_wave[4];
    const unsigned v0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    unsigned all = 0;  // three bits a voxel
#pragma unroll 1
    for (unsigned k = 0; k < 4; k++) {
        int ijk[3];
        double t[3];
        all |= (tsdf_edges(P, vol.n, v0 + k, n_vox, ijk, t) & 7u) << (3u * k);
    }
    const unsigned c = __popc(all), incl = wave_prefix(c, s_wave);
    unsigned long long at = block_offsets[blockIdx.x] + (waves_before(s_wave, 0u) + (incl - c));
#pragma unroll 1
    for (unsigned k = 0; k < 4; k++) {
        const unsigned bits = all >> (3u * k) & 7u;
        if (!bits) continue;
        int ijk[3];
        double t[3];
        (void)tsdf_edges(P, vol.n, v0 + k, n_vox, ijk, t);
#pragma unroll
        for (int axis = 0; axis < 3; axis++)
            if (bits >> axis & 1u) {
                float p[3], g[3];
                tsdf_edge(&P, &vol, v0 + k, ijk, axis, t[axis], p, g);
                for (int b = 0; b < 3; b++) xyz[3 * at + b] = p[b], normals[3 * at + b] = g[b];
                edge[at] = (int32_t)(3u * (v0 + k) + (unsigned)axis);
                at++;
            }
    }
}

static unsigned tsdf_voxels(const TsdfVolume &vol) { return (unsigned)vol.n[0] * (unsigned)vol.n[1] * (unsigned)vol.n[2]; }

// the memset of the call's two words, the depth planes and the integration of views [first_view, first_view + n_views) -- turns: their
// rotations, on the device; depth: n_views * px_view_stride doubles
int launch_tsdf_integrate(const KParams &P, int first_view, int n_views, const AlignCam &cam, const TsdfVolume &vol, double tx, double tz,
                          const TsdfTurn *turns, double *depth, int32_t *sum, uint32_t *weight, unsigned long long *words, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(words + TSDF_WORD_SAMPLES, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    (void)hipGetLastError();
    const ViewPlanes in = view_planes(P, first_view);
    const TsdfFrame frame = {in.valid, in.points, P.W, P.H, P.pitch, P.col0, P.row0};
    const unsigned n_vox = tsdf_voxels(vol);
#ifndef SL3D_TSDF_GATHER
    hipLaunchKernelGGL(k_tsdf_depth, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.H, (unsigned)n_views), dim3(256), 0, st, frame, P.px_view_stride, cam,
                       depth);
#endif
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((n_vox + 255u) / 256u), dim3(256), 0, st, frame, P.px_view_stride, cam, vol, tx, tz, turns, n_views, sum,
                       weight, n_vox, words, (const double *)depth);
    return (int)hipGetLastError();
}

// the memset of the extraction's two words, k_tsdf_count and k_compact_scan: words[TSDF_WORD_CROSSINGS] is the total once the stream has drained
int launch_tsdf_count(const TsdfPlanes &planes, const TsdfVolume &vol, const CompactScratch &s, unsigned long long *words, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(words + TSDF_WORD_KNOWN, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    (void)hipGetLastError();
    const unsigned n_vox = tsdf_voxels(vol), nb = (n_vox + 1023u) / 1024u;
    hipLaunchKernelGGL(k_tsdf_count, dim3(nb), dim3(256), 0, st, planes, vol, n_vox, s.cnt, words);
    (void)launch_compact_scan(s.cnt, s.off, (int)nb, 1, words + TSDF_WORD_CROSSINGS, st);
    return (int)hipGetLastError();
}

// ... and the scatter behind them, into arrays of at least that total
int launch_tsdf_scatter(const TsdfPlanes &planes, const TsdfVolume &vol, const CompactScratch &s, float *xyz, float *normals, int32_t *edge, void *stream)
{
    const unsigned n_vox = tsdf_voxels(vol), nb = (n_vox + 1023u) / 1024u;
    hipLaunchKernelGGL(k_tsdf_scatter, dim3(nb), dim3(256), 0, (hipStream_t)stream, planes, vol, n_vox, s.off, xyz, normals, edge);
    return (int)hipGetLastError();
}

}  // namespace sl3d
