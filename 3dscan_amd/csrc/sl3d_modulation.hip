// sl3d_modulation.hip -- gfx950 (MI355X, wave64) kernels of the fringe-modulation test (sl3d_modulation.h: gamma and the selection):
//   k_modulation_select : sl3d_set_masks_modulated -- the final 0/1 selection of each view of a call, written over the frame region of
//                         the view's slot of the mask staging plane, where k_mask_prepare or a MASKIN launch of k_fused picks it up
//   k_modulation_gamma  : sl3d_get_modulation -- gamma of one axis as a float plane
// One lane = one quad (4 pixels) of a row: dword loads of the fringe planes (rows start on 16-byte boundaries, pitch is a multiple of
// 16), integer d, e and sums, sqrtf and a correctly rounded division per pixel, one dword (select) or 16-byte (gamma) store.
// Compiled with -ffp-contract=off -fno-fast-math like every translation unit: gamma is bit exact with the host's float arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_internal.h"
#include "sl3d_modulation.h"

namespace sl3d {

// the three fringe bytes of pixel k of a quad, of one axis, as gamma
__device__ __forceinline__ float quad_gamma(unsigned f0, unsigned f1, unsigned f2, int k)
{
    return mod_gamma((int)((f0 >> (8 * k)) & 0xffu), (int)((f1 >> (8 * k)) & 0xffu), (int)((f2 >> (8 * k)) & 0xffu));
}

// Views first_view + blockIdx.y; lane t of a view owns quad (t mod qpr) of window row (t / qpr), qpr = quads that hold window pixels.
// staging: slot k (mask_view_stride bytes apart) holds view first_view + k's mask in its frame region (plane rows 2.., bytes
// SL3D_MASK_LPAD..) when has_mask; the selection bytes replace it there.  Bytes of the last quad behind the window's last column are
// written as 0 (they lie outside the region, where the staging plane is 0).
__global__ __launch_bounds__(256) void k_modulation_select(const KParams P, int first_view, uint8_t *__restrict__ staging, int has_mask, double thr)
{
    const int qpr = (P.W + 3) >> 2;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const int row = (int)(t / (unsigned)qpr), q = (int)(t - (unsigned)row * (unsigned)qpr);
    if (row >= P.H) return;
    const int view = first_view + (int)blockIdx.y;
    const uint8_t *fv = P.frames + (size_t)view * P.view_stride + (size_t)row * P.pitch + 4 * q;
    const uint8_t *fh = fv + (size_t)(P.F + 2 * P.Nv) * P.plane_stride;
    const unsigned v0 = *(const unsigned *)fv, v1 = *(const unsigned *)(fv + P.plane_stride), v2 = *(const unsigned *)(fv + 2 * P.plane_stride);
    const unsigned h0 = *(const unsigned *)fh, h1 = *(const unsigned *)(fh + P.plane_stride), h2 = *(const unsigned *)(fh + 2 * P.plane_stride);
    unsigned *dst = (unsigned *)(staging + (size_t)blockIdx.y * P.mask_view_stride + (size_t)(row + SL3D_MASK_HALO) * P.mpitch + SL3D_MASK_LPAD + 4 * q);
    const unsigned m = has_mask ? *dst : 0x01010101u;
    const int in_window = P.W - 4 * q;  // pixels of the quad inside the window (>= 1)
    unsigned out = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sel = mod_select(((m >> (8 * k)) & 0xffu) == 1u, quad_gamma(v0, v1, v2, k), quad_gamma(h0, h1, h2, k), thr);
        out |= (unsigned)(sel & (k < in_window)) << (8 * k);
    }
    *dst = out;
}

// the same for a one-axis context (SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL): the test of the coded axis alone -- mod_select with that axis's
// gamma in both places -- and no plane of the other axis read
__global__ __launch_bounds__(256) void k_modulation_select_one(const KParams P, int first_view, uint8_t *__restrict__ staging, int has_mask, double thr,
                                                               int axis)
{
    const int qpr = (P.W + 3) >> 2;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const int row = (int)(t / (unsigned)qpr), q = (int)(t - (unsigned)row * (unsigned)qpr);
    if (row >= P.H) return;
    const int view = first_view + (int)blockIdx.y;
    const uint8_t *f = P.frames + (size_t)view * P.view_stride + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride + (size_t)row * P.pitch + 4 * q;
    const unsigned f0 = *(const unsigned *)f, f1 = *(const unsigned *)(f + P.plane_stride), f2 = *(const unsigned *)(f + 2 * P.plane_stride);
    unsigned *dst = (unsigned *)(staging + (size_t)blockIdx.y * P.mask_view_stride + (size_t)(row + SL3D_MASK_HALO) * P.mpitch + SL3D_MASK_LPAD + 4 * q);
    const unsigned m = has_mask ? *dst : 0x01010101u;
    const int in_window = P.W - 4 * q;  // pixels of the quad inside the window (>= 1)
    unsigned out = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float g = quad_gamma(f0, f1, f2, k);
        const int sel = mod_select(((m >> (8 * k)) & 0xffu) == 1u, g, g, thr);
        out |= (unsigned)(sel & (k < in_window)) << (8 * k);
    }
    *dst = out;
}

// gamma of axis `axis` of `view`: out[row * pitch + col] (the pitch's padding columns hold gamma of whatever the padding bytes are)
__global__ __launch_bounds__(256) void k_modulation_gamma(const KParams P, int view, int axis, float *__restrict__ out)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int qpr = (P.W + 3) >> 2;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const int row = (int)(t / (unsigned)qpr), q = (int)(t - (unsigned)row * (unsigned)qpr);
    if (row >= P.H) return;
    const uint8_t *f = P.frames + (size_t)view * P.view_stride + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride + (size_t)row * P.pitch + 4 * q;
    const unsigned f0 = *(const unsigned *)f, f1 = *(const unsigned *)(f + P.plane_stride), f2 = *(const unsigned *)(f + 2 * P.plane_stride);
    f32x4 g;
    g.x = quad_gamma(f0, f1, f2, 0);
    g.y = quad_gamma(f0, f1, f2, 1);
    g.z = quad_gamma(f0, f1, f2, 2);
    g.w = quad_gamma(f0, f1, f2, 3);
    *(f32x4 *)(out + (size_t)row * P.pitch + 4 * q) = g;
}

static unsigned modulation_blocks(const KParams &P) { return (unsigned)(((long)((P.W + 3) >> 2) * P.H + 255) / 256); }

int launch_modulation_select(const KParams &P, int first_view, int n_views, uint8_t *staging, bool has_mask, double thr, void *stream)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_modulation_select, dim3(modulation_blocks(P), (unsigned)n_views), dim3(256), 0, (hipStream_t)stream, P, first_view, staging,
                       has_mask ? 1 : 0, thr);
    return (int)hipGetLastError();
}

int launch_modulation_select_one(const KParams &P, int first_view, int n_views, uint8_t *staging, bool has_mask, double thr, int axis, void *stream)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_modulation_select_one, dim3(modulation_blocks(P), (unsigned)n_views), dim3(256), 0, (hipStream_t)stream, P, first_view, staging,
                       has_mask ? 1 : 0, thr, axis);
    return (int)hipGetLastError();
}

int launch_modulation_gamma(const KParams &P, int view, int axis, float *out, void *stream)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_modulation_gamma, dim3(modulation_blocks(P)), dim3(256), 0, (hipStream_t)stream, P, view, axis, out);
    return (int)hipGetLastError();
}

}  // namespace sl3d
