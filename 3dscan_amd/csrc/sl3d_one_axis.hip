// sl3d_one_axis.hip -- gfx950 (MI355X, wave64): the one-axis scan of a timed context in ONE launch (SL3D_FLAG_ONLY_VERTICAL /
// SL3D_FLAG_ONLY_HORIZONTAL with SL3D_FLAG_SUBPIXEL, without SL3D_FLAG_KEEP_STAGES).  k_one_axis<AXIS, ANCHOR> leaves in the
// points and valid planes of the launch's views, bit for bit, what k_wrap and k_unwrap of axis AXIS, k_corr_one and k_subpixel_one leave
// there on a SL3D_FLAG_KEEP_STAGES context: per pixel the frames of ONE pattern direction -> stage 3 (wrapped_phase) -> stage 4 (Gray
// decode, shift_pi, unwrap_value) -> stage 5 (correspond of that axis: the merged valid byte; correspond_arg or, with ANCHOR,
// anchor_coordinate: the continuous coordinate) -> one_axis_project -> one_axis_solve, the exactly determined ray-plane intersection
// (sl3d_one_axis.h).  Every arithmetic step is the helper the staged kernels call, with the arguments they call it with.  No frame of the
// other axis is read; there is no residual.
//   shape   k_subpixel_fused's: a lane owns the 4 consecutive pixels of one dword of every u8 plane (the pitch is a multiple of 16: a quad
//           never straddles a row) and walks the views of the launch itself; the camera side (u, v) of a pixel is formed once per pixel
//           and launch, for the pixels some view of the launch selects.  The Gray planes are a run-time loop (0..16).
//   memory  per pixel and view: F + 2 N frame bytes of the coded axis and the prepared valid byte (`band`, read twice: once for the
//           camera side) in, 12 B of points and the valid byte out -- 16-byte stores per lane, streaming.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_anchor.h"
#include "sl3d_device.h"
#include "sl3d_internal.h"
#include "sl3d_one_axis.h"

namespace sl3d {

#define SL3D_OA_BLOCK 256  // lanes per block: 1024 pixels

typedef float oa_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned oa_load(const uint8_t *p) { return __builtin_nontemporal_load((const unsigned *)p); }
__device__ __forceinline__ unsigned oa_byte(unsigned w, int k) { return (w >> (8 * k)) & 0xffu; }

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (k_subpixel_fused)
template <int AXIS, bool ANCHOR>
__global__ __launch_bounds__(SL3D_OA_BLOCK) void k_one_axis(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views)
{
    const CONST_AS DevCal &C = *opaque_const(Cp);
    const size_t px0 = 4 * ((size_t)blockIdx.x * SL3D_OA_BLOCK + threadIdx.x);  // first pixel of the lane's quad, padding columns included
    if (px0 >= P.px_view_stride) return;                                         // (a multiple of 16: a quad is inside a view or outside it)
    const unsigned lane_off = (unsigned)px0;
    const int row = (int)(px0 / (size_t)P.pitch), col = (int)(px0 - (size_t)row * P.pitch);
    const int gx0 = P.col0 + col, gy = P.row0 + row;
    const bool decodes = P.F != 5;  // check_I_mod_criteria, 3/wrapped_phase.cpp:106-115: with 5 steps nothing is valid (k_wrap)
    const int N = AXIS == 0 ? P.Nv : P.Nh, fw = AXIS == 0 ? P.fwv : P.fwh, extent = AXIS == 0 ? P.PW : P.PH;
    // the camera side of the pixels some view of the launch selects
    unsigned need = 0u;
    if (decodes)
        for (int vi = 0; vi < n_views; vi++) need |= mask_quad_bits(load_mask_quad(P, first_view + vi, lane_off));
    double u[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u[k] = v[k] = 0.0;
        if (need >> k & 1u) undistort_reproject((double)(gx0 + k), (double)gy, C.cam, u[k], v[k]);
    }
    const AtanK K = atan_consts<false>();
    const float nanv = __builtin_nanf("");
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const size_t px = (size_t)view * P.px_view_stride + px0;
        const unsigned bits = decodes ? mask_quad_bits(load_mask_quad(P, view, lane_off)) : 0u;
        float out[12];
#pragma unroll
        for (int j = 0; j < 12; j++) out[j] = nanv;
        unsigned valid = 0u;
        if (bits) {
            // the planes of the coded axis alone: F fringe planes, then N Gray planes and their N inverses
            const uint8_t *fr = P.frames + (size_t)view * P.view_stride + px0 + (size_t)(AXIS == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride;
            const unsigned i0 = oa_load(fr), i1 = oa_load(fr + P.plane_stride), i2 = oa_load(fr + 2 * P.plane_stride);
            const unsigned i3 = P.F == 4 ? oa_load(fr + 3 * P.plane_stride) : 0u;
            const uint8_t *gr = fr + (size_t)P.F * P.plane_stride;
            unsigned b[4] = {0u, 0u, 0u, 0u};
            int code[4] = {0, 0, 0, 0};
#pragma unroll 2
            for (int i = 0; i < N; i++) {
                const unsigned pos = oa_load(gr + (size_t)i * P.plane_stride), inv = oa_load(gr + (size_t)(N + i) * P.plane_stride);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    b[k] ^= oa_byte(pos, k) >= oa_byte(inv, k) ? 1u : 0u;  // 4/phase_unwrap.cpp:183, :187-191
                    code[k] = code[k] * 2 + (int)b[k];                     // :193
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(bits >> k & 1u)) continue;  // the valid byte of stage 3's boundary removal
                const float phi = wrapped_phase<false>(P.F, oa_byte(i0, k), oa_byte(i1, k), oa_byte(i2, k), oa_byte(i3, k), nullptr, K);
                const int pos = AXIS == 0 ? gx0 + k : gy, full = AXIS == 0 ? P.fullW : P.fullH;
                const bool in_range = pos >= 1 && pos <= full - 2;  // :285 / :304
                const float w = in_range ? shift_pi(phi) : 0.f;
                const float unw = in_range ? unwrap_value(w, code[k]) : 0.f;
                long c;
                double d;
                if (!correspond(unw, fw, extent, c, d)) continue;  // k_corr_one
                // (where the formula does not apply the coordinate stays as it is: k_subpixel_one<AXIS, true>)
                const double s = ANCHOR && anchor_applies(N, pos, full) ? anchor_coordinate(w, code[k], fw, P.F) : correspond_arg(unw, fw);
                const double t = one_axis_project(s, C.proj.K[AXIS == 0 ? 0 : 4], AXIS == 0 ? C.proj.ifx : C.proj.ify, AXIS == 0 ? C.proj.cx : C.proj.cy);
                double X[3];
                one_axis_solve(C.Ac, C.Ap, AXIS, u[k], v[k], t, X);
                out[3 * k + 0] = (float)X[0];
                out[3 * k + 1] = (float)X[1];
                out[3 * k + 2] = (float)X[2];
                valid |= 1u << (8 * k);
            }
        }
        oa_f32x4 *pts = (oa_f32x4 *)(P.points + 3 * px);
#pragma unroll
        for (int j = 0; j < 3; j++) __builtin_nontemporal_store((oa_f32x4){out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]}, pts + j);
        *(unsigned *)(P.valid + px) = valid;
    }
}

int launch_one_axis(const KParams &P, const DevCal *C, int axis, int first_view, int n_views, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const size_t quads = P.px_view_stride / 4;
    const dim3 grid((unsigned)((quads + SL3D_OA_BLOCK - 1) / SL3D_OA_BLOCK));
#define SL3D_OA(AXIS, ANCHOR) hipLaunchKernelGGL((k_one_axis<AXIS, ANCHOR>), grid, dim3(SL3D_OA_BLOCK), 0, (hipStream_t)stream, P, C, first_view, n_views)
    if (axis == 0) { if (anchor) SL3D_OA(0, true); else SL3D_OA(0, false); }
    else { if (anchor) SL3D_OA(1, true); else SL3D_OA(1, false); }
#undef SL3D_OA
    return (int)hipGetLastError();
}

}  // namespace sl3d
