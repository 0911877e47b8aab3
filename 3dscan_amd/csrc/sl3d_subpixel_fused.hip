// sl3d_subpixel_fused.hip -- gfx950 (MI355X, wave64): the sub-pixel scan of a timed context in ONE launch (SL3D_FLAG_SUBPIXEL without
// SL3D_FLAG_KEEP_STAGES).  k_subpixel_fused leaves in the points, valid and residual planes of the launch's views, bit for
// bit, what k_wrap, k_unwrap (both axes), k_corr and k_subpixel(+inf) leave there on a SL3D_FLAG_KEEP_STAGES context -- without any of
// the stage planes between them: per pixel the frames -> stage 3 (wrapped_phase) -> stage 4 (Gray decode, shift_pi, unwrap_value) ->
// stage 5 (correspond: the merged valid byte; correspond_arg: the continuous projector coordinate) -> undistort_reproject of both
// devices -> triangulate_px -> subpixel_reproj_err2 / subpixel_residual.  Every arithmetic step is the helper the staged kernels call
// (sl3d_device.h, sl3d_subpixel.h), with the arguments they call it with; nothing is tabulated.
//   ANCHOR  k_subpixel_fused<true> (SL3D_FLAG_ANCHOR_PERIODS): the solve takes the anchored coordinates (sl3d_anchor.h) from the
//           shifted wrapped phase and the code where k_subpixel<true> takes them; the absolute phase still decides the valid byte.
//   shape   a lane owns the 4 consecutive pixels of one dword of every u8 plane (the pitch is a multiple of 16: a quad never straddles
//           a row) and walks the views of the launch itself: the camera side (u, v) of a pixel does not depend on the view and is
//           formed once per pixel and launch, for the pixels some view of the launch selects.  The Gray planes are a run-time loop
//           (0..16 per axis): one kernel, not a family.
//   memory  per pixel and view: 2 F + 2 (Nv + Nh) frame bytes and the prepared valid byte (`band`, read twice: once for the camera
//           side) in, 12 B of points, 4 B of residual and the valid byte out -- 16-byte stores per lane, streaming.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_anchor.h"
#include "sl3d_device.h"
#include "sl3d_internal.h"
#include "sl3d_subpixel.h"

namespace sl3d {

#define SL3D_SPF_BLOCK 256  // lanes per block: 1024 pixels

typedef float spf_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned spf_load(const uint8_t *p) { return __builtin_nontemporal_load((const unsigned *)p); }
__device__ __forceinline__ unsigned spf_byte(unsigned w, int k) { return (w >> (8 * k)) & 0xffu; }

// the absolute phase of one axis of the quad's pixels whose bit is set in `bits` (k_wrap + k_unwrap; 0 where stage 4's loop does not run),
// and with ANCHOR beside it what stage 4 leaves in the wrapped-phase and code planes where its loop runs: w = shift_pi(phi), code_out.
// (Without ANCHOR the text is the parent's, statement by statement: that instantiation keeps the parent's instruction stream.)
template <bool ANCHOR>
__device__ __forceinline__ void spf_axis(const KParams &P, const uint8_t *quad, int axis, unsigned bits, int gx0, int gy, const AtanK &K, float unw[4],
                                         float w[4], int code_out[4])
{
    const int N = axis == 0 ? P.Nv : P.Nh;
    const uint8_t *fr = quad + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride;
    const unsigned i0 = spf_load(fr), i1 = spf_load(fr + P.plane_stride), i2 = spf_load(fr + 2 * P.plane_stride);
    const unsigned i3 = P.F == 4 ? spf_load(fr + 3 * P.plane_stride) : 0u;
    const uint8_t *gr = fr + (size_t)P.F * P.plane_stride;
    unsigned b[4] = {0u, 0u, 0u, 0u};
    int code[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (int i = 0; i < N; i++) {
        const unsigned pos = spf_load(gr + (size_t)i * P.plane_stride), inv = spf_load(gr + (size_t)(N + i) * P.plane_stride);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] ^= spf_byte(pos, k) >= spf_byte(inv, k) ? 1u : 0u;  // 4/phase_unwrap.cpp:183, :187-191
            code[k] = code[k] * 2 + (int)b[k];                       // :193
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        unw[k] = 0.f;
        if (ANCHOR) {
            w[k] = 0.f;
            code_out[k] = code[k];
        }
        if (!(bits >> k & 1u)) continue;
        const float phi = wrapped_phase<false>(P.F, spf_byte(i0, k), spf_byte(i1, k), spf_byte(i2, k), spf_byte(i3, k), nullptr, K);
        const bool in_range = axis == 0 ? (gx0 + k >= 1 && gx0 + k <= P.fullW - 2) : (gy >= 1 && gy <= P.fullH - 2);  // :285 / :304
        if (in_range) unw[k] = unwrap_value(shift_pi(phi), code[k]);
        if (ANCHOR && in_range) w[k] = shift_pi(phi);
    }
}

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (as a kernel argument its 93
// doubles were loaded up front: 180 VGPRs with 128 SGPRs spilled into them, 2 waves per SIMD; this way 117 VGPRs, 4 waves)
template <bool ANCHOR>
__global__ __launch_bounds__(SL3D_SPF_BLOCK) void k_subpixel_fused(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views,
                                                                   float *__restrict__ residual)
{
    const CONST_AS DevCal &C = *opaque_const(Cp);
    const size_t px0 = 4 * ((size_t)blockIdx.x * SL3D_SPF_BLOCK + threadIdx.x);  // first pixel of the lane's quad, padding columns included
    if (px0 >= P.px_view_stride) return;                                          // (a multiple of 16: a quad is inside a view or outside it)
    const unsigned lane_off = (unsigned)px0;
    const int row = (int)(px0 / (size_t)P.pitch), col = (int)(px0 - (size_t)row * P.pitch);
    const int gx0 = P.col0 + col, gy = P.row0 + row;
    const bool decodes = P.F != 5;  // check_I_mod_criteria, 3/wrapped_phase.cpp:106-115: with 5 steps nothing is valid (k_wrap)
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
    PinnedRows PR;
    for (int j = 0; j < 4; j++) { PR.c2[j] = C.Ac[8 + j]; PR.p2[j] = C.Ap[8 + j]; }
    const AtanK K = atan_consts<false>();
    const float nanv = __builtin_nanf("");
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const size_t px = (size_t)view * P.px_view_stride + px0;
        const unsigned bits = decodes ? mask_quad_bits(load_mask_quad(P, view, lane_off)) : 0u;
        float out[12], res[4];
#pragma unroll
        for (int j = 0; j < 12; j++) out[j] = nanv;
#pragma unroll
        for (int k = 0; k < 4; k++) res[k] = nanv;
        unsigned valid = 0u;
        if (bits) {
            const uint8_t *quad = P.frames + (size_t)view * P.view_stride + px0;
            float unw0[4], unw1[4], w0[4], w1[4];
            int code0[4], code1[4];
            spf_axis<ANCHOR>(P, quad, 0, bits, gx0, gy, K, unw0, w0, code0);
            spf_axis<ANCHOR>(P, quad, 1, bits, gx0, gy, K, unw1, w1, code1);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(bits >> k & 1u)) continue;  // merge_valid_maps: both axes carry the valid byte of the boundary removal
                long cx, cy;
                double dx, dy;
                const bool okx = correspond(unw0[k], P.fwv, P.PW, cx, dx), oky = correspond(unw1[k], P.fwh, P.PH, cy, dy);
                if (!(okx && oky)) continue;      // k_corr
                // (where the formula does not apply the coordinate stays as it is: k_subpixel<true>)
                const double xs = ANCHOR && anchor_applies(P.Nv, gx0 + k, P.fullW) ? anchor_coordinate(w0[k], code0[k], P.fwv, P.F) : correspond_arg(unw0[k], P.fwv);
                const double ys = ANCHOR && anchor_applies(P.Nh, gy, P.fullH) ? anchor_coordinate(w1[k], code1[k], P.fwh, P.F) : correspond_arg(unw1[k], P.fwh);
                double up, vp, X[3];
                undistort_reproject(xs, ys, C.proj, up, vp);
                triangulate_px(C, PR, u[k], v[k], up, vp, X);
                double Ac[12], Ap[12];  // (subpixel_reproj_err2 takes a plain pointer: the matrices by value, scalar registers after inlining)
                for (int j = 0; j < 12; j++) { Ac[j] = C.Ac[j]; Ap[j] = C.Ap[j]; }
                res[k] = subpixel_residual(subpixel_reproj_err2(Ac, X, u[k], v[k]), subpixel_reproj_err2(Ap, X, up, vp));
                out[3 * k + 0] = (float)X[0];
                out[3 * k + 1] = (float)X[1];
                out[3 * k + 2] = (float)X[2];
                valid |= 1u << (8 * k);
            }
        }
        spf_f32x4 *pts = (spf_f32x4 *)(P.points + 3 * px);
#pragma unroll
        for (int j = 0; j < 3; j++) __builtin_nontemporal_store((spf_f32x4){out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]}, pts + j);
        __builtin_nontemporal_store((spf_f32x4){res[0], res[1], res[2], res[3]}, (spf_f32x4 *)(residual + px));
        *(unsigned *)(P.valid + px) = valid;
    }
}

int launch_subpixel_fused(const KParams &P, const DevCal *C, int first_view, int n_views, float *residual, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const size_t quads = P.px_view_stride / 4;
    const dim3 grid((unsigned)((quads + SL3D_SPF_BLOCK - 1) / SL3D_SPF_BLOCK));
    if (anchor) hipLaunchKernelGGL(k_subpixel_fused<true>, grid, dim3(SL3D_SPF_BLOCK), 0, (hipStream_t)stream, P, C, first_view, n_views, residual);
    else hipLaunchKernelGGL(k_subpixel_fused<false>, grid, dim3(SL3D_SPF_BLOCK), 0, (hipStream_t)stream, P, C, first_view, n_views, residual);
    return (int)hipGetLastError();
}

}  // namespace sl3d
