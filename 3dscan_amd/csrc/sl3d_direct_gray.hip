// sl3d_direct_gray.hip -- gfx950 (MI355X, wave64): the scans of a SL3D_FLAG_DIRECT_GRAY context (sl3d_direct_gray.h): stage 4's Gray
// bit is (2 * gray - (I0 + I2) >= 0), the Gray frame against the mean of the pixel's fringe frames, and no inverse Gray plane is read.
//   k_unwrap_direct   the staged route (SL3D_FLAG_KEEP_STAGES): k_unwrap with that bit, statement by statement otherwise.  It reads fringe
//                     planes 0 and 2 of the axis beside the N Gray planes.
//   k_direct_gray<AXES, ANCHOR>   the timed route, ONE launch: AXES = 0 / 1 what k_one_axis<AXES, ANCHOR> leaves (SL3D_FLAG_ONLY_VERTICAL /
//                     _HORIZONTAL: the exactly determined ray-plane solve, no residual), AXES = 2 what k_subpixel_fused<ANCHOR> leaves (both
//                     axes, the least-squares solve and its residual plane) -- bit for bit what k_wrap, k_unwrap_direct, k_corr / k_corr_one
//                     and k_subpixel / k_subpixel_one leave on a SL3D_FLAG_KEEP_STAGES context.  Every arithmetic step is the helper the
//                     staged kernels call, with the arguments they call it with.
//   shape   k_subpixel_fused's and k_one_axis's: a lane owns the 4 consecutive pixels of one dword of every u8 plane (the pitch is a
//           multiple of 16: a quad never straddles a row) and walks the views of the launch itself; the camera side (u, v) of a pixel is
//           formed once per pixel and launch, for the pixels some view of the launch selects.  The Gray planes are a run-time loop (0..16).
//   memory  per pixel, view and coded axis: F + N frame bytes -- I0 and I2 are in registers for the phase, the threshold costs no load --
//           and the prepared valid byte (`band`, read twice: once for the camera side) in; 12 B of points, with two axes 4 B of residual,
//           and the valid byte out -- 16-byte stores per lane, streaming.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_anchor.h"
#include "sl3d_device.h"
#include "sl3d_direct_gray.h"
#include "sl3d_internal.h"
#include "sl3d_one_axis.h"
#include "sl3d_subpixel.h"

static_assert(SL3D_MAX_GRAY <= 16, "direct_gray_step2 keeps a code in a 16-bit field");

namespace sl3d {

#define SL3D_DG_BLOCK 256  // lanes per block: 1024 pixels

typedef float dg_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned dg_load(const uint8_t *p) { return __builtin_nontemporal_load((const unsigned *)p); }
__device__ __forceinline__ int dg_byte(unsigned w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

// stage 4 of a SL3D_FLAG_DIRECT_GRAY context: unwrap_phase  4/phase_unwrap.cpp:367-393 (Gray-code mode, count == 1) with the direct bit
// (k_unwrap's text with another bit: a shared body changed k_unwrap's instruction stream -- 341 -> 366 instructions -- and was dropped, so a
// change to stage 4 goes into both; tests/test_gpu_direct_gray.py holds the stage planes of the two to each other where the codes agree)
__global__ __launch_bounds__(256) void k_unwrap_direct(const KParams P, int view, int axis)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(t / P.pitch), col = (int)(t - (long)row * P.pitch);
    if (row >= P.H) return;
    const size_t px = (size_t)view * P.px_view_stride + (size_t)row * P.pitch + col;
    const int gx = P.col0 + col, gy = P.row0 + row;
    const bool v = P.valid_axis[axis][px] == 1;
    int code = -1;  // :143 / :211
    float unw = 0.f;
    uint8_t dbg = 0;
    if (v) {
        const int N = axis == 0 ? P.Nv : P.Nh;
        const uint8_t *fr = P.frames + (size_t)view * P.view_stride + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride + (size_t)row * P.pitch + col;
        const int i0 = fr[0], i2 = fr[2 * P.plane_stride];
        const uint8_t *gr = fr + (size_t)P.F * P.plane_stride;
        int b = 0;
        code = 0;
        for (int i = 0; i < N; i++) {
            b ^= direct_gray_bit(gr[(size_t)i * P.plane_stride], i0, i2);  // (sl3d_direct_gray.h) :187-191
            code = code * 2 + b;                                           // :193
        }
        const bool in_range = axis == 0 ? (gx >= 1 && gx <= P.fullW - 2) : (gy >= 1 && gy <= P.fullH - 2);  // :285 / :304
        if (in_range) {
            float w = P.wrapped[axis][px];
            w = (float)((double)w + PI_REF);  // wrapped += Pi   :290 / :308
            P.wrapped[axis][px] = w;
            unw = unwrap_value(w, code);  // :291 / :309
        }
        // save_unwrap_phase_image :334-335 / :353-354: t is float, t*255 is float, cast to uchar (x86 wraps)
        const int ncodes = axis == 0 ? P.ncodes_v : P.ncodes_h;
        const float tt = (float)(unw / (2.0 * PI_REF * ncodes));
        dbg = (uint8_t)(int)(tt * 255);
    }
    P.code[axis][px] = code;
    P.unwrapped[axis][px] = unw;
    P.dbg4[axis][px] = dbg;
}

// the frames of one axis of a quad: the fringe dwords (for the phase AND the threshold) and stage 4's code of the four pixels.  F + N loads.
struct DgAxis {
    unsigned i0, i1, i2, i3;
    int code[4];
};
template <int AXIS>
__device__ __forceinline__ void dg_decode(const KParams &P, const uint8_t *quad, DgAxis &A)
{
    const int N = AXIS == 0 ? P.Nv : P.Nh;
    const uint8_t *fr = quad + (size_t)(AXIS == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride;
    A.i0 = dg_load(fr), A.i1 = dg_load(fr + P.plane_stride), A.i2 = dg_load(fr + 2 * P.plane_stride);
    A.i3 = P.F == 4 ? dg_load(fr + 3 * P.plane_stride) : 0u;
    const uint8_t *gr = fr + (size_t)P.F * P.plane_stride;
    // (two pixels per word in 16-bit fields, sl3d_direct_gray.h: 6 registers through the loop instead of 12, which keeps the one-axis forms at
    // 4 waves per SIMD; SL3D_MAX_GRAY planes fill a field exactly)
    const unsigned s_even = direct_gray_sum2(A.i0, A.i2, 0), s_odd = direct_gray_sum2(A.i0, A.i2, 1);
    unsigned b_even = 0u, b_odd = 0u, c_even = 0u, c_odd = 0u;
#pragma unroll 2
    for (int i = 0; i < N; i++) {
        const unsigned pos = dg_load(gr + (size_t)i * P.plane_stride);
        direct_gray_step2(pos, s_even, 0, b_even, c_even);  // 4/phase_unwrap.cpp:183 by the direct rule, :187-191, :193
        direct_gray_step2(pos, s_odd, 1, b_odd, c_odd);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) A.code[k] = direct_gray_field(c_even, c_odd, k);
}

// pixel k of the quad as stages 3 and 4 leave it: w = shift_pi(phi) and the absolute phase where stage 4's loop runs, 0 elsewhere
template <int AXIS>
__device__ __forceinline__ void dg_phase(const KParams &P, const DgAxis &A, int k, int gx0, int gy, const AtanK &K, float &w, float &unw)
{
    const float phi = wrapped_phase<false>(P.F, dg_byte(A.i0, k), dg_byte(A.i1, k), dg_byte(A.i2, k), dg_byte(A.i3, k), nullptr, K);
    const bool in_range = AXIS == 0 ? (gx0 + k >= 1 && gx0 + k <= P.fullW - 2) : (gy >= 1 && gy <= P.fullH - 2);  // :285 / :304
    w = in_range ? shift_pi(phi) : 0.f;
    unw = in_range ? unwrap_value(w, A.code[k]) : 0.f;
}

// the continuous coordinate of one axis of a pixel: correspond_arg, or with ANCHOR the anchored one where that rule applies (k_subpixel<ANCHOR>)
template <int AXIS, bool ANCHOR>
__device__ __forceinline__ double dg_coordinate(const KParams &P, float unw, float w, int code, int gx, int gy)
{
    const int N = AXIS == 0 ? P.Nv : P.Nh, fw = AXIS == 0 ? P.fwv : P.fwh;
    const int pos = AXIS == 0 ? gx : gy, full = AXIS == 0 ? P.fullW : P.fullH;
    return ANCHOR && anchor_applies(N, pos, full) ? anchor_coordinate(w, code, fw, P.F) : correspond_arg(unw, fw);
}

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (k_subpixel_fused)
template <int AXES, bool ANCHOR>
__global__ __launch_bounds__(SL3D_DG_BLOCK) void k_direct_gray(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views,
                                                               float *__restrict__ residual)
{
    const CONST_AS DevCal &C = *opaque_const(Cp);
    const size_t px0 = 4 * ((size_t)blockIdx.x * SL3D_DG_BLOCK + threadIdx.x);  // first pixel of the lane's quad, padding columns included
    if (px0 >= P.px_view_stride) return;                                         // (a multiple of 16: a quad is inside a view or outside it)
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
    if (AXES == 2)
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
            if (AXES == 2) {
                DgAxis A0, A1;
                dg_decode<0>(P, quad, A0);
                dg_decode<1>(P, quad, A1);
                float unw0[4], unw1[4], w0[4], w1[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    unw0[k] = unw1[k] = w0[k] = w1[k] = 0.f;
                    if (!(bits >> k & 1u)) continue;
                    dg_phase<0>(P, A0, k, gx0, gy, K, w0[k], unw0[k]);
                    dg_phase<1>(P, A1, k, gx0, gy, K, w1[k], unw1[k]);
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!(bits >> k & 1u)) continue;  // merge_valid_maps: both axes carry the valid byte of the boundary removal
                    long cx, cy;
                    double dx, dy;
                    const bool okx = correspond(unw0[k], P.fwv, P.PW, cx, dx), oky = correspond(unw1[k], P.fwh, P.PH, cy, dy);
                    if (!(okx && oky)) continue;      // k_corr
                    const double xs = dg_coordinate<0, ANCHOR>(P, unw0[k], w0[k], A0.code[k], gx0 + k, gy);
                    const double ys = dg_coordinate<1, ANCHOR>(P, unw1[k], w1[k], A1.code[k], gx0 + k, gy);
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
            } else {
                constexpr int AXIS = AXES == 1 ? 1 : 0;
                DgAxis A;
                dg_decode<AXIS>(P, quad, A);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!(bits >> k & 1u)) continue;  // the valid byte of stage 3's boundary removal
                    float w, unw;
                    dg_phase<AXIS>(P, A, k, gx0, gy, K, w, unw);
                    long c;
                    double d;
                    if (!correspond(unw, AXIS == 0 ? P.fwv : P.fwh, AXIS == 0 ? P.PW : P.PH, c, d)) continue;  // k_corr_one
                    const double s = dg_coordinate<AXIS, ANCHOR>(P, unw, w, A.code[k], gx0 + k, gy);
                    const double t = one_axis_project(s, C.proj.K[AXIS == 0 ? 0 : 4], AXIS == 0 ? C.proj.ifx : C.proj.ify, AXIS == 0 ? C.proj.cx : C.proj.cy);
                    double X[3];
                    one_axis_solve(C.Ac, C.Ap, AXIS, u[k], v[k], t, X);
                    out[3 * k + 0] = (float)X[0];
                    out[3 * k + 1] = (float)X[1];
                    out[3 * k + 2] = (float)X[2];
                    valid |= 1u << (8 * k);
                }
            }
        }
        dg_f32x4 *pts = (dg_f32x4 *)(P.points + 3 * px);
#pragma unroll
        for (int j = 0; j < 3; j++) __builtin_nontemporal_store((dg_f32x4){out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]}, pts + j);
        if (AXES == 2) __builtin_nontemporal_store((dg_f32x4){res[0], res[1], res[2], res[3]}, (dg_f32x4 *)(residual + px));
        *(unsigned *)(P.valid + px) = valid;
    }
}

int launch_unwrap_direct(const KParams &P, int view, int axis, void *stream)
{
    (void)hipGetLastError();
    const dim3 grid((unsigned)(((size_t)P.H * P.pitch + 255) / 256));
    hipLaunchKernelGGL(k_unwrap_direct, grid, dim3(256), 0, (hipStream_t)stream, P, view, axis);
    return (int)hipGetLastError();
}

// axes: 0 / 1: the one coded axis, 2: both (residual: the context's residual plane; not read otherwise)
int launch_direct_gray(const KParams &P, const DevCal *C, int axes, int first_view, int n_views, float *residual, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const size_t quads = P.px_view_stride / 4;
    const dim3 grid((unsigned)((quads + SL3D_DG_BLOCK - 1) / SL3D_DG_BLOCK));
#define SL3D_DG(AXES, ANCHOR) \
    hipLaunchKernelGGL((k_direct_gray<AXES, ANCHOR>), grid, dim3(SL3D_DG_BLOCK), 0, (hipStream_t)stream, P, C, first_view, n_views, residual)
    if (axes == 0) { if (anchor) SL3D_DG(0, true); else SL3D_DG(0, false); }
    else if (axes == 1) { if (anchor) SL3D_DG(1, true); else SL3D_DG(1, false); }
    else { if (anchor) SL3D_DG(2, true); else SL3D_DG(2, false); }
#undef SL3D_DG
    return (int)hipGetLastError();
}

}  // namespace sl3d
