// sl3d_quad.h -- what a quad-per-lane kernel is made of: the one-launch kernels of the timed contexts -- k_subpixel_fused
// (sl3d_subpixel_fused.hip), k_repair_fused (sl3d_repair_fused.hip), k_one_axis (sl3d_one_axis.hip) and k_direct_gray (sl3d_direct_gray.hip) --
// take from here every piece they have in common that could be shared without moving their vector instruction streams; where none of the forms
// tried could, a kernel keeps statements of its own and says so (the list: profiles/quad_kernels_isa.txt).  Every arithmetic step is the helper
// the staged kernels call (sl3d_device.h, sl3d_anchor.h, sl3d_one_axis.h, sl3d_subpixel.h), with their arguments; nothing is tabulated.
//   shape   a lane owns the 4 consecutive pixels of one dword of every u8 plane (the pitch is a multiple of 16: a quad never straddles a
//           row) and walks the views of the launch itself.  The camera side (u, v) of a pixel does not depend on the view and is formed
//           once per pixel and launch, for the pixels some view of the launch selects (quad_need).  That loop -- four unrolled
//           undistort_reproject(C.cam) -- is written in each kernel: as a helper filling u[4] / v[4] it comes out rolled
//           (profiles/quad_kernels_isa.txt).  The Gray planes are a run-time loop (0..16 per axis): one kernel, not a family.
//   memory  per pixel and view the prepared valid byte (`band`, read twice: once for the camera side) and the frame bytes of the coded
//           axes in, 12 B of points, the valid byte and (two axes) 4 B of residual out -- 16-byte stores per lane, streaming.
// Which forms of these helpers leave the kernels' instruction streams alone, and which were left out: profiles/quad_kernels_isa.txt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_anchor.h"
#include "sl3d_device.h"
#include "sl3d_internal.h"
#include "sl3d_one_axis.h"
#include "sl3d_subpixel.h"

namespace sl3d {

#define SL3D_QUAD_BLOCK 256  // lanes per block: 1024 pixels of a flat kernel

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned quad_load(const uint8_t *p) { return __builtin_nontemporal_load((const unsigned *)p); }
__device__ __forceinline__ unsigned quad_byte(unsigned w, int k) { return (w >> (8 * k)) & 0xffu; }

// the quad of a lane of a flat kernel (k_repair_fused has tiles).  quad_px0() at or beyond P.px_view_stride: the lane has none -- the
// kernel returns (that test inside a helper changes the compare's encoding and two waits in every flat kernel)
struct QuadFrame {
    size_t px0;    // first pixel of the lane's quad within a view, padding columns included
    int gx0, gy;   // ... and in the frame
    bool decodes;  // check_I_mod_criteria, 3/wrapped_phase.cpp:106-115: with 5 steps nothing is valid (k_wrap)
};
__device__ __forceinline__ size_t quad_px0() { return 4 * ((size_t)blockIdx.x * SL3D_QUAD_BLOCK + threadIdx.x); }
__device__ __forceinline__ QuadFrame quad_frame(const KParams &P, size_t px0)  // (px_view_stride is a multiple of 16: a quad is inside a view or outside it)
{
    const int row = (int)(px0 / (size_t)P.pitch), col = (int)(px0 - (size_t)row * P.pitch);
    return {px0, P.col0 + col, P.row0 + row, P.F != 5};
}

// the pixels of the quad some view of the launch selects: the ones that need the camera side
__device__ __forceinline__ unsigned quad_need(const KParams &P, bool decodes, int first_view, int n_views, unsigned lane_off)
{
    unsigned need = 0u;
    if (decodes)
        for (int vi = 0; vi < n_views; vi++) need |= mask_quad_bits(load_mask_quad(P, first_view + vi, lane_off));
    return need;
}

// the frames of one axis of a quad: the fringe dwords and stage 4's code of the four pixels
struct QuadAxis {
    unsigned i0, i1, i2, i3;
    int code[4];
};

// the fringe dwords of `axis` (F loads); returns the first of its Gray planes
__device__ __forceinline__ const uint8_t *quad_fringes(const KParams &P, const uint8_t *quad, int axis, QuadAxis &A)
{
    const uint8_t *fr = quad + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride;
    A.i0 = quad_load(fr), A.i1 = quad_load(fr + P.plane_stride), A.i2 = quad_load(fr + 2 * P.plane_stride);
    A.i3 = P.F == 4 ? quad_load(fr + 3 * P.plane_stride) : 0u;
    return fr + (size_t)P.F * P.plane_stride;
}

// ... and stage 4's codes from the N Gray planes against their N inverses (the direct rule: dg_decode, sl3d_direct_gray.hip)
__device__ __forceinline__ void quad_decode(const KParams &P, const uint8_t *quad, int axis, QuadAxis &A)
{
    const int N = axis == 0 ? P.Nv : P.Nh;
    const uint8_t *gr = quad_fringes(P, quad, axis, A);
    unsigned b[4] = {0u, 0u, 0u, 0u};
    int code[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (int i = 0; i < N; i++) {
        const unsigned pos = quad_load(gr + (size_t)i * P.plane_stride), inv = quad_load(gr + (size_t)(N + i) * P.plane_stride);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] ^= quad_byte(pos, k) >= quad_byte(inv, k) ? 1u : 0u;  // 4/phase_unwrap.cpp:183, :187-191
            code[k] = code[k] * 2 + (int)b[k];                         // :193
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) A.code[k] = code[k];
}

// pixel k of a decoded axis as stages 3 and 4 leave it (k_wrap + k_unwrap): w = shift_pi(phi) and the absolute phase where stage 4's loop
// runs; elsewhere w and unw stay what the caller made them, 0
__device__ __forceinline__ void quad_phase(const KParams &P, const QuadAxis &A, int axis, int k, int gx0, int gy, const AtanK &K, float &w, float &unw)
{
    const float phi = wrapped_phase<false>(P.F, quad_byte(A.i0, k), quad_byte(A.i1, k), quad_byte(A.i2, k), quad_byte(A.i3, k), nullptr, K);
    const int pos = axis == 0 ? gx0 + k : gy, full = axis == 0 ? P.fullW : P.fullH;
    const bool in_range = pos >= 1 && pos <= full - 2;  // :285 / :304
    if (in_range) {
        w = shift_pi(phi);
        unw = unwrap_value(w, A.code[k]);
    }
}

// stages 3 and 4 of one axis of a quad: quad_decode, and quad_phase of the pixels whose bit is set in `bits` (zeros for the others)
__device__ __forceinline__ void quad_axis(const KParams &P, const uint8_t *quad, int axis, unsigned bits, int gx0, int gy, const AtanK &K, QuadAxis &A,
                                          float w[4], float unw[4])
{
    quad_decode(P, quad, axis, A);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        w[k] = unw[k] = 0.f;
        if (bits >> k & 1u) quad_phase(P, A, axis, k, gx0, gy, K, w[k], unw[k]);
    }
}

// the continuous coordinate of one axis of a pixel at (gx, gy): correspond_arg, or with ANCHOR the anchored one (sl3d_anchor.h) where that
// rule applies -- where it does not the coordinate stays as it is (k_subpixel<ANCHOR>, k_subpixel_one<AXIS, ANCHOR>)
template <bool ANCHOR>
__device__ __forceinline__ double quad_coordinate(const KParams &P, int axis, float unw, float w, int code, int gx, int gy)
{
    const int N = axis == 0 ? P.Nv : P.Nh, fw = axis == 0 ? P.fwv : P.fwh;
    const int pos = axis == 0 ? gx : gy, full = axis == 0 ? P.fullW : P.fullH;
    return ANCHOR && anchor_applies(N, pos, full) ? anchor_coordinate(w, code, fw, P.F) : correspond_arg(unw, fw);
}

// stage 5 of a pixel: both axes (k_corr; merge_valid_maps: both carry the valid byte of the boundary removal; cx, cy: the c_p_map's
// integers), or the coded one alone (k_corr_one)
__device__ __forceinline__ bool quad_correspond(const KParams &P, float unw0, float unw1, long &cx, long &cy)
{
    double dx, dy;
    const bool okx = correspond(unw0, P.fwv, P.PW, cx, dx), oky = correspond(unw1, P.fwh, P.PH, cy, dy);
    return okx && oky;
}
__device__ __forceinline__ bool quad_correspond_one(const KParams &P, int axis, float unw)
{
    long c;
    double d;
    return correspond(unw, axis == 0 ? P.fwv : P.fwh, axis == 0 ? P.PW : P.PH, c, d);
}

// the two-axis solve of pixel k from the projector coordinate (xs, ys) -- the continuous one (k_subpixel) or the c_p_map's integers (k_tri) --
// and the camera side (u, v): the point, the valid byte and with RES the reprojection residual (quad_residual: a function of its own, inside
// quad_solve's body the two-axis kernels spill 16 more registers -- profiles/quad_kernels_isa.txt)
template <typename CalT>
__device__ __forceinline__ float quad_residual(const CalT &C, const double X[3], double u, double v, double up, double vp)
{
    double Ac[12], Ap[12];  // (subpixel_reproj_err2 takes a plain pointer: the matrices by value, scalar registers after inlining)
    for (int j = 0; j < 12; j++) { Ac[j] = C.Ac[j]; Ap[j] = C.Ap[j]; }
    return subpixel_residual(subpixel_reproj_err2(Ac, X, u, v), subpixel_reproj_err2(Ap, X, up, vp));
}
template <bool RES, typename CalT>
__device__ __forceinline__ void quad_solve(const CalT &C, const PinnedRows &PR, double xs, double ys, double u, double v, int k, float out[12],
                                           float res[4], unsigned &valid)
{
    double up, vp, X[3];
    undistort_reproject(xs, ys, C.proj, up, vp);
    triangulate_px(C, PR, u, v, up, vp, X);
    if (RES) res[k] = quad_residual(C, X, u, v, up, vp);
    out[3 * k + 0] = (float)X[0];
    out[3 * k + 1] = (float)X[1];
    out[3 * k + 2] = (float)X[2];
    valid |= 1u << (8 * k);
}

// the one-axis solve of pixel k from the continuous coordinate s of axis AXIS (k_subpixel_one): the exactly determined ray-plane
// intersection (sl3d_one_axis.h), no residual
template <int AXIS, typename CalT>
__device__ __forceinline__ void quad_solve_one(const CalT &C, double s, double u, double v, int k, float out[12], unsigned &valid)
{
    const double t = one_axis_project(s, C.proj.K[AXIS == 0 ? 0 : 4], AXIS == 0 ? C.proj.ifx : C.proj.ify, AXIS == 0 ? C.proj.cx : C.proj.cy);
    double X[3];
    one_axis_solve(C.Ac, C.Ap, AXIS, u, v, t, X);
    out[3 * k + 0] = (float)X[0];
    out[3 * k + 1] = (float)X[1];
    out[3 * k + 2] = (float)X[2];
    valid |= 1u << (8 * k);
}

// a view of a quad begins with nothing valid ...
template <bool RES>
__device__ __forceinline__ void quad_clear(float out[12], float res[4], unsigned &valid)
{
    const float nanv = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = nanv;
    if (RES) {
#pragma unroll
        for (int k = 0; k < 4; k++) res[k] = nanv;
    }
    valid = 0u;
}

// ... and ends with its stores: px = the quad's first pixel among all views'
template <bool RES>
__device__ __forceinline__ void quad_store(const KParams &P, size_t px, const float out[12], const float res[4], unsigned valid, float *residual)
{
    f32x4 *pts = (f32x4 *)(P.points + 3 * px);
#pragma unroll
    for (int j = 0; j < 3; j++) __builtin_nontemporal_store((f32x4){out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]}, pts + j);
    if (RES) __builtin_nontemporal_store((f32x4){res[0], res[1], res[2], res[3]}, (f32x4 *)(residual + px));
    *(unsigned *)(P.valid + px) = valid;
}

// host: the grid of a flat kernel, and a launch between two reads of the error state (returns the launch's hipError_t)
inline dim3 quad_grid(const KParams &P) { return dim3((unsigned)((P.px_view_stride / 4 + SL3D_QUAD_BLOCK - 1) / SL3D_QUAD_BLOCK)); }
template <typename... Params, typename... Args>
inline int quad_launch(void (*kernel)(Params...), dim3 grid, void *stream, Args... args)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, grid, dim3(SL3D_QUAD_BLOCK), 0, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}

}  // namespace sl3d
