// sl3d_direct_gray.hip -- gfx950 (MI355X, wave64): the scans of a SL3D_FLAG_DIRECT_GRAY context (sl3d_direct_gray.h): stage 4's Gray
// bit is (2 * gray - (I0 + I2) >= 0), the Gray frame against the mean of the pixel's fringe frames, and no inverse Gray plane is read.
//   k_unwrap_direct   the staged route (SL3D_FLAG_KEEP_STAGES): k_unwrap with that bit, statement by statement otherwise.  It reads fringe
//                     planes 0 and 2 of the axis beside the N Gray planes.
//   k_direct_gray<AXES, ANCHOR>   the timed route, ONE launch: AXES = 0 / 1 what k_one_axis<AXES, ANCHOR> leaves (SL3D_FLAG_ONLY_VERTICAL /
//                     _HORIZONTAL: the exactly determined ray-plane solve, no residual), AXES = 2 what k_subpixel_fused<ANCHOR> leaves (both
//                     axes, the least-squares solve and its residual plane) -- bit for bit what k_wrap, k_unwrap_direct, k_corr / k_corr_one
//                     and k_subpixel / k_subpixel_one leave on a SL3D_FLAG_KEEP_STAGES context.  Every arithmetic step is the helper the
//                     staged kernels call, with the arguments they call it with.
//   shape   the quad-per-lane kernel of sl3d_quad.h, its pieces from there but the decode (dg_decode: the packed direct rule), the camera-side
//           loop and, with two axes, the phase step (dg_phase: quad_phase with selects).  With two axes k_subpixel_fused's order (both axes
//           decoded and their phases formed, then the solves), with one k_one_axis's.
//   memory  sl3d_quad.h's; per pixel, view and coded axis F + N frame bytes in -- I0 and I2 are in registers for the phase, the threshold
//           costs no load --, with two axes the residual out.
// Compiled with -ffp-contract=off.
#include "sl3d_direct_gray.h"
#include "sl3d_quad.h"

static_assert(SL3D_MAX_GRAY <= 16, "direct_gray_step2 keeps a code in a 16-bit field");

namespace sl3d {

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

// stage 4's code of the four pixels of one axis of a quad by the direct rule (quad_decode's place): the fringe dwords serve the phase AND the
// threshold.  F + N loads.
template <int AXIS>
__device__ __forceinline__ void dg_decode(const KParams &P, const uint8_t *quad, QuadAxis &A)
{
    const int N = AXIS == 0 ? P.Nv : P.Nh;
    const uint8_t *gr = quad_fringes(P, quad, AXIS, A);
    // (two pixels per word in 16-bit fields, sl3d_direct_gray.h: 6 registers through the loop instead of 12, which keeps the one-axis forms at
    // 4 waves per SIMD; SL3D_MAX_GRAY planes fill a field exactly)
    const unsigned s_even = direct_gray_sum2(A.i0, A.i2, 0), s_odd = direct_gray_sum2(A.i0, A.i2, 1);
    unsigned b_even = 0u, b_odd = 0u, c_even = 0u, c_odd = 0u;
#pragma unroll 2
    for (int i = 0; i < N; i++) {
        const unsigned pos = quad_load(gr + (size_t)i * P.plane_stride);
        direct_gray_step2(pos, s_even, 0, b_even, c_even);  // 4/phase_unwrap.cpp:183 by the direct rule, :187-191, :193
        direct_gray_step2(pos, s_odd, 1, b_odd, c_odd);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) A.code[k] = direct_gray_field(c_even, c_odd, k);
}

// quad_phase's statements with selects for its branch, for k_direct_gray<2> (with quad_phase itself those two instantiations lose 12 / 24
// v_mov_b32: profiles/quad_kernels_isa.txt)
__device__ __forceinline__ void dg_phase(const KParams &P, const QuadAxis &A, int axis, int k, int gx0, int gy, const AtanK &K, float &w, float &unw)
{
    const float phi = wrapped_phase<false>(P.F, quad_byte(A.i0, k), quad_byte(A.i1, k), quad_byte(A.i2, k), quad_byte(A.i3, k), nullptr, K);
    const int pos = axis == 0 ? gx0 + k : gy, full = axis == 0 ? P.fullW : P.fullH;
    const bool in_range = pos >= 1 && pos <= full - 2;  // :285 / :304
    w = in_range ? shift_pi(phi) : 0.f;
    unw = in_range ? unwrap_value(w, A.code[k]) : 0.f;
}

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (k_subpixel_fused)
template <int AXES, bool ANCHOR>
__global__ __launch_bounds__(SL3D_QUAD_BLOCK) void k_direct_gray(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views,
                                                                 float *__restrict__ residual)
{
    const CONST_AS DevCal &C = *opaque_const(Cp);
    if (quad_px0() >= P.px_view_stride) return;
    const QuadFrame q = quad_frame(P, quad_px0());
    const unsigned lane_off = (unsigned)q.px0;
    const unsigned need = quad_need(P, q.decodes, first_view, n_views, lane_off);
    double u[4], v[4];  // the camera side (written here: sl3d_quad.h, shape)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u[k] = v[k] = 0.0;
        if (need >> k & 1u) undistort_reproject((double)(q.gx0 + k), (double)q.gy, C.cam, u[k], v[k]);
    }
    PinnedRows PR;
    if (AXES == 2)
        for (int j = 0; j < 4; j++) { PR.c2[j] = C.Ac[8 + j]; PR.p2[j] = C.Ap[8 + j]; }
    const AtanK K = atan_consts<false>();
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const size_t px = (size_t)view * P.px_view_stride + q.px0;
        const unsigned bits = q.decodes ? mask_quad_bits(load_mask_quad(P, view, lane_off)) : 0u;
        float out[12], res[4];
        unsigned valid;
        quad_clear<AXES == 2>(out, res, valid);
        if (bits) {
            const uint8_t *quad = P.frames + (size_t)view * P.view_stride + q.px0;
            if (AXES == 2) {
                QuadAxis A0, A1;
                dg_decode<0>(P, quad, A0);
                dg_decode<1>(P, quad, A1);
                float unw0[4], unw1[4], w0[4], w1[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    unw0[k] = unw1[k] = w0[k] = w1[k] = 0.f;
                    if (!(bits >> k & 1u)) continue;
                    dg_phase(P, A0, 0, k, q.gx0, q.gy, K, w0[k], unw0[k]);
                    dg_phase(P, A1, 1, k, q.gx0, q.gy, K, w1[k], unw1[k]);
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!(bits >> k & 1u)) continue;
                    long cx, cy;
                    if (!quad_correspond(P, unw0[k], unw1[k], cx, cy)) continue;
                    const double xs = quad_coordinate<ANCHOR>(P, 0, unw0[k], w0[k], A0.code[k], q.gx0 + k, q.gy);
                    const double ys = quad_coordinate<ANCHOR>(P, 1, unw1[k], w1[k], A1.code[k], q.gx0 + k, q.gy);
                    quad_solve<true>(C, PR, xs, ys, u[k], v[k], k, out, res, valid);
                }
            } else {
                constexpr int AXIS = AXES == 1 ? 1 : 0;
                QuadAxis A;
                dg_decode<AXIS>(P, quad, A);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!(bits >> k & 1u)) continue;  // the valid byte of stage 3's boundary removal
                    float w = 0.f, unw = 0.f;
                    quad_phase(P, A, AXIS, k, q.gx0, q.gy, K, w, unw);
                    if (!quad_correspond_one(P, AXIS, unw)) continue;
                    quad_solve_one<AXIS>(C, quad_coordinate<ANCHOR>(P, AXIS, unw, w, A.code[k], q.gx0 + k, q.gy), u[k], v[k], k, out, valid);
                }
            }
        }
        quad_store<AXES == 2>(P, px, out, res, valid, residual);
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
    static void (*const kernel[3][2])(KParams, const DevCal *, int, int, float *) = {{k_direct_gray<0, false>, k_direct_gray<0, true>},
                                                                                     {k_direct_gray<1, false>, k_direct_gray<1, true>},
                                                                                     {k_direct_gray<2, false>, k_direct_gray<2, true>}};
    return quad_launch(kernel[axes == 0 ? 0 : axes == 1 ? 1 : 2][anchor], quad_grid(P), stream, P, C, first_view, n_views, residual);
}

}  // namespace sl3d
