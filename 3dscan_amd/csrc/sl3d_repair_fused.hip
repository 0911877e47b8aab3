// sl3d_repair_fused.hip -- gfx950 (MI355X, wave64): the period-repaired scan of a timed context in ONE launch (SL3D_FLAG_REPAIR_PERIODS
// without SL3D_FLAG_KEEP_STAGES).  k_repair_fused<SUB> leaves in the points and valid planes (SUB: and the residual plane) of
// the launch's views, bit for bit, what k_wrap, k_unwrap (both axes), one pass of k_period_jumps<AXIS, 4> + k_period_apply over every
// axis that has Gray planes, k_corr and k_tri (SUB: k_subpixel(+inf)) leave there on a SL3D_FLAG_KEEP_STAGES context -- without any of
// the stage planes between them.  Every arithmetic step is the helper the staged kernels call (sl3d_device.h, sl3d_period.h,
// sl3d_subpixel.h), with the arguments they call it with; the per-pixel chain and the quad-per-lane shape are sl3d_quad.h's.  From that header:
// the types and loads, quad_need, quad_correspond, quad_store, the launch.  As this unit's own statements, because the header's helper in their
// place moves vector instructions of an instantiation (profiles/quad_kernels_isa.txt: which, and by what): the decode and phase step of an axis
// (rpf_axis), a view's NaN fill, and the solve with its residual -- a change to those goes into sl3d_quad.h AND here.
//   tile    256 lanes own 64 columns x 16 rows (the origin a multiple of 4: the radius of 4 is exactly one quad of columns each side), a
//           lane the 4 consecutive pixels of one dword of every u8 plane.  The repair is a Jacobi pass over stage 4's output: a pixel
//           needs the absolute phase and the sample-ness of up to 4 neighbours each side, along its row for the vertical axis and down
//           its column for the horizontal one.  No stage plane holds them, so the block decodes a plus-shaped halo itself: the vertical
//           axis over 72 x 16 pixels (32 halo quads), the horizontal one over 64 x 24 (128 halo quads) -- 1.31 x the decodes and frame
//           bytes of k_subpixel_fused -- and stages the phases in LDS (10.5 KB), a non-sample as +infinity (period_staged).  Then a lane
//           reads the 12 consecutive words of its row run and the 9 words down each of its 4 columns, computes j and k' and recomputes
//           the phase of its OWN pixels only (the code of a halo pixel is not needed), and goes on to stage 5 and stage 7.
//   views   walked inside the block, two barriers per view (staged -> read, read -> the next view's staging); the camera side (u, v) of
//           a pixel is formed once per launch.
//   bounds  a halo quad outside the window is never addressed: it is staged as +infinity, which is how period_request clips a
//           neighbourhood to the window.  A lane whose quad lies beyond the pitch or the last row stages +infinity and stores nothing.
// No atomics (the flag returns no counts), no scratch.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_period.h"
#include "sl3d_quad.h"

namespace sl3d {

#define SL3D_RPF_BLOCK SL3D_QUAD_BLOCK  // lanes per block
#define SL3D_RPF_RADIUS SL3D_REPAIR_FUSED_RADIUS  // the radius of the flag's repair: Scanner.repair_periods' default
constexpr int RPF_COLS = 64, RPF_ROWS = 16;              // the pixels a block owns
constexpr int RPF_QUADS = RPF_COLS / 4;                  // lanes per tile row
constexpr int RPF_RUN = RPF_COLS + 2 * SL3D_RPF_RADIUS;  // a staged row of the vertical axis
constexpr int RPF_BAND = RPF_ROWS + 2 * SL3D_RPF_RADIUS; // the staged rows of the horizontal axis
constexpr int RPF_HALO_V = 2 * RPF_ROWS;                 // halo quads of the vertical axis: one each side of every row
constexpr int RPF_HALO_H = 2 * SL3D_RPF_RADIUS * RPF_QUADS;  // ... of the horizontal axis: 4 rows above and below, 16 quads each
static_assert(SL3D_RPF_RADIUS == 4, "the halo of a row is one quad each side");
static_assert(RPF_QUADS * RPF_ROWS == SL3D_RPF_BLOCK && RPF_HALO_H + RPF_HALO_V <= SL3D_RPF_BLOCK, "a lane owns one quad and decodes at most one halo quad");
static_assert(RPF_HALO_H % 64 == 0, "the two halo axes do not share a wave");

// (quad_axis's statements) one axis of a quad as stages 3 and 4 leave it (k_wrap + k_unwrap), for the pixels whose bit is set in `bits`: the wrapped phase after
// stage 4's += Pi, the Gray code and the absolute phase (0 where stage 4's loop does not run)
struct RpfAxis {
    float w[4], unw[4];
    int code[4];
};
__device__ __forceinline__ void rpf_axis(const KParams &P, const uint8_t *quad, int axis, unsigned bits, int gx0, int gy, const AtanK &K, RpfAxis &a)
{
    const int N = axis == 0 ? P.Nv : P.Nh;
    const uint8_t *fr = quad + (size_t)(axis == 0 ? 0 : P.F + 2 * P.Nv) * P.plane_stride;
    const unsigned i0 = quad_load(fr), i1 = quad_load(fr + P.plane_stride), i2 = quad_load(fr + 2 * P.plane_stride);
    const unsigned i3 = P.F == 4 ? quad_load(fr + 3 * P.plane_stride) : 0u;
    const uint8_t *gr = fr + (size_t)P.F * P.plane_stride;
    unsigned b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) a.code[k] = 0;
#pragma unroll 2
    for (int i = 0; i < N; i++) {
        const unsigned pos = quad_load(gr + (size_t)i * P.plane_stride), inv = quad_load(gr + (size_t)(N + i) * P.plane_stride);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] ^= quad_byte(pos, k) >= quad_byte(inv, k) ? 1u : 0u;  // 4/phase_unwrap.cpp:183, :187-191
            a.code[k] = a.code[k] * 2 + (int)b[k];                   // :193
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a.w[k] = a.unw[k] = 0.f;
        if (!(bits >> k & 1u)) continue;
        const float phi = wrapped_phase<false>(P.F, quad_byte(i0, k), quad_byte(i1, k), quad_byte(i2, k), quad_byte(i3, k), nullptr, K);
        const bool in_range = axis == 0 ? (gx0 + k >= 1 && gx0 + k <= P.fullW - 2) : (gy >= 1 && gy <= P.fullH - 2);  // :285 / :304
        if (in_range) {
            a.w[k] = shift_pi(phi);
            a.unw[k] = unwrap_value(a.w[k], a.code[k]);
        }
    }
}

// what the pixels of a quad at window (col0, row) bring into a neighbourhood of `axis` (period_request / period_staged): the absolute
// phase of a sample -- valid bit set, inside window columns 1..W-2 (vertical axis) or window rows 1..H-2 (horizontal) -- else +infinity
__device__ __forceinline__ f32x4 rpf_staged(const KParams &P, int axis, unsigned bits, int col0, int row, const float unw[4])
{
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool in_range = axis == 0 ? (col0 + k >= 1 && col0 + k <= P.W - 2) : (row >= 1 && row <= P.H - 2);
        s[k] = (bits >> k & 1u) && in_range ? unw[k] : period_no_sample();
    }
    return (f32x4){s[0], s[1], s[2], s[3]};
}

// k_period_jumps + k_period_apply of one pixel: v = its neighbourhood (v[4] the pixel itself), w / code / unw = what stage 4 left
__device__ __forceinline__ float rpf_repair(const float (&v)[2 * SL3D_RPF_RADIUS + 1], int n_gray, float w, int code, float unw)
{
    if (!(v[SL3D_RPF_RADIUS] < period_no_sample())) return unw;  // no sample
    int n;
    const float m = period_median<2 * SL3D_RPF_RADIUS + 1>(v, &n);
    const long j = period_sample_jump(v[SL3D_RPF_RADIUS], m, n, SL3D_RPF_RADIUS);
    if (j == 0) return unw;
    const long kk = (long)code - j;
    if (!period_in_range(kk, n_gray)) return unw;  // unrepairable
    return period_value(w, kk);
}

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (k_subpixel_fused)
template <bool SUB>
__global__ __launch_bounds__(SL3D_RPF_BLOCK) void k_repair_fused(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views,
                                                                 float *__restrict__ residual)
{
    __shared__ __attribute__((aligned(16))) float s_v[RPF_ROWS][RPF_RUN];   // vertical axis: tile columns -4 .. 67 of every tile row
    __shared__ __attribute__((aligned(16))) float s_h[RPF_BAND][RPF_COLS];  // horizontal axis: tile rows -4 .. 19
    const CONST_AS DevCal &C = *opaque_const(Cp);
    const int t = (int)threadIdx.x, q = t % RPF_QUADS, tr = t / RPF_QUADS;
    const int c0 = (int)blockIdx.x * RPF_COLS, r0 = (int)blockIdx.y * RPF_ROWS;
    const int col = c0 + 4 * q, row = r0 + tr;       // the lane's quad, padding columns included
    const bool owns = col < P.pitch && row < P.H;    // (the pitch is a multiple of 16: a quad is inside a row or outside it)
    const size_t px0 = owns ? (size_t)row * P.pitch + col : 0;
    const int gx0 = P.col0 + col, gy = P.row0 + row;
    // the halo quad the lane decodes besides its own: lanes 0..127 the horizontal axis (16 quads of the 4 rows above and the 4 below), lanes
    // 128..159 the vertical axis (the quad left and the quad right of every row) -- wave-uniform.  Outside the window: none
    const int haxis = t < RPF_HALO_H ? 1 : t < RPF_HALO_H + RPF_HALO_V ? 0 : -1;
    int hcol = 0, hrow = 0, hslot = 0;  // window position, and the staged row (axis 1) / the staged column (axis 0)
    if (haxis == 1) {
        const int hr = t / RPF_QUADS;  // 0..7
        hslot = hr < SL3D_RPF_RADIUS ? hr : hr + RPF_ROWS;
        hrow = r0 - SL3D_RPF_RADIUS + hslot, hcol = col;
    } else if (haxis == 0) {
        const int i = t - RPF_HALO_H;
        hslot = i & 1 ? RPF_RUN - 4 : 0;
        hrow = r0 + (i >> 1), hcol = c0 - SL3D_RPF_RADIUS + hslot;
    }
    const bool halo = haxis >= 0 && hcol >= 0 && hcol < P.pitch && hrow >= 0 && hrow < P.H && (haxis == 0 ? P.Nv : P.Nh) != 0;
    const size_t hpx0 = halo ? (size_t)hrow * P.pitch + hcol : 0;
    const bool decodes = P.F != 5;  // check_I_mod_criteria, 3/wrapped_phase.cpp:106-115: with 5 steps nothing is valid (k_wrap)
    const unsigned need = quad_need(P, decodes && owns, first_view, n_views, (unsigned)px0);
    double u[4], v[4];  // the camera side (written here: sl3d_quad.h, shape)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u[k] = v[k] = 0.0;
        if (need >> k & 1u) undistort_reproject((double)(gx0 + k), (double)gy, C.cam, u[k], v[k]);
    }
    PinnedRows PR;
    for (int j = 0; j < 4; j++) { PR.c2[j] = C.Ac[8 + j]; PR.p2[j] = C.Ap[8 + j]; }
    const AtanK K = atan_consts<false>();
    const float nanv = __builtin_nanf("");
    const f32x4 none = {period_no_sample(), period_no_sample(), period_no_sample(), period_no_sample()};
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const uint8_t *frames = P.frames + (size_t)view * P.view_stride;
        const unsigned bits = decodes && owns ? mask_quad_bits(load_mask_quad(P, view, (unsigned)px0)) : 0u;
        RpfAxis a0, a1;
        if (bits) {
            rpf_axis(P, frames + px0, 0, bits, gx0, gy, K, a0);
            rpf_axis(P, frames + px0, 1, bits, gx0, gy, K, a1);
        }
        *(f32x4 *)&s_v[tr][SL3D_RPF_RADIUS + 4 * q] = bits ? rpf_staged(P, 0, bits, col, row, a0.unw) : none;
        *(f32x4 *)&s_h[SL3D_RPF_RADIUS + tr][4 * q] = bits ? rpf_staged(P, 1, bits, col, row, a1.unw) : none;
        if (haxis >= 0) {
            const unsigned hbits = decodes && halo ? mask_quad_bits(load_mask_quad(P, view, (unsigned)hpx0)) : 0u;
            f32x4 s = none;
            if (hbits) {
                RpfAxis h;
                rpf_axis(P, frames + hpx0, haxis, hbits, P.col0 + hcol, P.row0 + hrow, K, h);
                s = rpf_staged(P, haxis, hbits, hcol, hrow, h.unw);
            }
            if (haxis == 1) *(f32x4 *)&s_h[hslot][4 * q] = s;
            else *(f32x4 *)&s_v[(t - RPF_HALO_H) >> 1][hslot] = s;
        }
        __syncthreads();
        float out[12], res[4];  // (quad_clear's statements)
#pragma unroll
        for (int j = 0; j < 12; j++) out[j] = nanv;
#pragma unroll
        for (int k = 0; k < 4; k++) res[k] = nanv;
        unsigned valid = 0u;
        if (bits) {
            if (P.Nv != 0) {  // (an axis without Gray planes is skipped: sl3d_repair_periods refuses it)
                float run[4 + 2 * SL3D_RPF_RADIUS];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const f32x4 x = *(const f32x4 *)&s_v[tr][4 * q + 4 * j];
                    run[4 * j] = x.x, run[4 * j + 1] = x.y, run[4 * j + 2] = x.z, run[4 * j + 3] = x.w;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float nb[2 * SL3D_RPF_RADIUS + 1];
#pragma unroll
                    for (int d = 0; d < 2 * SL3D_RPF_RADIUS + 1; d++) nb[d] = run[k + d];
                    a0.unw[k] = rpf_repair(nb, P.Nv, a0.w[k], a0.code[k], a0.unw[k]);
                }
            }
            if (P.Nh != 0) {
                float colv[2 * SL3D_RPF_RADIUS + 1][4];
#pragma unroll
                for (int d = 0; d < 2 * SL3D_RPF_RADIUS + 1; d++) {
                    const f32x4 x = *(const f32x4 *)&s_h[tr + d][4 * q];
                    colv[d][0] = x.x, colv[d][1] = x.y, colv[d][2] = x.z, colv[d][3] = x.w;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float nb[2 * SL3D_RPF_RADIUS + 1];
#pragma unroll
                    for (int d = 0; d < 2 * SL3D_RPF_RADIUS + 1; d++) nb[d] = colv[d][k];
                    a1.unw[k] = rpf_repair(nb, P.Nh, a1.w[k], a1.code[k], a1.unw[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(bits >> k & 1u)) continue;  // merge_valid_maps: both axes carry the valid byte of the boundary removal
                long cx, cy;
                if (!quad_correspond(P, a0.unw[k], a1.unw[k], cx, cy)) continue;
                // (quad_coordinate<false>'s and quad_solve<SUB>'s statements)
                // k_subpixel: the continuous projector coordinate; k_tri: the c_p_map's integers
                const double xs = SUB ? correspond_arg(a0.unw[k], P.fwv) : (double)cx, ys = SUB ? correspond_arg(a1.unw[k], P.fwh) : (double)cy;
                double up, vp, X[3];
                undistort_reproject(xs, ys, C.proj, up, vp);
                triangulate_px(C, PR, u[k], v[k], up, vp, X);
                if (SUB) {
                    double Ac[12], Ap[12];  // (subpixel_reproj_err2 takes a plain pointer: the matrices by value, scalar registers after inlining)
                    for (int j = 0; j < 12; j++) { Ac[j] = C.Ac[j]; Ap[j] = C.Ap[j]; }
                    res[k] = subpixel_residual(subpixel_reproj_err2(Ac, X, u[k], v[k]), subpixel_reproj_err2(Ap, X, up, vp));
                }
                out[3 * k + 0] = (float)X[0];
                out[3 * k + 1] = (float)X[1];
                out[3 * k + 2] = (float)X[2];
                valid |= 1u << (8 * k);
            }
        }
        if (owns) quad_store<SUB>(P, (size_t)view * P.px_view_stride + px0, out, res, valid, residual);
        __syncthreads();  // (every lane has read its neighbourhood: the next view may be staged)
    }
}

int launch_repair_fused(const KParams &P, const DevCal *C, int first_view, int n_views, float *residual, void *stream)
{
    const dim3 grid((unsigned)((P.pitch + RPF_COLS - 1) / RPF_COLS), (unsigned)((P.H + RPF_ROWS - 1) / RPF_ROWS));
    return quad_launch(residual ? k_repair_fused<true> : k_repair_fused<false>, grid, stream, P, C, first_view, n_views, residual);
}

}  // namespace sl3d
