// sl3d_subpixel_fused.hip -- gfx950 (MI355X, wave64): the sub-pixel scan of a timed context in ONE launch (SL3D_FLAG_SUBPIXEL without
// SL3D_FLAG_KEEP_STAGES).  k_subpixel_fused leaves in the points, valid and residual planes of the launch's views, bit for
// bit, what k_wrap, k_unwrap (both axes), k_corr and k_subpixel(+inf) leave there on a SL3D_FLAG_KEEP_STAGES context -- without any of
// the stage planes between them: per pixel the frames -> stage 3 (wrapped_phase) -> stage 4 (Gray decode, shift_pi, unwrap_value) ->
// stage 5 (correspond: the merged valid byte; correspond_arg: the continuous projector coordinate) -> undistort_reproject of both
// devices -> triangulate_px -> subpixel_reproj_err2 / subpixel_residual.
//   ANCHOR  k_subpixel_fused<true> (SL3D_FLAG_ANCHOR_PERIODS): the solve takes the anchored coordinates (sl3d_anchor.h) from the
//           shifted wrapped phase and the code where k_subpixel<true> takes them; the absolute phase still decides the valid byte.
//   shape   the quad-per-lane kernel of sl3d_quad.h, every piece from there: both axes of the quad are decoded (quad_axis), then solved pixel
//           by pixel.  Both instantiations are the same text; the one without ANCHOR never reads the shifted phase or the code again.
//   memory  sl3d_quad.h's; per pixel and view 2 F + 2 (Nv + Nh) frame bytes in, the residual out.
// Compiled with -ffp-contract=off.
#include "sl3d_quad.h"

namespace sl3d {

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (as a kernel argument its 93
// doubles were loaded up front: 180 VGPRs with 128 SGPRs spilled into them, 2 waves per SIMD; this way 117 VGPRs, 4 waves)
template <bool ANCHOR>
__global__ __launch_bounds__(SL3D_QUAD_BLOCK) void k_subpixel_fused(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views,
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
    for (int j = 0; j < 4; j++) { PR.c2[j] = C.Ac[8 + j]; PR.p2[j] = C.Ap[8 + j]; }
    const AtanK K = atan_consts<false>();
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const size_t px = (size_t)view * P.px_view_stride + q.px0;
        const unsigned bits = q.decodes ? mask_quad_bits(load_mask_quad(P, view, lane_off)) : 0u;
        float out[12], res[4];
        unsigned valid;
        quad_clear<true>(out, res, valid);
        if (bits) {
            const uint8_t *quad = P.frames + (size_t)view * P.view_stride + q.px0;
            QuadAxis A0, A1;
            float unw0[4], unw1[4], w0[4], w1[4];
            quad_axis(P, quad, 0, bits, q.gx0, q.gy, K, A0, w0, unw0);
            quad_axis(P, quad, 1, bits, q.gx0, q.gy, K, A1, w1, unw1);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(bits >> k & 1u)) continue;
                long cx, cy;
                if (!quad_correspond(P, unw0[k], unw1[k], cx, cy)) continue;
                const double xs = quad_coordinate<ANCHOR>(P, 0, unw0[k], w0[k], A0.code[k], q.gx0 + k, q.gy);
                const double ys = quad_coordinate<ANCHOR>(P, 1, unw1[k], w1[k], A1.code[k], q.gx0 + k, q.gy);
                quad_solve<true>(C, PR, xs, ys, u[k], v[k], k, out, res, valid);
            }
        }
        quad_store<true>(P, px, out, res, valid, residual);
    }
}

int launch_subpixel_fused(const KParams &P, const DevCal *C, int first_view, int n_views, float *residual, bool anchor, void *stream)
{
    return quad_launch(anchor ? k_subpixel_fused<true> : k_subpixel_fused<false>, quad_grid(P), stream, P, C, first_view, n_views, residual);
}

}  // namespace sl3d
