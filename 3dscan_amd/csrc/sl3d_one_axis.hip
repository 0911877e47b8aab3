// sl3d_one_axis.hip -- gfx950 (MI355X, wave64): the one-axis scan of a timed context in ONE launch (SL3D_FLAG_ONLY_VERTICAL /
// SL3D_FLAG_ONLY_HORIZONTAL with SL3D_FLAG_SUBPIXEL, without SL3D_FLAG_KEEP_STAGES).  k_one_axis<AXIS, ANCHOR> leaves in the
// points and valid planes of the launch's views, bit for bit, what k_wrap and k_unwrap of axis AXIS, k_corr_one and k_subpixel_one leave
// there on a SL3D_FLAG_KEEP_STAGES context: per pixel the frames of ONE pattern direction -> stage 3 (wrapped_phase) -> stage 4 (Gray
// decode, shift_pi, unwrap_value) -> stage 5 (correspond of that axis: the merged valid byte; correspond_arg or, with ANCHOR,
// anchor_coordinate: the continuous coordinate) -> one_axis_project -> one_axis_solve, the exactly determined ray-plane intersection
// (sl3d_one_axis.h).  No frame of the other axis is read; there is no residual.
//   shape   the quad-per-lane kernel of sl3d_quad.h, its pieces from there: the coded axis of the quad is decoded (quad_decode), then a
//           pixel goes from its phase (written here, see below) to its point (quad_solve_one) before the next one starts.
//   memory  sl3d_quad.h's; per pixel and view F + 2 N frame bytes of the coded axis in.
// Compiled with -ffp-contract=off.
#include "sl3d_quad.h"

namespace sl3d {

// Cp: the context's device copy of the calibration, read through scalar loads where a constant is used (k_subpixel_fused)
template <int AXIS, bool ANCHOR>
__global__ __launch_bounds__(SL3D_QUAD_BLOCK) void k_one_axis(const KParams P, const DevCal *__restrict__ Cp, int first_view, int n_views)
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
    const AtanK K = atan_consts<false>();
#pragma unroll 1
    for (int vi = 0; vi < n_views; vi++) {
        const int view = first_view + vi;
        const size_t px = (size_t)view * P.px_view_stride + q.px0;
        const unsigned bits = q.decodes ? mask_quad_bits(load_mask_quad(P, view, lane_off)) : 0u;
        float out[12];
        unsigned valid;
        quad_clear<false>(out, nullptr, valid);
        if (bits) {
            QuadAxis A;  // the planes of the coded axis alone: F fringe planes, then N Gray planes and their N inverses
            quad_decode(P, P.frames + (size_t)view * P.view_stride + q.px0, AXIS, A);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(bits >> k & 1u)) continue;  // the valid byte of stage 3's boundary removal
                // quad_phase's statements (as a call the anchored forms gain 4 v_mov_b64 and lose 4 v_cvt_f64_f32: profiles/quad_kernels_isa.txt)
                const float phi = wrapped_phase<false>(P.F, quad_byte(A.i0, k), quad_byte(A.i1, k), quad_byte(A.i2, k), quad_byte(A.i3, k), nullptr, K);
                const int pos = AXIS == 0 ? q.gx0 + k : q.gy, full = AXIS == 0 ? P.fullW : P.fullH;
                const bool in_range = pos >= 1 && pos <= full - 2;  // :285 / :304
                const float w = in_range ? shift_pi(phi) : 0.f;
                const float unw = in_range ? unwrap_value(w, A.code[k]) : 0.f;
                if (!quad_correspond_one(P, AXIS, unw)) continue;
                quad_solve_one<AXIS>(C, quad_coordinate<ANCHOR>(P, AXIS, unw, w, A.code[k], q.gx0 + k, q.gy), u[k], v[k], k, out, valid);
            }
        }
        quad_store<false>(P, px, out, nullptr, valid, nullptr);
    }
}

int launch_one_axis(const KParams &P, const DevCal *C, int axis, int first_view, int n_views, bool anchor, void *stream)
{
    static void (*const kernel[2][2])(KParams, const DevCal *, int, int) = {{k_one_axis<0, false>, k_one_axis<0, true>},
                                                                            {k_one_axis<1, false>, k_one_axis<1, true>}};
    return quad_launch(kernel[axis != 0][anchor], quad_grid(P), stream, P, C, first_view, n_views);
}

}  // namespace sl3d
