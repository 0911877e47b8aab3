// sl3d_subpixel.hip -- gfx950 (MI355X, wave64) kernels of sl3d_triangulate_subpixel and sl3d_get_correspondences_subpixel:
// stage 7 from the CONTINUOUS projector coordinates -- the doubles stage 5 hands to lrint (correspond_arg) -- instead of the rounded
// c_p_map, with the reprojection residual of the 4 x 3 least-squares solve as a plane of its own and, on request, a rejection by it.
//   k_subpixel         all views of a call in one launch (the view in blockIdx.y), a pixel per lane.  Reads the merged valid byte and
//                      the two absolute phases (9 B/px), writes points, intersection_points and the residual (40 B/px) and, where a
//                      pixel is rejected, its valid byte.  Per pixel: the camera's and the projector's five-iteration undistortion
//                      (undistort_reproject -- the projector's at the continuous point, no table), the T2/T3 solve of k_tri
//                      (triangulate_px), two reprojections (sl3d_subpixel.h): fp64 VALU.  If the caller wants the counts, a block
//                      leaves its triangulated and rejected pixels as one word of `partials` -- a plain store
//   k_subpixel_counts  a block per view: the sum of the view's partial words -> counts[view][2].  No atomic add anywhere: one per wave
//                      and count on the views' two words cost more than the triangulation itself (measured)
//   k_subpixel_coords  (xs, ys) of one view into a scratch plane of double pairs, NaN where either axis valid byte is not 1
// k_subpixel and k_subpixel_coords have an ANCHOR instantiation each (SL3D_FLAG_ANCHOR_PERIODS): the coordinates come from
// the wrapped-phase and code planes of both axes (sl3d_anchor.h: anchor_coordinate) where stage 4's loop ran on an axis with Gray planes,
// from the absolute phase elsewhere -- about 25 B/px in instead of 9.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_anchor.h"
#include "sl3d_block.h"
#include "sl3d_device.h"
#include "sl3d_internal.h"
#include "sl3d_one_axis.h"
#include "sl3d_subpixel.h"

namespace sl3d {

// the continuous projector coordinate of one axis of pixel px of the planes, at column gx and row gy of the frame
template <bool ANCHOR>
__device__ __forceinline__ double subpixel_coordinate(const KParams &P, int axis, size_t px, int gx, int gy)
{
    const int fw = axis == 0 ? P.fwv : P.fwh;
    if (ANCHOR && (axis == 0 ? anchor_applies(P.Nv, gx, P.fullW) : anchor_applies(P.Nh, gy, P.fullH)))
        return anchor_coordinate(P.wrapped[axis][px], P.code[axis][px], fw, P.F);
    return correspond_arg(P.unwrapped[axis][px], fw);
}

// partials: NULL, or [gridDim.y][gridDim.x] words: triangulated pixels of the block | rejected ones << 16 (at most 256 of either)
template <bool ANCHOR>
__global__ __launch_bounds__(256) void k_subpixel(const KParams P, const DevCal C, int first_view, double max_residual, float *__restrict__ residual,
                                                  unsigned *__restrict__ partials)
{
    __shared__ unsigned s_cnt[4];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;  // pixel of the view, padding columns included
    const bool in_view = t < P.px_view_stride;
    const size_t px = (size_t)(first_view + (int)blockIdx.y) * P.px_view_stride + (in_view ? t : 0);
    const bool valid = in_view && P.valid[px] == 1;
    const float nanv = __builtin_nanf("");
    float x = nanv, y = nanv, z = nanv, res = nanv;
    double X[3] = {0, 0, 0};
    bool rejected = false;
    if (valid) {
        const int row = (int)(t / (size_t)P.pitch), col = (int)(t - (size_t)row * P.pitch);
        const int gx = P.col0 + col, gy = P.row0 + row;
        const double xs = subpixel_coordinate<ANCHOR>(P, 0, px, gx, gy), ys = subpixel_coordinate<ANCHOR>(P, 1, px, gx, gy);
        double u, v, up, vp;
        undistort_reproject((double)gx, (double)gy, C.cam, u, v);
        undistort_reproject(xs, ys, C.proj, up, vp);
        PinnedRows PR;
        for (int j = 0; j < 4; j++) { PR.c2[j] = C.Ac[8 + j]; PR.p2[j] = C.Ap[8 + j]; }
        triangulate_px(C, PR, u, v, up, vp, X);
        res = subpixel_residual(subpixel_reproj_err2(C.Ac, X, u, v), subpixel_reproj_err2(C.Ap, X, up, vp));
        rejected = subpixel_rejected(res, max_residual);
        if (rejected) {
            X[0] = X[1] = X[2] = 0.0;
            P.valid[px] = 0;
        } else {
            x = (float)X[0];
            y = (float)X[1];
            z = (float)X[2];
        }
    }
    if (in_view) {
        P.ipoints[3 * px + 0] = X[0];
        P.ipoints[3 * px + 1] = X[1];
        P.ipoints[3 * px + 2] = X[2];
        P.points[3 * px + 0] = x;
        P.points[3 * px + 1] = y;
        P.points[3 * px + 2] = z;
        residual[px] = res;
    }
    if (partials) {  // (a kernel argument: the whole block takes the branch or none of it)
        unsigned c = (valid ? 1u : 0u) | (rejected ? 1u << 16 : 0u);
        BLOCK_SUM(c, s_cnt);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
    }
}

__global__ __launch_bounds__(256) void k_subpixel_counts(const unsigned *__restrict__ partials, unsigned n_blocks, unsigned *__restrict__ counts)
{
    __shared__ unsigned s_tri[4], s_rej[4];
    unsigned tri = 0, rej = 0;
    for (unsigned i = threadIdx.x; i < n_blocks; i += 256) {
        const unsigned w = partials[(size_t)blockIdx.x * n_blocks + i];
        tri += w & 0xffffu;
        rej += w >> 16;
    }
    BLOCK_SUM(tri, s_tri);
    BLOCK_SUM(rej, s_rej);
    if (threadIdx.x == 0) {
        counts[2 * blockIdx.x + 0] = BLOCK_SUM_TOTAL(s_tri);
        counts[2 * blockIdx.x + 1] = BLOCK_SUM_TOTAL(s_rej);
    }
}

template <bool ANCHOR>
__global__ __launch_bounds__(256) void k_subpixel_coords(const KParams P, int view, double *__restrict__ xy)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P.px_view_stride) return;
    const size_t px = (size_t)view * P.px_view_stride + t;
    const double nand = __builtin_nan("");
    double xs = nand, ys = nand;
    if (P.valid_axis[0][px] == 1 && P.valid_axis[1][px] == 1) {  // merge_valid_maps: the pixels stage 5 forms the doubles of
        const int row = (int)(t / (size_t)P.pitch), col = (int)(t - (size_t)row * P.pitch);
        xs = subpixel_coordinate<ANCHOR>(P, 0, px, P.col0 + col, P.row0 + row);
        ys = subpixel_coordinate<ANCHOR>(P, 1, px, P.col0 + col, P.row0 + row);
    }
    xy[2 * t + 0] = xs;
    xy[2 * t + 1] = ys;
}

// The one-axis forms (SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL; sl3d_one_axis.h): k_subpixel_one triangulates from the continuous
// coordinate of axis AXIS alone -- the exactly determined ray-plane solve, no residual, nothing to reject -- and reads no plane of the other
// axis; k_subpixel_coords_one leaves NaN in the other component.
template <int AXIS, bool ANCHOR>
__global__ __launch_bounds__(256) void k_subpixel_one(const KParams P, const DevCal C, int first_view, unsigned *__restrict__ partials)
{
    __shared__ unsigned s_cnt[4];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;  // pixel of the view, padding columns included
    const bool in_view = t < P.px_view_stride;
    const size_t px = (size_t)(first_view + (int)blockIdx.y) * P.px_view_stride + (in_view ? t : 0);
    const bool valid = in_view && P.valid[px] == 1;
    const float nanv = __builtin_nanf("");
    float x = nanv, y = nanv, z = nanv;
    double X[3] = {0, 0, 0};
    if (valid) {
        const int row = (int)(t / (size_t)P.pitch), col = (int)(t - (size_t)row * P.pitch);
        const int gx = P.col0 + col, gy = P.row0 + row;
        const double s = subpixel_coordinate<ANCHOR>(P, AXIS, px, gx, gy);
        double u, v;
        undistort_reproject((double)gx, (double)gy, C.cam, u, v);
        const double tp = one_axis_project(s, C.proj.K[AXIS == 0 ? 0 : 4], AXIS == 0 ? C.proj.ifx : C.proj.ify, AXIS == 0 ? C.proj.cx : C.proj.cy);
        one_axis_solve(C.Ac, C.Ap, AXIS, u, v, tp, X);
        x = (float)X[0];
        y = (float)X[1];
        z = (float)X[2];
    }
    if (in_view) {
        P.ipoints[3 * px + 0] = X[0];
        P.ipoints[3 * px + 1] = X[1];
        P.ipoints[3 * px + 2] = X[2];
        P.points[3 * px + 0] = x;
        P.points[3 * px + 1] = y;
        P.points[3 * px + 2] = z;
    }
    if (partials) {  // (a kernel argument: the whole block takes the branch or none of it)
        unsigned c = valid ? 1u : 0u;
        BLOCK_SUM(c, s_cnt);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = BLOCK_SUM_TOTAL(s_cnt);
    }
}

template <int AXIS, bool ANCHOR>
__global__ __launch_bounds__(256) void k_subpixel_coords_one(const KParams P, int view, double *__restrict__ xy)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P.px_view_stride) return;
    const size_t px = (size_t)view * P.px_view_stride + t;
    const double nand = __builtin_nan("");
    double s = nand;
    if (P.valid_axis[AXIS][px] == 1) {
        const int row = (int)(t / (size_t)P.pitch), col = (int)(t - (size_t)row * P.pitch);
        s = subpixel_coordinate<ANCHOR>(P, AXIS, px, P.col0 + col, P.row0 + row);
    }
    xy[2 * t + AXIS] = s;
    xy[2 * t + (1 - AXIS)] = nand;
}

unsigned subpixel_blocks(const KParams &P) { return (unsigned)((P.px_view_stride + 255) / 256); }

int launch_subpixel(const KParams &P, const DevCal &C, int first_view, int n_views, double max_residual, float *residual, unsigned *partials,
                    unsigned *counts, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const unsigned n_blocks = subpixel_blocks(P);
    const dim3 grid(n_blocks, (unsigned)n_views);
    if (anchor) hipLaunchKernelGGL(k_subpixel<true>, grid, dim3(256), 0, (hipStream_t)stream, P, C, first_view, max_residual, residual, partials);
    else hipLaunchKernelGGL(k_subpixel<false>, grid, dim3(256), 0, (hipStream_t)stream, P, C, first_view, max_residual, residual, partials);
    int e = (int)hipGetLastError();
    if (e || !partials) return e;
    hipLaunchKernelGGL(k_subpixel_counts, dim3((unsigned)n_views), dim3(256), 0, (hipStream_t)stream, partials, n_blocks, counts);
    return (int)hipGetLastError();
}

int launch_subpixel_coords(const KParams &P, int view, double *xy, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const dim3 grid((unsigned)((P.px_view_stride + 255) / 256));
    if (anchor) hipLaunchKernelGGL(k_subpixel_coords<true>, grid, dim3(256), 0, (hipStream_t)stream, P, view, xy);
    else hipLaunchKernelGGL(k_subpixel_coords<false>, grid, dim3(256), 0, (hipStream_t)stream, P, view, xy);
    return (int)hipGetLastError();
}

int launch_subpixel_one(const KParams &P, const DevCal &C, int axis, int first_view, int n_views, unsigned *partials, unsigned *counts, bool anchor,
                        void *stream)
{
    (void)hipGetLastError();
    const unsigned n_blocks = subpixel_blocks(P);
    const dim3 grid(n_blocks, (unsigned)n_views);
#define SL3D_ONE(AXIS, ANCHOR) hipLaunchKernelGGL((k_subpixel_one<AXIS, ANCHOR>), grid, dim3(256), 0, (hipStream_t)stream, P, C, first_view, partials)
    if (axis == 0) { if (anchor) SL3D_ONE(0, true); else SL3D_ONE(0, false); }
    else { if (anchor) SL3D_ONE(1, true); else SL3D_ONE(1, false); }
#undef SL3D_ONE
    int e = (int)hipGetLastError();
    if (e || !partials) return e;
    hipLaunchKernelGGL(k_subpixel_counts, dim3((unsigned)n_views), dim3(256), 0, (hipStream_t)stream, partials, n_blocks, counts);
    return (int)hipGetLastError();
}

int launch_subpixel_coords_one(const KParams &P, int axis, int view, double *xy, bool anchor, void *stream)
{
    (void)hipGetLastError();
    const dim3 grid((unsigned)((P.px_view_stride + 255) / 256));
#define SL3D_ONE(AXIS, ANCHOR) hipLaunchKernelGGL((k_subpixel_coords_one<AXIS, ANCHOR>), grid, dim3(256), 0, (hipStream_t)stream, P, view, xy)
    if (axis == 0) { if (anchor) SL3D_ONE(0, true); else SL3D_ONE(0, false); }
    else { if (anchor) SL3D_ONE(1, true); else SL3D_ONE(1, false); }
#undef SL3D_ONE
    return (int)hipGetLastError();
}

}  // namespace sl3d
