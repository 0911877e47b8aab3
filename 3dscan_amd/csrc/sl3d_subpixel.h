// sl3d_subpixel.h -- the sub-pixel triangulation (sl3d_triangulate_subpixel): the reprojection residual of one pixel, the
// rejection rule and the argument checks of the entry point.
//
// Shared by k_subpixel (sl3d_subpixel.hip), by sl3d_capi_subpixel.cpp and by the CPU check the test suite runs
// (tests/native/subpixel_check.cpp): plain C++, no HIP types.
//
// Per pixel whose merged valid byte is 1, with (xs, ys) the doubles stage 5 hands to lrint (sl3d_device.h: correspond_arg), (u, v) /
// (u', v') the undistorted camera / projector point and X the least-squares point of stage 7 at (u, v, u', v'):
//   h = A_D * (X, 1),  e_D = (h0 / h2 - u_D, h1 / h2 - v_D)   for D = camera, projector (A_D: the 3 x 4 projection matrix, row-major)
//   residual = (float)sqrt(e_c . e_c + e_p . e_p)             the reprojection error in undistorted pixels, both devices together
//   rejected iff max_residual is finite and !((double)residual <= max_residual) -- on the STORED float: a NaN residual is rejected
#pragma once

#ifdef __HIPCC__
#define SL3D_SUBPIXEL_FN __host__ __device__ __forceinline__
#else
#define SL3D_SUBPIXEL_FN static inline
#endif

#include <math.h>

// e_D . e_D of one device: the squared distance between the projection of X by A (3 x 4, row-major) and the undistorted point (u, v)
SL3D_SUBPIXEL_FN double subpixel_reproj_err2(const double *A, const double X[3], double u, double v)
{
    const double h0 = fma(A[0], X[0], fma(A[1], X[1], fma(A[2], X[2], A[3])));
    const double h1 = fma(A[4], X[0], fma(A[5], X[1], fma(A[6], X[2], A[7])));
    const double h2 = fma(A[8], X[0], fma(A[9], X[1], fma(A[10], X[2], A[11])));
    const double ih = 1.0 / h2;
    const double eu = fma(h0, ih, -u), ev = fma(h1, ih, -v);
    return fma(eu, eu, ev * ev);
}

// the stored residual of a pixel from the two devices' squared errors
SL3D_SUBPIXEL_FN float subpixel_residual(double err2_cam, double err2_proj) { return (float)sqrt(err2_cam + err2_proj); }

// does the call reject at all?  (+infinity: never)
SL3D_SUBPIXEL_FN bool subpixel_rejects(double max_residual) { return max_residual < (double)__builtin_inff(); }

// the rejection of a pixel, on the stored float (a NaN residual compares false: rejected)
SL3D_SUBPIXEL_FN bool subpixel_rejected(float residual, double max_residual) { return subpixel_rejects(max_residual) && !((double)residual <= max_residual); }

// The argument checks of sl3d_triangulate_subpixel in the order the entry point makes them (views, KEEP_STAGES, max_residual,
// calibration): 0 or the status to return, in the values of include/sl3d.h (SL3D_E_INVALID_ARG -1, SL3D_E_STATE -4)
SL3D_SUBPIXEL_FN int subpixel_check_args(int first_view, int n_views, int max_views, int keep, int have_cal, double max_residual)
{
    if (first_view < 0 || n_views < 1 || first_view > max_views - n_views) return -1;
    if (!keep) return -4;
    if (!(max_residual > 0.0)) return -1;  // (NaN compares false)
    if (!have_cal) return -4;
    return 0;
}
