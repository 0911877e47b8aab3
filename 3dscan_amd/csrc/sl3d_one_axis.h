// sl3d_one_axis.h -- the one-axis scan of SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL: a pixel triangulated from ONE
// continuous projector coordinate.  A projector column (or row) is a plane in space and a camera pixel is a ray: three equations, three
// unknowns, an exactly determined 3 x 3 system instead of stage 7's 4 x 3 least squares -- and therefore no residual.
//
// Shared by k_corr_one / k_subpixel_one / k_subpixel_coords_one (sl3d_one_axis.hip, the staged route), k_one_axis (the same unit, the timed
// route), sl3d_create / sl3d_group_create / sl3d_set_calibration (the refusals) and the CPU check the test suite runs
// (tests/native/one_axis_check.cpp): plain C++, no HIP types.  Both device routes call one_axis_project and one_axis_solve with the same
// arguments, so they agree bit for bit.
//
// With a the coded axis (0: the projector column, 1: the row), s its continuous coordinate, (u, v) the undistorted camera point, Ac / Ap the
// 3 x 4 projection matrices (row major), all in IEEE double, fma where written, nothing else contracted:
//   t    = fma(f_a, (s - c_a) * (1.0 / f_a), c_a)       f_a, c_a = Kp[0], Kp[2] (a = 0) or Kp[4], Kp[5] (a = 1): what undistort + re-project
//                                                       returns for that coordinate on a plain, undistorted projector, whatever the other is
//   r0j  = fma(-u, Ac[2][j], Ac[0][j])   f0 = fma(Ac[2][3], u, -Ac[0][3])          j = 0..2
//   r1j  = fma(-v, Ac[2][j], Ac[1][j])   f1 = fma(Ac[2][3], v, -Ac[1][3])
//   r2j  = fma(-t, Ap[2][j], Ap[a][j])   f2 = fma(Ap[2][3], t, -Ap[a][3])
//   c0 = r1 x r2, c1 = r2 x r0, c2 = r0 x r1            each component fma(p, q, -(r * s)) in the cyclic order written in one_axis_cross
//   det  = fma(r0[0], c0[0], fma(r0[1], c0[1], r0[2] * c0[2]))
//   n_j  = fma(f0, c0[j], fma(f1, c1[j], f2 * c2[j]))   (the adjugate's columns are the cross products of the rows)
//   X_j  = n_j * (1.0 / det);  det == 0: X = 0 (the valid byte stays, as in stage 7)
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SL3D_ONE_AXIS_FN __host__ __device__ __forceinline__
#else
#define SL3D_ONE_AXIS_FN static inline
#endif

#include <math.h>

// the coded axis of a flag word: 0 (SL3D_FLAG_ONLY_VERTICAL), 1 (SL3D_FLAG_ONLY_HORIZONTAL), -1: a two-axis context
#define SL3D_ONE_AXIS_VERTICAL_BIT 1024u
#define SL3D_ONE_AXIS_HORIZONTAL_BIT 2048u
SL3D_ONE_AXIS_FN int one_axis_of_flags(unsigned flags)
{
    return (flags & SL3D_ONE_AXIS_VERTICAL_BIT) ? 0 : (flags & SL3D_ONE_AXIS_HORIZONTAL_BIT) ? 1 : -1;
}

// The refusal of a flag combination by sl3d_create / sl3d_group_create, before a device is touched: NULL, or the text that goes with
// SL3D_E_UNSUPPORTED
SL3D_ONE_AXIS_FN const char *one_axis_refusal(bool only_v, bool only_h, bool subpixel, bool repair)
{
    if (!only_v && !only_h) return 0;
    if (only_v && only_h)
        return "SL3D_FLAG_ONLY_VERTICAL | SL3D_FLAG_ONLY_HORIZONTAL is not supported: a one-axis scan reads one pattern direction (choose one of the two "
               "flags, or drop both for the two-axis scan)";
    if (!subpixel)
        return only_v ? "SL3D_FLAG_ONLY_VERTICAL needs SL3D_FLAG_SUBPIXEL: the one-axis solve takes the continuous coordinate (add SL3D_FLAG_SUBPIXEL, or drop "
                        "the flag)"
                      : "SL3D_FLAG_ONLY_HORIZONTAL needs SL3D_FLAG_SUBPIXEL: the one-axis solve takes the continuous coordinate (add SL3D_FLAG_SUBPIXEL, or "
                        "drop the flag)";
    if (repair)
        return only_v ? "SL3D_FLAG_ONLY_VERTICAL | SL3D_FLAG_REPAIR_PERIODS is not supported: the fused period repair has no one-axis form (drop one of "
                        "the two flags)"
                      : "SL3D_FLAG_ONLY_HORIZONTAL | SL3D_FLAG_REPAIR_PERIODS is not supported: the fused period repair has no one-axis form (drop one of "
                        "the two flags)";
    return 0;
}

// The refusal of a calibration by sl3d_set_calibration on a one-axis context: NULL, or the text that goes with SL3D_E_UNSUPPORTED.  With
// the other coordinate unknown, a column of a distorted (or skewed, or perspective) projector is a curve in the undistorted image, not a line.
SL3D_ONE_AXIS_FN const char *one_axis_calibration_refusal(int axis, const double Kp[9], const double dp[5])
{
    if (axis < 0) return 0;
    const bool distorted = dp[0] != 0 || dp[1] != 0 || dp[2] != 0 || dp[3] != 0 || dp[4] != 0;
    const bool plain = Kp[1] == 0 && Kp[3] == 0 && Kp[6] == 0 && Kp[7] == 0 && Kp[8] == 1;
    if (distorted)
        return axis == 0 ? "set_calibration: SL3D_FLAG_ONLY_VERTICAL needs an undistorted projector (every dp == 0): the other coordinate is unknown, so a "
                           "distorted column is a curve and not a line; the previous calibration stays in force"
                         : "set_calibration: SL3D_FLAG_ONLY_HORIZONTAL needs an undistorted projector (every dp == 0): the other coordinate is unknown, so a "
                           "distorted row is a curve and not a line; the previous calibration stays in force";
    if (!plain)
        return axis == 0 ? "set_calibration: SL3D_FLAG_ONLY_VERTICAL needs a plain projector matrix (Kp[1] = Kp[3] = Kp[6] = Kp[7] = 0, Kp[8] = 1): the other "
                           "coordinate is unknown, so a column is a curve and not a line of its own; the previous calibration stays in force"
                         : "set_calibration: SL3D_FLAG_ONLY_HORIZONTAL needs a plain projector matrix (Kp[1] = Kp[3] = Kp[6] = Kp[7] = 0, Kp[8] = 1): the other "
                           "coordinate is unknown, so a row is a curve and not a line of its own; the previous calibration stays in force";
    return 0;
}

// t: the undistorted, re-projected coordinate of s on a plain, undistorted projector.  f, inv_f = 1.0 / f, c: Kp[0], Kp[2] or Kp[4], Kp[5]
SL3D_ONE_AXIS_FN double one_axis_project(double s, double f, double inv_f, double c) { return fma(f, (s - c) * inv_f, c); }

SL3D_ONE_AXIS_FN void one_axis_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = fma(a[1], b[2], -(a[2] * b[1]));
    c[1] = fma(a[2], b[0], -(a[0] * b[2]));
    c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

// X of the ray of (u, v) and the plane of coordinate t of axis `axis`.  Ac, Ap: anything that indexes as 12 doubles, row major
template <typename AC, typename AP>
SL3D_ONE_AXIS_FN void one_axis_solve(AC Ac, AP Ap, int axis, double u, double v, double t, double X[3])
{
    double r0[3], r1[3], r2[3];
    for (int j = 0; j < 3; j++) {
        r0[j] = fma(-u, Ac[8 + j], Ac[j]);
        r1[j] = fma(-v, Ac[8 + j], Ac[4 + j]);
        r2[j] = fma(-t, Ap[8 + j], Ap[4 * axis + j]);
    }
    const double f0 = fma(Ac[11], u, -Ac[3]), f1 = fma(Ac[11], v, -Ac[7]), f2 = fma(Ap[11], t, -Ap[4 * axis + 3]);
    double c0[3], c1[3], c2[3];
    one_axis_cross(r1, r2, c0);
    one_axis_cross(r2, r0, c1);
    one_axis_cross(r0, r1, c2);
    const double det = fma(r0[0], c0[0], fma(r0[1], c0[1], r0[2] * c0[2]));
    const double rdet = det != 0.0 ? 1.0 / det : 0.0;
    for (int j = 0; j < 3; j++) X[j] = fma(f0, c0[j], fma(f1, c1[j], f2 * c2[j])) * rdet;
}
