// sl3d_modulation.h -- the fringe-modulation test that rejects shadow and background pixels (the criterion the reference wrote as
// check_I_mod_criteria under "another criteria to eliminate shadow+background", 3/wrapped_phase.cpp:63-104, and left commented out):
// the per-pixel modulation gamma of one axis and the selection test built on it.
//
// Shared by k_modulation_select / k_modulation_gamma (sl3d_modulation.hip) and by the CPU check the test suite runs over every
// (I0, I1, I2) triple (tests/native/modulation_check.cpp): plain C, no HIP types.
//
// The literal arithmetic of 3/wrapped_phase.cpp:92-94, with the three fringe bytes of one axis:
//   d  = I0 - I2,  e = 2*I1 - I0 - I2                 integers, exact
//   t1 = sqrtf((float)(3*d*d + e*e))                  the argument is an integer <= 455175 < 2^24: the cast is exact
//   t2 = (float)(I0 + I1 + I2)
//   gamma = t1 / t2                                   t2 == 0 (a black pixel) gives 0/0 = NaN
// Both operations are correctly rounded on the host and, compiled without fast-math and without approximate intrinsics, on gfx950
// (v_sqrt_f32 + its fma fix-up, v_div_scale / v_div_fmas / v_div_fixup): gamma is the same float everywhere.
//
// The selection (the comparison in double and strict, as 3/wrapped_phase.cpp:96; NaN never passes):
//   selected = (no mask || mask byte == 1) && (double)gamma_v > thr && (double)gamma_h > thr
// Unlike the reference's (never run) per-axis test, the two axes are ANDed into ONE selection per view before stage 3's boundary
// removal: every kernel of this library works on one selection per view.
#pragma once

#ifdef __HIPCC__
#define SL3D_MOD_FN __host__ __device__ __forceinline__
#else
#define SL3D_MOD_FN static inline
#endif

#include <math.h>

// gamma of one axis from its three fringe bytes
SL3D_MOD_FN float mod_gamma(int i0, int i1, int i2)
{
    const int d = i0 - i2, e = 2 * i1 - i0 - i2;
    const float t1 = sqrtf((float)(3 * d * d + e * e));
    const float t2 = (float)(i0 + i1 + i2);
    return t1 / t2;
}

// the test of one axis: strictly above the threshold, compared in double (false for NaN)
SL3D_MOD_FN int mod_pass(float gamma, double thr) { return (double)gamma > thr; }

// the selection of one pixel: mask_selected (the caller's byte == 1, or 1 without a mask) and both axes well modulated
SL3D_MOD_FN int mod_select(int mask_selected, float gamma_v, float gamma_h, double thr)
{
    return (mask_selected != 0) & mod_pass(gamma_v, thr) & mod_pass(gamma_h, thr);  // (no short cut: no branch per lane)
}
