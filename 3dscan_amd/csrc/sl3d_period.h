// sl3d_period.h -- the repair of 2*Pi period jumps of the absolute phase (sl3d_repair_periods): the arithmetic of one pixel and
// the argument checks of the entry point.
//
// Shared by k_period_jumps / k_period_apply (sl3d_period.hip), by sl3d_capi_period.cpp and by the CPU check the test suite runs
// (tests/native/period_check.cpp): plain C++, no HIP types.
//
// A SAMPLE of axis a is a pixel whose axis valid byte is 1 and that lies where stage 4 defines the absolute phase (window columns 1..W-2
// for the vertical axis, window rows 1..H-2 for the horizontal one).  Per sample p, from the planes as they were when the call was
// enqueued, with the 2*radius + 1 pixels along the coded direction around p (p included, clipped to the window):
//   S  = the absolute phases of the samples among them, n = |S|;   n < radius + 1: p is left alone
//   m  = the lower median of S (element (n - 1) / 2 of S sorted ascending)
//   j  = (long)rint(((double)u_p - (double)m) / ((2.0 * 22.0) / 7.0))       half to even;   j == 0: p is left alone
//   k' = code_p - j;   k' < 0 or k' >= 2^N: p is left alone and counted as unrepairable
//   else code_p = k', u_p = (float)((double)wrapped_p + (((double)k' * 2.0) * 22.0) / 7.0) (stage 4's expression), counted as repaired
// A pixel that is no sample enters the kernels' windows as +infinity: it is never below anything, so it is counted out of n and never
// selected.  Every absolute phase is finite.
#pragma once

#ifdef __HIPCC__
#define SL3D_PERIOD_FN __host__ __device__ __forceinline__
#define SL3D_PERIOD_UNROLL _Pragma("unroll")
#else
#define SL3D_PERIOD_FN static inline
#define SL3D_PERIOD_UNROLL
#endif

#include <math.h>

#define SL3D_PERIOD_MAX_RADIUS 8
#define SL3D_PERIOD_WIDE (-128)  // this value in the jump plane says: j does not fit a byte, it is in the wide plane

// what a pixel that is no sample holds in a window
SL3D_PERIOD_FN float period_no_sample() { return __builtin_inff(); }

// The lower median of the finite values among v[0 .. K) (the others are +infinity), and their number in *n.  Selection by counting: the
// rank of v[i] in the ascending order that keeps equal values in index order is  #{j > i: v[j] < v[i]} + #{j < i: v[j] <= v[i]}  -- one
// comparison per pair, a = v[j] < v[i] for i < j, counted up for i and down for j -- the ranks are a permutation of 0 .. K - 1, the
// infinities take the last ones, and the median is the value of rank (n - 1) / 2.  Equal floats need no tie rule of the definition's:
// whichever of them has that rank, the value is the same.  K is a compile-time constant and every loop unrolls: v stays in registers.
// n == 0: +infinity.  One comparison and two additions per pair matter: at radius 8 the kernels are bound by them.
template <int K>
SL3D_PERIOD_FN float period_median(const float (&v)[K], int *n)
{
    int up[K], down[K], cnt = 0;
SL3D_PERIOD_UNROLL
    for (int i = 0; i < K; i++) {
        up[i] = down[i] = 0;
        cnt += v[i] < period_no_sample() ? 1 : 0;
    }
SL3D_PERIOD_UNROLL
    for (int i = 0; i < K; i++)
SL3D_PERIOD_UNROLL
        for (int j = i + 1; j < K; j++) {
            const int a = v[j] < v[i] ? 1 : 0;
            up[i] += a, down[j] += a;
        }
    const int t = (cnt - 1) / 2;
    float m = period_no_sample();
SL3D_PERIOD_UNROLL
    for (int i = 0; i < K; i++)
        if (up[i] + i - down[i] == t) m = v[i];
    *n = cnt;
    return m;
}

// j of a sample with absolute phase u and neighbourhood median m.  |u - m| < 3 is less than 0.4773 periods, which rounds to 0: the
// division is left out there, with the same result
SL3D_PERIOD_FN long period_jump(float u, float m)
{
    const double d = (double)u - (double)m;
    if (fabs(d) < 3.0) return 0;
    return (long)rint(d / ((2.0 * 22.0) / 7.0));
}

// j of a sample whose neighbourhood holds n samples with median m; 0: the pixel is left alone
SL3D_PERIOD_FN long period_sample_jump(float u, float m, int n, int radius) { return n < radius + 1 ? 0 : period_jump(u, m); }

// can code k be stored for an axis of n_gray Gray planes?  If not the pixel is unrepairable
SL3D_PERIOD_FN bool period_in_range(long k, int n_gray) { return k >= 0 && k < (1L << n_gray); }

// the absolute phase of code k: stage 4's expression with its operation order (4/phase_unwrap.cpp:291 / :309)
SL3D_PERIOD_FN float period_value(float wrapped_shifted, long k) { return (float)((double)wrapped_shifted + (((double)k * 2.0) * 22.0) / 7.0); }

// what the jump plane holds for a repaired pixel's j: j itself, or SL3D_PERIOD_WIDE (N >= 8 only: |j| < 2^N)
SL3D_PERIOD_FN int period_byte(long j) { return j >= -127 && j <= 127 ? (int)j : SL3D_PERIOD_WIDE; }

// The argument checks of sl3d_repair_periods in the order the entry point makes them (view, KEEP_STAGES, axis, radius, N of the axis):
// 0 or the status to return, in the values of include/sl3d.h (SL3D_E_INVALID_ARG -1, SL3D_E_STATE -4, SL3D_E_UNSUPPORTED -5)
SL3D_PERIOD_FN int period_check_args(int view, int max_views, int keep, int axis, int radius, int n_gray_v, int n_gray_h)
{
    if (view < 0 || view >= max_views) return -1;
    if (!keep) return -4;
    if (axis != 0 && axis != 1) return -1;
    if (radius < 1 || radius > SL3D_PERIOD_MAX_RADIUS) return -1;
    if ((axis == 0 ? n_gray_v : n_gray_h) == 0) return -5;
    return 0;
}
