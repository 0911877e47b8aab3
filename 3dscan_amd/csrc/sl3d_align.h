// sl3d_align.h -- the arithmetic of the turntable refinement (sl3d_align_sums, sl3d_align_solve, sl3d_refine_turntable; the rule:
// include/sl3d_align.h): the step of a source point into the frame of the view before it, its projection into the camera, the centre
// pixel of its search window, the squared distance to a candidate, the fixed-point coordinates that are summed, and the closed-form
// solve over the sums.
//
// Shared by k_align_pass (sl3d_align.hip), by the host code (sl3d_capi_align.cpp) and by the CPU check the test suite runs
// (tests/native/align_check.cpp): plain C, no HIP types, each piece spelled once.  Every operation is one IEEE double operation, no
// contraction (the library is built with -ffp-contract=off), in the order the parentheses give:
//
//   p^       = (c * x - s * z) + tx, (double)p.y, (s * x + c * z) + tz with x = (double)p.x - tx, z = (double)p.z - tz       (align_step)
//   xc[i]    = ((Rc[3i] * p^.x + Rc[3i+1] * p^.y) + Rc[3i+2] * p^.z) + tc[i]; no candidate unless xc.z > 0 and finite
//   xn, yn   = xc.x / xc.z, xc.y / xc.z;  r2 = xn * xn + yn * yn;  rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
//   xd       = xn * rad + (2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn));  yd = yn * rad + (p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn)
//   u, v, w  = (K[3i] * xd + K[3i+1] * yd) + K[3i+2];  u / w, v / w                                                         (align_project)
//   cc, rr   = rint(u) - col0, rint(v) - row0 (ties to even): a centre iff both are finite and below 2^30 in magnitude      (align_centre)
//   d2       = (ex * ex + ey * ey) + ez * ez, e = (double)q - p^                                                            (align_d2)
//   quantised coordinate of w about o: e = ((double)w - o) * Q, in range iff |e| < 2^18, its integer (int64)rint(e)         (align_quant)
// A product of two quantised coordinates is below 2^36 in magnitude, a word's term below 2^37: a frame of fewer than 2^25 pixels sums
// inside an int64, and the linear words of the 64 lanes of a wave over 8 rows (below 2^18 * 2^9) inside an int.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sl3d_mesh.h"  // SL3D_MESH_FN

#define ALIGN_WORDS 12             // int64 words per pair (include/sl3d_align.h lists them)
#define ALIGN_MAX_WINDOW 4
#define ALIGN_Q_ONE 262144.0       // 2^18: Q = ALIGN_Q_ONE / range, and the bound of a quantised coordinate
#define ALIGN_PIXEL_LIMIT 1073741824.0  // 2^30
#define ALIGN_MAX_PIXELS 33554432  // 2^25: a window of that many pixels or more is refused

// the camera as the pass uses it: the 26 doubles sl3d_get_align_camera hands out, in its order
struct AlignCam {
    double Rc[9], tc[3], Kc[9], dc[5];
};
// one pass: the estimate, the quantisation centre and scale, the acceptance threshold
struct AlignPass {
    double c, s, tx, tz;
    double ox, oz, Q, thr2;
};

SL3D_MESH_FN double align_Q(float range) { return ALIGN_Q_ONE / (double)range; }
SL3D_MESH_FN double align_thr2(float max_dist) { return (double)max_dist * (double)max_dist; }

// is p a source / a candidate's point: three finite coordinates
SL3D_MESH_FN int align_finite(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// step 1: the source point turned once by the step about the axis.  (tsdf_step, sl3d_tsdf.h, is this text over a double point: routed
// through one form the pass kernels' instructions come out in another order, so a change here goes there too)
SL3D_MESH_FN void align_step(const float *p, const struct AlignPass *a, double *ph)
{
    const double x = (double)p[0] - a->tx, z = (double)p[2] - a->tz;
    ph[0] = (a->c * x - a->s * z) + a->tx;
    ph[1] = (double)p[1];
    ph[2] = (a->s * x + a->c * z) + a->tz;
}

// step 2: ph into the camera: *pu, *pv the pixel it projects to, unrounded, *zc = xc.z.  0: nothing (xc.z <= 0 or not finite)
SL3D_MESH_FN int align_project(const double *ph, const struct AlignCam *m, double *pu, double *pv, double *zc)
{
    double xc[3];
    for (int i = 0; i < 3; i++) xc[i] = ((m->Rc[3 * i] * ph[0] + m->Rc[3 * i + 1] * ph[1]) + m->Rc[3 * i + 2] * ph[2]) + m->tc[i];
    if (!(xc[2] > 0.0) || !isfinite(xc[2])) return 0;
    const double xn = xc[0] / xc[2], yn = xc[1] / xc[2];
    const double k1 = m->dc[0], k2 = m->dc[1], p1 = m->dc[2], p2 = m->dc[3], k3 = m->dc[4];
    const double r2 = xn * xn + yn * yn;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double xd = xn * rad + (2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn));
    const double yd = yn * rad + (p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn);
    const double *K = m->Kc;
    const double w = (K[6] * xd + K[7] * yd) + K[8];
    const double u = ((K[0] * xd + K[1] * yd) + K[2]) / w, v = ((K[3] * xd + K[4] * yd) + K[5]) / w;
    *pu = u, *pv = v, *zc = xc[2];
    return 1;
}

// steps 2 and 3: the centre pixel (window coordinates, as doubles that hold integers) of ph's search window; 0: no candidate
SL3D_MESH_FN int align_centre(const double *ph, const struct AlignCam *m, int col0, int row0, double *cc, double *rr)
{
    double u, v, zc;
    if (!align_project(ph, m, &u, &v, &zc)) return 0;
    *cc = rint(u) - (double)col0;
    *rr = rint(v) - (double)row0;
    return fabs(*cc) < ALIGN_PIXEL_LIMIT && fabs(*rr) < ALIGN_PIXEL_LIMIT;  // false for NaN and the infinities
}

// step 4: the squared distance of candidate q.  +inf or NaN for a q that is not finite (and for a finite one whose distance
// overflows): never below the running best, which starts at +inf, so the strict comparison alone keeps such a q out
SL3D_MESH_FN double align_d2(const float *q, const double *ph)
{
    const double ex = (double)q[0] - ph[0], ey = (double)q[1] - ph[1], ez = (double)q[2] - ph[2];
    return (ex * ex + ey * ey) + ez * ez;
}

// step 5: the quantised coordinate of w about o into *out; is it in range?  (*out is written only then)
SL3D_MESH_FN int align_quant(float w, double o, double Q, int64_t *out)
{
    const double e = ((double)w - o) * Q;
    if (!(fabs(e) < ALIGN_Q_ONE)) return 0;
    *out = (int64_t)rint(e);
    return 1;
}

// ... and the pair: source p (untransformed), best candidate q at d2.  1: accepted, t[0 .. 4] = ax, az, bx, bz, dy.  |q.y - p.y| <=
// max_dist <= range once d2 is in range, so dy is at most 2^18 in magnitude
SL3D_MESH_FN int align_accept(const float *p, const float *q, double d2, const struct AlignPass *a, int64_t *t)
{
    if (!(d2 <= a->thr2)) return 0;
    if (!(align_quant(p[0], a->ox, a->Q, &t[0]) & align_quant(p[2], a->oz, a->Q, &t[1]) & align_quant(q[0], a->ox, a->Q, &t[2]) &
          align_quant(q[2], a->oz, a->Q, &t[3])))
        return 0;
    t[4] = (int64_t)rint(((double)q[1] - (double)p[1]) * a->Q);
    return 1;
}

// The solve over the words of n_pairs pairs (host only).  The pairs' words are added in 128 bits; the centred moments are formed as
// exact integers N * S5 - (S1 * S3 + S2 * S4) ... and rounded to double once, then divided by N -- the C, X, Saa, Sbb of the rule with
// one rounding instead of three.  est_in / est_out: c, s, tx, tz; stats: N, rms_xz, rms_y, degenerate (1.0 / 0.0; the two rms are NaN
// then and est_out = est_in).  (Wrap-around arithmetic: words no pass can produce give nonsense, not undefined behaviour.)
static inline void align_solve(const int64_t *sums, int n_pairs, double Q, double ox, double oz, const double *est_in, double *est_out, double *stats)
{
    typedef unsigned __int128 u128;
    typedef __int128 i128;
    u128 S[ALIGN_WORDS];
    for (int k = 0; k < ALIGN_WORDS; k++) S[k] = 0;
    for (int j = 0; j < n_pairs; j++)
        for (int k = 0; k < ALIGN_WORDS; k++) S[k] += (u128)(i128)sums[(size_t)j * ALIGN_WORDS + k];
    const u128 Nn = S[0];
    const double N = (double)(i128)Nn;
    for (int k = 0; k < 4; k++) est_out[k] = est_in[k];
    stats[0] = N, stats[1] = stats[2] = (double)NAN, stats[3] = 1.0;
    if ((i128)Nn < 2) return;
    const double C = (double)(i128)(Nn * S[5] - (S[1] * S[3] + S[2] * S[4])) / N;
    const double X = (double)(i128)(Nn * S[6] - (S[1] * S[4] - S[2] * S[3])) / N;
    if (X == 0.0 && C == 0.0) return;
    const double th = atan2(X, C), c = cos(th), s = sin(th);
    if (c == 1.0) return;
    const double ax = (double)(i128)S[1] / N, az = (double)(i128)S[2] / N, bx = (double)(i128)S[3] / N, bz = (double)(i128)S[4] / N;
    const double dx = bx - (c * ax - s * az), dz = bz - (s * ax + c * az);
    const double m = 1.0 - c, det = m * m + s * s;
    const double tx = (m * dx - s * dz) / det, tz = (s * dx + m * dz) / det;
    est_out[0] = c, est_out[1] = s, est_out[2] = ox + tx / Q, est_out[3] = oz + tz / Q;
    const double Saa = (double)(i128)(Nn * S[7] - (S[1] * S[1] + S[2] * S[2])) / N;
    const double Sbb = (double)(i128)(Nn * S[8] - (S[3] * S[3] + S[4] * S[4])) / N;
    double E = (Saa + Sbb) - 2.0 * (c * C + s * X);
    if (!(E > 0.0)) E = 0.0;
    stats[1] = sqrt(E / N) / Q;
    stats[2] = sqrt((double)(i128)(Nn * S[10] - S[9] * S[9]) / (N * N)) / Q;
    stats[3] = 0.0;
}
