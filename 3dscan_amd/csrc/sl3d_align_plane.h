// sl3d_align_plane.h -- the arithmetic of the point-to-plane turntable refinement (sl3d_align_normals, sl3d_align_plane_sums,
// sl3d_align_plane_solve, sl3d_refine_turntable_plane; the rule: include/sl3d_align_plane.h): the normal of a pixel from its four
// neighbours, the five features of an accepted pair and their fixed-point form, and the Gauss-Newton solve over the moments.  The step
// into the target's frame, the centre pixel and the squared distance are those of sl3d_align.h (align_step, align_centre, align_d2).
//
// Shared by k_align_normals and k_align_plane_pass (sl3d_align_plane.hip), by the host code (sl3d_capi_align_plane.cpp) and by the CPU
// check the test suite runs (tests/native/align_plane_check.cpp): plain C, no HIP types, each piece spelled once.  Every operation is one
// IEEE double operation, no contraction (-ffp-contract=off), in the order the parentheses give:
//
//   normal at q from l, r (the row's neighbours) and u, d (the column's): all five finite, d2(neighbour, q) <= edge2 (align_d2);
//            a = (double)r - (double)l, b = (double)d - (double)u;  n = a x b, each component (x * y) - (z * w);
//            len2 = (nx * nx + ny * ny) + nz * nz, len = sqrt(len2); finite and > 0: (float)(n / len), else three NaNs      (align_normal)
//   features of source p (untransformed), target q, normal n about o: p' = (double)p - o, q' = (double)q - o
//            A = nx * p'x + nz * p'z;  B = nz * p'x - nx * p'z;  D = ny * ((double)p.y - (double)q.y) - (nx * q'x + nz * q'z)
//   fixed point: e = A * Qp, B * Qp, nx * Qn, nz * Qn, D * Qp with Qp = 2^16 / range, Qn = 2^16; in range iff |e| < 2^18,
//            its integer (int64)rint(e)                                                                                     (align_plane_features)
//   the pair: d2 <= thr2, then a normal at the best candidate's pixel (else the source is lost), then five features in range (align_plane_accept)
// A product of two features is below 2^36 in magnitude: a frame of fewer than 2^25 pixels sums inside an int64 (below 2^61).
#pragma once
#include "sl3d_align.h"

#define ALIGN_PLANE_WORDS 18            // int64 words per pair (include/sl3d_align_plane.h lists them)
#define ALIGN_PLANE_FEATURES 5
#define ALIGN_PLANE_Q_ONE 65536.0       // 2^16: Qp = ALIGN_PLANE_Q_ONE / range, Qn = ALIGN_PLANE_Q_ONE
#define ALIGN_PLANE_LIMIT 262144.0      // 2^18: the bound of a quantised feature
#define ALIGN_PLANE_STEPS 8             // Gauss-Newton steps of the solve
#define ALIGN_PLANE_PIVOT 9.094947017729282379150390625e-13  // 2^-40: a pivot at or below this share of its diagonal entry is degenerate

SL3D_MESH_FN double align_plane_Q(float range) { return ALIGN_PLANE_Q_ONE / (double)range; }

// the normal at q from its neighbours l, r, u, d (the caller has seen five valid bytes of 1 inside the frame window); edge2: align_thr2 of
// normal_edge.  n: the normal, or three NaNs; returns whether there is one
SL3D_MESH_FN int align_normal(const float *q, const float *l, const float *r, const float *u, const float *d, double edge2, float *n)
{
    n[0] = n[1] = n[2] = __builtin_nanf("");
    if (!(align_finite(q) && align_finite(l) && align_finite(r) && align_finite(u) && align_finite(d))) return 0;
    const double c[3] = {(double)q[0], (double)q[1], (double)q[2]};
    if (!(align_d2(l, c) <= edge2 && align_d2(r, c) <= edge2 && align_d2(u, c) <= edge2 && align_d2(d, c) <= edge2)) return 0;
    const double ax = (double)r[0] - (double)l[0], ay = (double)r[1] - (double)l[1], az = (double)r[2] - (double)l[2];
    const double bx = (double)d[0] - (double)u[0], by = (double)d[1] - (double)u[1], bz = (double)d[2] - (double)u[2];
    const double nx = (ay * bz) - (az * by), ny = (az * bx) - (ax * bz), nz = (ax * by) - (ay * bx);
    const double len2 = (nx * nx + ny * ny) + nz * nz, len = sqrt(len2);
    if (!(len > 0.0) || !isfinite(len)) return 0;
    n[0] = (float)(nx / len), n[1] = (float)(ny / len), n[2] = (float)(nz / len);
    return 1;
}

// does a pixel of the normal plane hold a normal?  (all three floats are NaN, or none is)
SL3D_MESH_FN int align_has_normal(const float *n) { return n[0] == n[0]; }

// a feature in fixed point: e into *out if |e| < 2^18 (*out is written only then)
SL3D_MESH_FN int align_plane_quant(double e, int64_t *out)
{
    if (!(fabs(e) < ALIGN_PLANE_LIMIT)) return 0;
    *out = (int64_t)rint(e);
    return 1;
}

// the five features of the pair (source p untransformed, best candidate q with normal n) about (a->ox, a->oz), a->Q = Qp.  1: all in
// range, f[0 .. 4] = A, B, nx, nz, D
SL3D_MESH_FN int align_plane_features(const float *p, const float *q, const float *n, const struct AlignPass *a, int64_t *f)
{
    const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
    const double px = (double)p[0] - a->ox, pz = (double)p[2] - a->oz, qx = (double)q[0] - a->ox, qz = (double)q[2] - a->oz;
    const double A = nx * px + nz * pz;
    const double B = nz * px - nx * pz;
    const double D = ny * ((double)p[1] - (double)q[1]) - (nx * qx + nz * qz);
    return align_plane_quant(A * a->Q, &f[0]) & align_plane_quant(B * a->Q, &f[1]) & align_plane_quant(nx * ALIGN_PLANE_Q_ONE, &f[2]) &
           align_plane_quant(nz * ALIGN_PLANE_Q_ONE, &f[3]) & align_plane_quant(D * a->Q, &f[4]);
}

// the verdict on a source whose best candidate q at d2 has the entry n of the normal plane (read only behind the distance test): 0 = no
// pair, 1 = accepted, f[0 .. 4] written, 2 = within max_dist but lost to a missing normal
SL3D_MESH_FN int align_plane_accept(const float *p, const float *q, const float *n, double d2, const struct AlignPass *a, int64_t *f)
{
    if (!(d2 <= a->thr2)) return 0;
    const float nn[3] = {n[0], n[1], n[2]};
    if (!align_has_normal(nn)) return 2;
    return align_plane_features(p, q, nn, a, f);
}

// The solve over the words of n_pairs pairs (host only).  The pairs' words are added in 128 bits, each moment is rounded to double once
// and the rows and columns of nx and nz are scaled back by 2^-16 (exact): M is the moment matrix of (A Qp, B Qp, nx, nz, D Qp).  The sum
// of the squared residuals (in units of 1 / Qp) is g M g with g = (c, s, u, w, 1), u = (1 - c) t'x + s t'z, w = (1 - c) t'z - s t'x, t' the
// axis point about the centre times Qp.  ALIGN_PLANE_STEPS Gauss-Newton steps on (u, w, theta) from est_in; the 3 x 3 system by Cholesky in
// the form L D L^T, eliminated in the order u, w, theta.  est_in / est_out: c, s, tx, tz; stats: N, rms_plane, NaN, degenerate (1.0 / 0.0;
// the rms is NaN then and est_out = est_in).
static inline void align_plane_solve(const int64_t *sums, int n_pairs, double Qp, double ox, double oz, const double *est_in, double *est_out, double *stats)
{
    typedef unsigned __int128 u128;
    typedef __int128 i128;
    u128 S[ALIGN_PLANE_WORDS];
    for (int k = 0; k < ALIGN_PLANE_WORDS; k++) S[k] = 0;
    for (int j = 0; j < n_pairs; j++)
        for (int k = 0; k < ALIGN_PLANE_WORDS; k++) S[k] += (u128)(i128)sums[(size_t)j * ALIGN_PLANE_WORDS + k];
    const double N = (double)(i128)S[0];
    for (int k = 0; k < 4; k++) est_out[k] = est_in[k];
    stats[0] = N, stats[1] = stats[2] = (double)NAN, stats[3] = 1.0;
    if ((i128)S[0] < 3) return;
    double M[5][5];
    for (int i = 0, k = 1; i < 5; i++)
        for (int j = i; j < 5; j++, k++) {
            const int normals = (i == 2 || i == 3) + (j == 2 || j == 3);
            M[i][j] = M[j][i] = (double)(i128)S[k] * (normals == 2 ? 0x1p-32 : normals == 1 ? 0x1p-16 : 1.0);
        }
    double th = atan2(est_in[1], est_in[0]), c = cos(th), s = sin(th);
    const double tpx = (est_in[2] - ox) * Qp, tpz = (est_in[3] - oz) * Qp;
    double u = (1.0 - c) * tpx + s * tpz, w = (1.0 - c) * tpz - s * tpx;
    double g[5], Mg[5];
    for (int it = 0; it <= ALIGN_PLANE_STEPS; it++) {
        c = cos(th), s = sin(th);
        g[0] = c, g[1] = s, g[2] = u, g[3] = w, g[4] = 1.0;
        for (int i = 0; i < 5; i++) Mg[i] = (((M[i][0] * g[0] + M[i][1] * g[1]) + M[i][2] * g[2]) + M[i][3] * g[3]) + M[i][4] * g[4];
        if (it == ALIGN_PLANE_STEPS) break;
        const double j0 = -s, j1 = c;  // d g / d theta = (-s, c, 0, 0, 0)
        const double bu = Mg[2], bw = Mg[3], bt = j0 * Mg[0] + j1 * Mg[1];
        const double Huu = M[2][2], Huw = M[2][3], Hww = M[3][3];
        const double Hut = M[2][0] * j0 + M[2][1] * j1, Hwt = M[3][0] * j0 + M[3][1] * j1;
        const double Htt = j0 * (M[0][0] * j0 + M[0][1] * j1) + j1 * (M[1][0] * j0 + M[1][1] * j1);
        const double d0 = Huu;
        if (!(d0 > ALIGN_PLANE_PIVOT * Huu)) return;
        const double l10 = Huw / d0, l20 = Hut / d0;
        const double d1 = Hww - l10 * Huw;
        if (!(d1 > ALIGN_PLANE_PIVOT * Hww)) return;
        const double e21 = Hwt - l10 * Hut, l21 = e21 / d1;
        const double d2 = (Htt - l20 * Hut) - l21 * e21;
        if (!(d2 > ALIGN_PLANE_PIVOT * Htt)) return;
        const double y0 = -bu, y1 = -bw - l10 * y0, y2 = (-bt - l20 * y0) - l21 * y1;
        const double z2 = y2 / d2, z1 = y1 / d1 - l21 * z2, z0 = (y0 / d0 - l10 * z1) - l20 * z2;
        u += z0, w += z1, th += z2;
        if (!(isfinite(u) && isfinite(w) && isfinite(th))) return;
    }
    if (c == 1.0) return;
    const double m = 1.0 - c, det = m * m + s * s;
    const double tx = (m * u - s * w) / det, tz = (s * u + m * w) / det;
    double E = (((g[0] * Mg[0] + g[1] * Mg[1]) + g[2] * Mg[2]) + g[3] * Mg[3]) + g[4] * Mg[4];
    if (!(E > 0.0)) E = E == E ? 0.0 : E;
    const double ex = ox + tx / Qp, ez = oz + tz / Qp, rms = sqrt(E / N) / Qp;
    if (!(isfinite(ex) && isfinite(ez) && isfinite(rms))) return;
    est_out[0] = c, est_out[1] = s, est_out[2] = ex, est_out[3] = ez;
    stats[1] = rms, stats[3] = 0.0;
}
