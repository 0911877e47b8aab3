/* sl3d_align_plane.h -- the turntable's axis and step estimated from the scan with the point-to-plane error metric (libsl3d 0.25.0 and
 * later): five calls, four of them on a context of include/sl3d.h.  Plain C; it includes sl3d_align.h, whose structures, camera and first
 * four steps it takes over; the functions are exported by the same library. */
#ifndef SL3D_ALIGN_PLANE_H
#define SL3D_ALIGN_PLANE_H

#include "sl3d_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* POINT-TO-PLANE REFINEMENT.  sl3d_refine_turntable (sl3d_align.h) minimises the distance between a source point and its correspondence;
 * projective correspondences are never the true partner, the error along the surface does not average out, and the estimate settles half
 * a degree off.  Here the residual is measured along the target's surface normal, so a correspondence may slide along the surface without
 * cost.  The dense planes are organised by pixel: a target normal is a 5-point stencil (k_align_normals), the correspondence search is that
 * of sl3d_align.h (k_align_plane_pass), the solve minimises a quadratic form over five features on the host.
 *
 * THE RULE of a view's normals.  Inputs: the view's dense planes (points, valid) as they stand and normal_edge (float, > 0).  All
 * arithmetic is IEEE double, no contraction, in the order of the parentheses.  The pixel (r, c) of the frame window with point q has a
 * normal iff
 * 1. valid == 1 and three finite coordinates at the pixel and at its four neighbours (r, c - 1), (r, c + 1), (r - 1, c), (r + 1, c), all
 *    five inside the frame window [0, width) x [0, height) of the context, never the pitch of its planes: a pixel of the window's border
 *    has no normal;
 * 2. each neighbour m within normal_edge of q: (ex * ex + ey * ey) + ez * ez <= (double)normal_edge * (double)normal_edge with
 *    e = (double)m - (double)q;
 * 3. a = right - left, b = down - up, each component a difference of two floats promoted to double;
 *      n.x = (a.y * b.z) - (a.z * b.y),  n.y = (a.z * b.x) - (a.x * b.z),  n.z = (a.x * b.y) - (a.y * b.x)
 *      len2 = (n.x * n.x + n.y * n.y) + n.z * n.z,  len = sqrt(len2)
 *    len finite and > 0: the normal is ((float)(n.x / len), (float)(n.y / len), (float)(n.z / len)).
 * Otherwise all three floats are NaN: no normal.  The orientation is whatever the cross product gives; the residual is squared.
 *
 * THE RULE of one point-to-plane pass.  Inputs as sl3d_align_sums: views, est = (c, s, tx, tz), the quantisation centre (ox, oz), range,
 * max_dist, window; in addition the target views' normals.  Steps 1 - 4 of the rule in sl3d_align.h are taken over verbatim -- the source
 * turned by the estimate, its projection, the centre pixel, the nearest candidate in row-major order with a strictly smaller d2 -- and the
 * best candidate's pixel is remembered with its point q.
 * 5. the pair is accepted iff a best candidate exists, d2 <= (double)max_dist * (double)max_dist, the best candidate's pixel has a normal n,
 *    and the five features are in range.  A source whose best candidate within max_dist has no normal is lost: it is counted in word 17
 *    and not re-matched with a farther candidate.
 * 6. the features, from the UNTRANSFORMED source p, with p'x = (double)p.x - ox, p'z = (double)p.z - oz, q'x = (double)q.x - ox,
 *    q'z = (double)q.z - oz and n promoted to double:
 *      A = n.x * p'x + n.z * p'z
 *      B = n.z * p'x - n.x * p'z
 *      D = n.y * ((double)p.y - (double)q.y) - (n.x * q'x + n.z * q'z)
 *    With u = (1 - c) t'x + s t'z and w = (1 - c) t'z - s t'x, t' the axis point about the centre, the residual along the normal is
 *    n . (R (p - t) + t - q) = c A + s B + u n.x + w n.z + D.
 * 7. fixed point: Qp = 65536.0 / (double)range for the lengths, Qn = 65536.0 for the normal's components; e = A * Qp, B * Qp, n.x * Qn,
 *    n.z * Qn, D * Qp; a feature is in range iff |e| < 262144.0, its integer (int64)rint(e): f = (fA, fB, fnx, fnz, fD).
 * 8. per pair eighteen int64 words: 0 = accepted pairs n; 1 - 15 = the upper triangle, row-major, of sum f_i * f_j (1 = sum fA * fA, 2 =
 *    sum fA * fB, ... 5 = sum fA * fD, 6 = sum fB * fB, ... 15 = sum fD * fD); 16 = sources; 17 = sources lost to a missing normal.
 * No overflow: a feature is below 2^18 in magnitude, a product below 2^36; a frame window of width * height >= 2^25 pixels is refused
 * (SL3D_E_UNSUPPORTED), so a word stays below 2^61.  (Where every coordinate lies within range of the centre, |A| and |B| are at most
 * sqrt(2) range and |D| <= max_dist + sqrt(2) range < 2.42 range: 2^16 leaves room, the range test is never the limit there.)  Every sum is
 * an exact integer, so the order of arrival cannot matter; every atomic of the kernel is an integer atomic, there are no float atomics.
 * Given the correspondences the words do not depend on the estimate.
 *
 * THE SOLVE (host, double).  The pairs' words are added in 128 bits: S0 .. S17, N = S0; each moment is rounded to double once and the
 * rows and columns of fnx and fnz are scaled by 2^-16 (exact): M, 5 x 5 symmetric, the moments of (A Qp, B Qp, n.x, n.z, D Qp).  The sum of
 * the squared residuals is g M g / Qp^2 with g = (c, s, u, w, 1), u and w in units of 1 / Qp.  Start from est_in: theta = atan2(s, c),
 * t' = ((tx - ox) * Qp, (tz - oz) * Qp), u = (1 - c) * t'x + s * t'z, w = (1 - c) * t'z - s * t'x with c = cos(theta), s = sin(theta).
 * SL3D_ALIGN_PLANE_STEPS Gauss-Newton steps on (u, w, theta); in each, with Mg[i] = (((M[i][0] * c + M[i][1] * s) + M[i][2] * u) +
 * M[i][3] * w) + M[i][4] and the Jacobian rows over g (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (-s, c, 0, 0, 0):
 *   gradient  bu = Mg[2], bw = Mg[3], bt = -s * Mg[0] + c * Mg[1]
 *   Huu = M[2][2], Huw = M[2][3], Hww = M[3][3], Hut = M[2][0] * -s + M[2][1] * c, Hwt = M[3][0] * -s + M[3][1] * c,
 *   Htt = -s * (M[0][0] * -s + M[0][1] * c) + c * (M[1][0] * -s + M[1][1] * c)
 *   Cholesky as L D L^T, eliminated in the order u, w, theta:  d0 = Huu;  l10 = Huw / d0, l20 = Hut / d0;  d1 = Hww - l10 * Huw;
 *   e21 = Hwt - l10 * Hut, l21 = e21 / d1;  d2 = (Htt - l20 * Hut) - l21 * e21
 *   y0 = -bu, y1 = -bw - l10 * y0, y2 = (-bt - l20 * y0) - l21 * y1;  z2 = y2 / d2, z1 = y1 / d1 - l21 * z2, z0 = (y0 / d0 - l10 * z1) - l20 * z2
 *   u += z0, w += z1, theta += z2
 * then c' = cos(theta), s' = sin(theta), m = 1 - c', det = m * m + s' * s', t'x = (m * u - s' * w) / det, t'z = (s' * u + m * w) / det,
 * tx' = ox + t'x / Qp, tz' = oz + t'z / Qp, and rms_plane = sqrt(max(g M g, 0) / N) / Qp at the final g.
 * The solve is degenerate iff N < 3, or a pivot d0, d1, d2 is not greater than 2^-40 times its diagonal entry Huu, Hww, Htt (a single
 * plane, a surface of revolution about the axis), or any quantity is not finite, or c' == 1.0 -- exact conditions; it then returns the
 * estimate it was given, the rms is NaN, and it says so.  ty is unobservable under this model and is passed through.
 *
 * THE LOOP.  sl3d_refine_turntable_plane computes the normals of its target views once, before the first pass, and then runs one pass
 * launch and one solve per iteration.  The first estimate, the conversion of rot_step under Pi = 22/7, the fixed quantisation centre and
 * both stopping rules -- a degenerate solve, a pass that repeats the words of the pass before -- are those of sl3d_refine_turntable.  It
 * fills the two structures of sl3d_align.h: rms_xz carries rms_plane, rms_y is NaN.
 *
 * Refusals are those of sl3d_align.h, made before anything is allocated or enqueued, and a refused call changes nothing; in addition
 * SL3D_E_INVALID_ARG for a normal_edge that is NaN, infinite or <= 0.  sl3d_get_align_normals: SL3D_E_STATE if that view's normals were
 * never computed.  The calls read points and valid only.  The context owns the normal planes -- one float3 per pixel, laid out like
 * points, allocated on first use for the span of views asked for so far (a call that widens the span allocates anew and the earlier
 * normals are gone) -- the pairs' records and a pinned block; sl3d_destroy frees them.  The normals are a snapshot: a later sl3d_run does
 * not refresh them, sl3d_align_plane_sums and sl3d_refine_turntable_plane always recompute their own.
 *
 * There is no group entry point and no shim call. */
#define SL3D_ALIGN_PLANE_WORDS 18
#define SL3D_ALIGN_PLANE_STEPS 8

/* The normals of views [first_view, first_view + n_views), n_views >= 1: one launch, asynchronous on the context's stream. */
int sl3d_align_normals(sl3d_ctx *ctx, int first_view, int n_views, float normal_edge);

/* One view's normal plane: height rows of width * 3 floats, row_stride_bytes apart.  Synchronises. */
int sl3d_get_align_normals(sl3d_ctx *ctx, int view, float *dst, size_t row_stride_bytes);

/* The normals of the call's target views, then one pass: sums[n_views - 1][18].  It always recomputes the normals.  sums == NULL leaves
 * the call asynchronous; otherwise the words are downloaded and the call returns with the stream idle. */
int sl3d_align_plane_sums(sl3d_ctx *ctx, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist,
                          float normal_edge, int window, int64_t *sums);

/* The solve over the words of n_pairs pairs.  Host only: no context, no GPU.  est_in / est_out: (c, s, tx, tz); stats: N, rms_plane, NaN,
 * degenerate (1.0 or 0.0).  SL3D_E_INVALID_ARG: a null pointer, n_pairs < 1, range NaN, infinite or <= 0, ox, oz or est_in not finite. */
int sl3d_align_plane_solve(const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4],
                           double stats[4]);

/* Normals, then pass and solve `iterations` times (1 .. 64), as sl3d_refine_turntable.  log: NULL, or `iterations` entries; *n_done (not
 * NULL): the iterations made; out: not NULL.  Synchronises. */
int sl3d_refine_turntable_plane(sl3d_ctx *ctx, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range,
                                float max_dist, float normal_edge, int window, int iterations, sl3d_turntable *out, sl3d_align_iteration *log,
                                int *n_done);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_ALIGN_PLANE_H */
