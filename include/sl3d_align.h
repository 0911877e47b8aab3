/* sl3d_align.h -- the turntable's axis and step estimated from the scan itself (libsl3d 0.24.0 and later): four calls, three of them on a
 * context of include/sl3d.h.  Plain C, like sl3d.h, which it includes; the functions are exported by the same library. */
#ifndef SL3D_ALIGN_H
#define SL3D_ALIGN_H

#include "sl3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TURNTABLE REFINEMENT.  sl3d_register_views and sl3d_register_clouds take the axis point (tx, ty, tz) and the step angle rot_step from the
 * caller; a rig knows its step roughly and its axis hardly at all, and an axis off by a millimetre leaves double layers in the registered
 * cloud.  Consecutive views overlap, their dense planes (points, valid) are organised by camera pixel and the context knows the camera: the
 * four numbers are an ICP problem with projective data association -- no spatial index, one gather launch per iteration (k_align_pass), a
 * closed-form solve on the host for the three parameters the model has: a rotation about Y through (tx, ., tz).
 *
 * THE RULE of one correspondence pass.
 * Inputs: the views [first_view, first_view + n_views), n_views >= 2, their dense planes as they stand; an estimate est = (c, s, tx, tz) in
 * double, c and s the cosine and sine of the step; a quantisation centre (ox, oz) in double; range (float, > 0), max_dist (float, 0 <
 * max_dist <= range) and window (0 .. SL3D_ALIGN_MAX_WINDOW).  All arithmetic is IEEE double, no contraction, in the order of the parentheses.
 * R is the rotation sl3d_register_views applies: X = c x - s z, Z = s x + c z, Y = y.  A point of view k + 1, turned once by the step about
 * the axis, lies in the frame of view k: pair j is (source view first_view + j + 1, target view first_view + j).
 *
 * For every source: a pixel of the source view with valid == 1 and three finite coordinates p --
 * 1. p^ = R (p - t) + t with t = (tx, 0, tz):
 *      x = (double)p.x - tx, z = (double)p.z - tz;  p^.x = (c * x - s * z) + tx,  p^.y = (double)p.y,  p^.z = (s * x + c * z) + tz
 * 2. into the camera: xc[i] = ((Rc[3i] * p^.x + Rc[3i+1] * p^.y) + Rc[3i+2] * p^.z) + tc[i], with [Rc|tc], Kc and dc = (k1, k2, p1, p2,
 *    k3) the doubles of sl3d_get_align_camera.  xc.z <= 0 or not finite: a source with no candidate.  xn = xc.x / xc.z, yn = xc.y / xc.z,
 *      r2 = xn * xn + yn * yn
 *      rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *      xd = xn * rad + (2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn))
 *      yd = yn * rad + (p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn)
 *      u = ((Kc[0] * xd + Kc[1] * yd) + Kc[2]) / w,  v = ((Kc[3] * xd + Kc[4] * yd) + Kc[5]) / w,  w = (Kc[6] * xd + Kc[7] * yd) + Kc[8]
 *    Zero coefficients are multiplied like any others.
 * 3. the centre pixel cc = rint(u) - col0, rr = rint(v) - row0, ties to even; both are tested as doubles -- finite, magnitude < 2^30 --
 *    before any conversion to an integer, else the source has no candidate.  Candidates are the target pixels (cc + dx, rr + dy), |dx|,
 *    |dy| <= window, inside [0, width) x [0, height), with valid == 1 and three finite coordinates q: the window is clipped to the frame
 *    window of the context, never to the pitch of its planes.
 * 4. d2 = (ex * ex + ey * ey) + ez * ez with e = (double)q - p^.  The best candidate has the smallest d2: the best starts at +infinity,
 *    candidates are visited in row-major order and one replaces the best only if its d2 is strictly smaller -- ties go to the first, an
 *    overflowed d2 is never chosen.
 * 5. the pair is accepted iff a best candidate exists, d2 <= (double)max_dist * (double)max_dist, and the four quantised coordinates are
 *    in range: Q = 262144.0 / (double)range; for w in {p.x, p.z, q.x, q.z} of the UNTRANSFORMED source p and the target q, about o = ox
 *    for an x and oz for a z: e = ((double)w - o) * Q, in range iff |e| < 262144.0, its integer (int64)rint(e).  They are ax, az (source)
 *    and bx, bz (target); dy = (int64)rint(((double)q.y - (double)p.y) * Q).
 * 6. per pair twelve int64 words: 0 = accepted pairs n; 1 - 4 = sum ax, sum az, sum bx, sum bz; 5 = sum (ax * bx + az * bz); 6 = sum (ax *
 *    bz - az * bx); 7 = sum (ax * ax + az * az); 8 = sum (bx * bx + bz * bz); 9 = sum dy; 10 = sum dy * dy; 11 = sources.
 * Every sum is an exact integer, so the order of arrival cannot matter: a term is below 2^37 in magnitude, and a frame window of width *
 * height >= 2^25 pixels is refused (SL3D_E_UNSUPPORTED), so a word stays below 2^62.  Every atomic of the kernel is an integer atomic; there
 * are no float atomics.
 *
 * THE SOLVE (host, double).  The pairs' words are added in 128 bits: S0 .. S11, N = S0.  The centred moments
 *   C = S5 - (S1 * S3 + S2 * S4) / N,  X = S6 - (S1 * S4 - S2 * S3) / N,  Saa = S7 - (S1 * S1 + S2 * S2) / N,  Sbb = S8 - (S3 * S3 + S4 * S4) / N
 * are formed as the exact integers N * S5 - (S1 * S3 + S2 * S4) ..., rounded to double once and divided by (double)N.
 *   theta = atan2(X, C), c' = cos(theta), s' = sin(theta)
 *   a~ = (S1 / N, S2 / N), b~ = (S3 / N, S4 / N);  d = b~ - R' a~:  dx = b~x - (c' * a~x - s' * a~z), dz = b~z - (s' * a~x + c' * a~z)
 *   the axis point solves (I - R') t' = d:  m = 1 - c', det = m * m + s' * s';  t'x = (m * dx - s' * dz) / det, t'z = (s' * dx + m * dz) / det
 *   tx' = ox + t'x / Q,  tz' = oz + t'z / Q
 *   rms_xz = sqrt(max((Saa + Sbb) - 2 * (c' * C + s' * X), 0) / N) / Q;  rms_y = sqrt((N * S10 - S9 * S9) / (N * N)) / Q, the spread of dy
 *   about its mean (the numerator an exact integer)
 * The solve is degenerate iff N < 2, or X == 0 and C == 0, or c' == 1.0 -- exact conditions; it then returns the estimate it was given,
 * both rms are NaN, and it says so.  ty is unobservable under this model and is passed through.
 *
 * Refusals are made before anything is allocated or enqueued, and a refused call changes nothing.  SL3D_E_INVALID_ARG: n_views < 2, views
 * out of range, range or max_dist NaN, infinite or <= 0, max_dist > range, window outside 0 .. 4, iterations outside 1 .. 64, an estimate
 * that is not finite, null outputs where one is required.  SL3D_E_STATE: no calibration, or no dense result yet (no sl3d_run,
 * sl3d_process_views, sl3d_triangulate or sl3d_triangulate_subpixel has run on the context).  SL3D_E_UNSUPPORTED: width * height >= 2^25.
 * The calls read points and valid only: they write no view's planes, clouds or meshes, nor the registered cloud, nor the voxel result.
 * The context owns the pairs' records and a pinned block the words are downloaded into; sl3d_destroy frees them.
 *
 * There is no group entry point and no shim call. */
#define SL3D_ALIGN_WORDS      12
#define SL3D_ALIGN_MAX_WINDOW 4
#define SL3D_ALIGN_MAX_ITERATIONS 64

/* what sl3d_refine_turntable leaves: tx, ty, tz, rot_step as sl3d_register_views takes them (rot_step in degrees under Pi = 22/7: atan2(s,
 * c) * 180 * 7 / 22, the inverse of the conversion the registration makes; ty as given); the estimate in double; accepted pairs, sources
 * and both rms of the last pass; degenerate: 1 if the last solve was degenerate */
typedef struct { float tx, ty, tz, rot_step; double est[4]; int64_t n, sources; double rms_xz, rms_y; int32_t degenerate, reserved; } sl3d_turntable;
/* one iteration: the estimate (c, s, tx, tz) its pass used, the pass's accepted pairs and sources, the rms of its solve */
typedef struct { double est[4]; int64_t n, sources; double rms_xz, rms_y; } sl3d_align_iteration;

/* One pass, one launch (behind the memset of the pairs' records) on the context's stream: sums[n_views - 1][12].  sums == NULL leaves the
 * call asynchronous; otherwise the words are downloaded and the call returns with the stream idle. */
int sl3d_align_sums(sl3d_ctx *ctx, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist,
                    int window, int64_t *sums);

/* The solve over the words of n_pairs pairs.  Host only: no context, no GPU.  est_in / est_out: (c, s, tx, tz); stats: N, rms_xz, rms_y,
 * degenerate (1.0 or 0.0).  SL3D_E_INVALID_ARG: a null pointer, n_pairs < 1, range NaN, infinite or <= 0, ox, oz or est_in not finite. */
int sl3d_align_solve(const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4],
                     double stats[4]);

/* Pass, then solve, `iterations` times (1 .. 64) from (tx, tz, rot_step): the first estimate is c = cos(a), s = sin(a), a = rot_step * 22.0 /
 * 7.0 / 180.0 as the registration converts it, and ((double)tx, (double)tz); the quantisation centre is ((double)tx, (double)tz) as given,
 * fixed for the whole call.  Iteration i runs a pass with its estimate, solves, stores log[i] (log: NULL, or `iterations` entries) and takes
 * the solve's estimate; the loop ends behind a degenerate solve (the estimate stays) and behind an iteration whose pass returned the same
 * 12 * (n_views - 1) words as the pass before it.  *n_done (not NULL): the iterations made.  out: not NULL.  Synchronises. */
int sl3d_refine_turntable(sl3d_ctx *ctx, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range, float max_dist,
                          int window, int iterations, sl3d_turntable *out, sl3d_align_iteration *log, int *n_done);

/* The camera exactly as the pass uses it: cam[0 .. 8] = Rc (row-major, from rc by Rodrigues' formula at sl3d_set_calibration), cam[9 .. 11] =
 * tc, cam[12 .. 20] = Kc, cam[21 .. 25] = dc, so that a restatement reproduces the pass bit for bit.  SL3D_E_STATE before sl3d_set_calibration. */
int sl3d_get_align_camera(sl3d_ctx *ctx, double cam[26]);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_ALIGN_H */
