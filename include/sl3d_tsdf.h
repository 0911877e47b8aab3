/* sl3d_tsdf.h -- a turntable scan fused into one surface: a TSDF volume on the device (libsl3d 0.26.0 and later): five calls on a context
 * of include/sl3d.h.  Plain C, like sl3d_align.h, which it includes; the functions are exported by the same library. */
#ifndef SL3D_TSDF_H
#define SL3D_TSDF_H

#include "sl3d_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VOLUMETRIC FUSION of the views of a turntable scan.  Every view votes, with a truncated signed distance along the camera's depth, into a
 * regular voxel volume; the surface is the zero level of the averaged votes.  Where views overlap their layers are averaged, what one view
 * misses another fills, and -- unlike the centroids of sl3d_voxel_grid -- the result is oriented: points with normals.  The volume is
 * two planes on the device, sum int32[n] and weight uint32[n]; nothing leaves the device unless the caller asks for it.
 *
 * THE RULE OF THE VOLUME AND ONE INTEGRATION.  All arithmetic is IEEE double, no contraction, in the order of the parentheses.
 *
 * The volume.  L = (double)voxel, T = (double)trunc.  Voxel (i, j, k) of dims (nx, ny, nz) has the linear index v = (k * ny + j) * nx + i;
 * its centre is X_a = ((double)i_a + 0.5) * L + (double)origin[a], a = 0, 1, 2.
 *
 * The turntable.  est = (c, s, tx, tz) is sl3d_turntable.est: cosine and sine of the step, the axis point.  The rotation of turntable
 * index m comes from the recurrence c_0 = 1, s_0 = 0; c_{m+1} = c_m * c - s_m * s; s_{m+1} = s_m * c + c_m * s, run on the host from index
 * 0 up to the index needed: no libm call is involved.  View slot first_view + j of a call is the view with turntable index first_step + j.
 *
 * One sample.  For every voxel and every view of the call, in view order:
 * 1. The centre goes into the view's own frame by the inverse turn, the step of sl3d_align.h with (c_m, -s_m, tx, tz):
 *      x = X.x - tx, z = X.z - tz
 *      P.x = (c_m * x - (-s_m) * z) + tx
 *      P.y = X.y
 *      P.z = ((-s_m) * x + c_m * z) + tz
 * 2. P goes into the camera exactly as step 2 of sl3d_align.h takes p^ there, with the 26 doubles of sl3d_get_align_camera:
 *      xc[i] = ((Rc[3i] * P.x + Rc[3i+1] * P.y) + Rc[3i+2] * P.z) + tc[i];   xc.z <= 0 or not finite: no sample
 *      xn, yn, r2, rad, xd, yd, w as there;  u = ((Kc[0] * xd + Kc[1] * yd) + Kc[2]) / w,  v = ((Kc[3] * xd + Kc[4] * yd) + Kc[5]) / w
 *    u and v stay unrounded doubles.
 * 3. fu = floor(u) - col0, fv = floor(v) - row0, tested as doubles, before any conversion to an integer: unless 0 <= fu, fu + 1 < width,
 *    0 <= fv and fv + 1 < height there is no sample (a NaN fails).  a = u - floor(u), b = v - floor(v).
 * 4. The four pixels (fu + dx, fv + dy), dx, dy in {0, 1}, of the view's window: each needs valid == 1 and three finite coordinates q,
 *    otherwise there is no sample.  The depth of each is z_dxdy = ((Rc[6] * q.x + Rc[7] * q.y) + Rc[8] * q.z) + tc[2], q converted to double.
 * 5. Unless max z - min z <= T there is no sample: the depth-discontinuity guard.
 * 6. zq = ((z00 * (1 - a) + z10 * a) * (1 - b)) + ((z01 * (1 - a) + z11 * a) * b)
 * 7. sdf = zq - xc.z.  Unless sdf >= -T there is no sample: the voxel is hidden behind the surface.  d = sdf / T, and a d > 1 becomes 1.
 *    q = (int32)rint(d * 32767.0), ties to even.
 * 8. sum[v] += q; weight[v] += 1.
 *
 * Both words are exact integers, so neither the order of the views nor the number of calls can matter; a scan with more views than the
 * context has slots is fused in batches into the same volume.  A call that would take the number of views integrated since the last reset
 * past 65535 is refused, so sum stays inside an int32.  counts[0] = the samples this call took, counts[1] = the voxels with weight > 0
 * after it; counts == NULL leaves the call asynchronous.
 *
 * THE RULE OF EXTRACTION.
 * A voxel is known iff weight >= min_weight (min_weight >= 1); its value is f(v) = (double)sum / (double)weight.
 * Take every known voxel v0 in ascending v, and every axis a = 0, 1, 2 whose neighbour v1 = v0 + e_a is inside the volume and known.  The
 * edge carries a crossing iff (f0 < 0) != (f1 < 0); t = f0 / (f0 - f1).
 * Position: the coordinate along axis a is (float)(X_a(v0) + t * L), the other two are the floats of v0's centre.
 * Normal: the gradient component g_b(v) along axis b uses v's known neighbours inside the volume -- both: (f(v+) - f(v-)) * 0.5; only the
 * + neighbour: f(v+) - f(v); only the - neighbour: f(v) - f(v-); none: 0.0.  n_b = (g_b(v0) * (1 - t)) + (g_b(v1) * t),
 * len = sqrt((n0 * n0 + n1 * n1) + n2 * n2); the normal is (float)(n_b / len) if len > 0 and finite, otherwise three NaNs.  f is positive
 * towards the camera, so the normal points out of the object.
 * Output: three parallel arrays in that order of (v0, a): xyz float[m][3], normals float[m][3], edge int32[m] = 3 * v0 + a -- a caller
 * gathers the weights through edge.  counts = (voxels, known voxels, m).  The result is a pure function of the two planes and
 * min_weight.  The arrays are sized by m, so the call synchronises once; device_out (or NULL) receives their device addresses (NULL
 * for m == 0), which stay valid until the next extraction, the next reset or sl3d_destroy.
 *
 * Refusals are made before anything is allocated or enqueued, and a refused call changes nothing.
 * SL3D_E_INVALID_ARG: null pointers where one is required; voxel, trunc or an origin that is NaN or infinite, voxel or trunc <= 0; a
 * dim < 1, or nx * ny * nz > 2^28 (so that 3 * v + 2 fits an int32); views out of range, n_views < 1; first_step < 0 or first_step +
 * n_views > 65535; an est that is not finite; min_weight < 1; capacity < 0.
 * SL3D_E_STATE: no calibration, or no dense result yet; integrate, extract or sl3d_get_tsdf before a reset; sl3d_get_tsdf_surface before
 * an extract (a reset discards the surface).
 * SL3D_E_UNSUPPORTED: the 65535-view limit would be passed.
 *
 * The calls read points and valid only: they write no view's planes, clouds or meshes, nor the registered cloud, the voxel result or
 * the align records.  The context owns the volume, the surface and the depth planes an integration derives from its views
 * (8 bytes a pixel and view of the largest call), grows them on demand and keeps them; sl3d_destroy frees them.
 *
 * There is no group entry point and no shim call. */
typedef struct { float origin[3]; float voxel; float trunc; int32_t dims[3]; } sl3d_tsdf_volume;
typedef struct { const float *xyz; const float *normals; const int32_t *edge; } sl3d_tsdf_surface;   /* device pointers */

/* defines or redefines the volume and clears it; asynchronous */
int sl3d_tsdf_reset(sl3d_ctx *ctx, const sl3d_tsdf_volume *volume);

int sl3d_tsdf_integrate(sl3d_ctx *ctx, int first_view, int n_views, int first_step, const double est[4],
                        int64_t counts[2] /* or NULL: stays asynchronous */);

int sl3d_tsdf_extract(sl3d_ctx *ctx, int64_t min_weight, sl3d_tsdf_surface *device_out /* or NULL */, int64_t counts[3] /* or NULL */);

/* The planes of the volume, by the size-then-fill protocol of sl3d_get_voxel_grid: at most `capacity` words are written to each output
 * that is not NULL, *n (not NULL) always receives nx * ny * nz.  Synchronises. */
int sl3d_get_tsdf(sl3d_ctx *ctx, int32_t *sum, uint32_t *weight, int64_t capacity, int64_t *n);

/* The surface of the last sl3d_tsdf_extract, by the same protocol: *n always receives m.  Synchronises. */
int sl3d_get_tsdf_surface(sl3d_ctx *ctx, float *xyz, float *normals, int32_t *edge, int64_t capacity, int64_t *n);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_TSDF_H */
