/* sl3d_filter.h -- outlier rejection of the dense scan on the device (libsl3d 0.22.0 and later): two calls on a context of include/sl3d.h.
 * Plain C, like sl3d.h, which it includes; the functions are exported by the same library. */
#ifndef SL3D_FILTER_H
#define SL3D_FILTER_H

#include "sl3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RADIUS OUTLIER FILTER of the dense result: a pixel of a scan that has too few 3-D neighbours among the pixels around it is removed
 * from the scan -- isolated speckle (a wrong Gray bit, a period jump that survives the repair) and the flying pixels along depth
 * discontinuities.  What PCL's RadiusOutlierRemoval does on an unorganised cloud with a k-d tree is, on an organised scan, a window
 * stencil over planes that are already resident.  The call edits the points / valid planes of its views in place, so everything that
 * reads a dense result afterwards -- sl3d_get_points, sl3d_compact_views, sl3d_get_cloud_rgb, sl3d_register_views, every mesh call --
 * sees the filtered scan and needs no change.  Two launches (k_outlier_support<radius>, k_outlier_apply); nothing leaves the device.
 *
 * THE RULE.
 * For every view of the call, every window pixel decides from the planes as they were when the call was enqueued.
 * It does not see its neighbours' rejections.
 *
 * 1. A sample is a window pixel whose merged valid byte is 1.
 * 2. The neighbourhood of pixel (r, c) is the pixels (r + dr, c + dc) with |dr| <= radius, |dc| <= radius and (dr, dc) != (0, 0),
 *    clipped to the context's window.  The padding columns of the pitch are not pixels.
 * 3. len2(p, q) is the one of the mesh stage (sl3d.h): (dx*dx + dy*dy) + dz*dz with dx = (double)p.x - (double)q.x, in IEEE double, no
 *    contraction.  thr2 = (double)max_dist * (double)max_dist.  q is within range of p iff len2(p, q) <= thr2.  A NaN len2 is not within
 *    range.
 * 4. support(p) is the number of samples q in p's neighbourhood with len2(p, q) <= thr2.  It is at most 80.
 * 5. The support plane gets support(p) at every sample and 0xFF at every other window pixel.
 * 6. If min_neighbours > 0, a sample with support < min_neighbours is rejected:
 *    - its merged valid byte becomes 0;
 *    - its point becomes the NaN every dense kernel writes (__builtin_nanf(""), 0x7FC00000 in all three floats);
 *    - its intersection_points entry becomes 0 on a SL3D_FLAG_KEEP_STAGES context;
 *    - its residual, c_p_map and per-axis planes stay as they are (as in step 6 of sl3d_triangulate_subpixel).
 * 7. min_neighbours == 0 writes the support plane and changes nothing else.
 * 8. counts[2k] is the number of samples of view first_view + k on entry.  counts[2k + 1] is the number of those that were rejected.
 * 9. counts == NULL leaves the call asynchronous.  Otherwise the counts are downloaded and the call returns with the stream idle.
 *
 * The valid byte, not the point, decides what a sample is: a sample with a NaN or an infinite coordinate has support 0 for every finite
 * max_dist, and nobody counts it.  An invalid pixel never counts, whatever point lies under it.  max_dist = +infinity makes thr2
 * +infinity: every sample of the neighbourhood whose len2 is not NaN counts, a pure 2-D density filter.  The relation is symmetric
 * (len2(p, q) == len2(q, p) bit for bit), the result is the same on every run and does not depend on the batch a view is filtered in.
 *
 * A second call is a second pass over the result of the first.  sl3d_run, sl3d_triangulate and sl3d_triangulate_subpixel over the view
 * write its points and valid planes anew and so restore what the filter removed.  Nothing outside the views of the call is touched, and
 * of those views nothing but what steps 5 and 6 name.
 *
 * Works on every context sl3d_create accepts, timed or SL3D_FLAG_KEEP_STAGES, with any flag.  Like every call that is not a run it comes
 * behind the launch lanes: a run over one of the views that is still in flight finishes first.
 * Views that hold no dense result: like sl3d_compact_views the call has no precondition on the state of a view and returns SL3D_OK.
 * Before any run the planes are as sl3d_create left them -- no pixel is valid, so there is no sample: counts are 0 and the support plane is
 * 0xFF; after sl3d_run_clouds alone, which does not write the dense planes, the call works on what they held before.
 *
 * Refusals are made before anything is allocated or enqueued, and a refused call changes nothing.
 * SL3D_E_INVALID_ARG: a view out of range or n_views < 1; radius outside 1..SL3D_FILTER_MAX_RADIUS; max_dist NaN or <= 0 (+infinity is
 * allowed); min_neighbours outside 0..(2*radius + 1)^2 - 1.
 *
 * There is no group entry point and no shim call: a neighbourhood is clipped to the context's window, so a row stripe would decide
 * differently from the whole frame within `radius` rows of a seam -- the reason sl3d_group_create refuses SL3D_FLAG_REPAIR_PERIODS. */
#define SL3D_FILTER_MAX_RADIUS 4
int sl3d_filter_outliers(sl3d_ctx *ctx, int first_view, int n_views, int radius, float max_dist, int min_neighbours, uint32_t *counts /* 2 * n_views or NULL */);

/* The support plane the last sl3d_filter_outliers over `view` left (step 5), window-sized row-major bytes (out[row * stride + col], stride
 * >= width).  The support planes (max_views x pitch x height bytes) and the count words are allocated on the first filter call, owned by
 * the context and freed by sl3d_destroy.
 * SL3D_E_INVALID_ARG: view out of range, null out, stride < width; SL3D_E_STATE: no filter call has written this view on this context.
 * Synchronises. */
int sl3d_get_support(sl3d_ctx *ctx, int view, uint8_t *out, size_t stride);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_FILTER_H */
