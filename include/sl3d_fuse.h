/* sl3d_fuse.h -- exposure fusion on the device (libsl3d 0.21.0 and later): two calls on a context of include/sl3d.h.
 * Plain C, like sl3d.h, which it includes; the functions are exported by the same library. */
#ifndef SL3D_FUSE_H
#define SL3D_FUSE_H

#include "sl3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EXPOSURE FUSION on the device: one pattern set captured at several exposures becomes ONE view that holds, per pixel, the bytes
 * of the brightest exposure that does not clip (Zhang & Yau 2009).  The output is an ordinary view: sl3d_run with any flag, the staged
 * calls, clouds and meshes work on it unchanged.  One HBM-bound launch (k_fuse_exposures); no frame leaves the device.
 *
 * THE RULE.
 * Exposure e = 0 .. E-1 is view first_view + e, with 1 <= E <= 8.
 * Everything is decided per window pixel, in integers.
 *
 * Planes in use.
 * The coded axes are both axes, or the one axis of SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL.
 * Per coded axis the planes in use are:
 * - the F fringe planes,
 * - the N Gray planes,
 * - the N inverse-Gray planes, unless the context has SL3D_FLAG_DIRECT_GRAY.
 * An axis with n_gray == 0 still contributes its fringes.
 * No other plane is read or written by anything in this feature.
 *
 * Clip count.
 * n_e is the number of planes in use whose byte at the pixel is >= saturation.
 * saturation is 1..256, so 256 means nothing ever clips.
 * The largest possible n_e is 72.
 *
 * Score.
 * S_a(e) = t1*t1 + t2*t2, where t1 and t2 are the integers stage 3 hands to atan2 for axis a.
 * - F == 3: t1 = I0 - I2, t2 = 2*I1 - I0 - I2.
 * - F == 4: t1 = I3 - I1, t2 = I0 - I2.
 * S_a(e) <= 325125 < 2^19.
 * Q_e is the minimum of S_a(e) over the coded axes.
 *
 * Choice.
 * Choose the exposure with the smallest n_e.
 * Among those, take the largest Q_e; among those, take the smallest e.
 * This is the same as the argmax of the packed key K_e = ((127 - n_e) << 22) | (Q_e << 3) | (7 - e).
 *
 * Output.
 * - Every plane in use of dst_view gets the byte of the chosen exposure at that pixel.
 * - The exposure map of dst_view gets the byte e | (n_e > 0 ? 0x80 : 0).
 * - counts[e], for e < E, is the number of window pixels taken from exposure e.
 * - counts[E] is the number of window pixels whose chosen exposure has n_e > 0, that is, pixels clipped in every exposure.
 *
 * Untouched.
 * - Masks of every view, and dense results of every view.
 * - The source views.
 * - Planes of dst_view that are not in use.
 * - Bytes outside the window's rows.
 * Pitch-padding bytes of dst_view's used planes are unspecified.
 * Nothing is written outside the view's own planes.
 *
 * The mask of dst_view is the caller's: set it as for any view (sl3d_set_mask, or sl3d_set_masks_modulated on the fused view); bit 7 of
 * the map is the mask of the pixels no exposure captures without clipping.  Reads frames only: works before sl3d_set_calibration, with and
 * without SL3D_FLAG_KEEP_STAGES, with every flag combination sl3d_create accepts.  Like every call that is not a run it comes behind the
 * launch lanes: a run over dst_view or over an exposure that is still in flight finishes first.  counts == NULL: the call enqueues and
 * returns; otherwise counts[n_exposures + 1] is downloaded and the call returns after the stream is idle.
 * SL3D_E_INVALID_ARG: a view out of range, n_exposures outside 1..SL3D_MAX_EXPOSURES, dst_view inside [first_view, first_view +
 * n_exposures), saturation outside 1..256.  SL3D_E_UNSUPPORTED: n_fringe == 5.  A refused call leaves every frame and map as it was. */
#define SL3D_MAX_EXPOSURES 8
int sl3d_fuse_exposures(sl3d_ctx *ctx, int first_view, int n_exposures, int dst_view, int saturation, uint32_t *counts /* [n_exposures + 1] or NULL */);

/* The exposure map the last sl3d_fuse_exposures into `view` left, window-sized row-major bytes (out[row * stride + col], stride >= width).
 * The map planes (max_views x pitch x height bytes) are allocated on the first fusion, owned by the context and freed by sl3d_destroy.
 * SL3D_E_INVALID_ARG: view out of range, null out, stride < width; SL3D_E_STATE: no fusion has written this view on this context.
 * Synchronises. */
int sl3d_get_exposure_map(sl3d_ctx *ctx, int view, uint8_t *out, size_t stride);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_FUSE_H */
