// sl3d_capi_subpixel.cpp -- sl3d_triangulate_subpixel, sl3d_get_residuals, sl3d_get_correspondences_subpixel: stage 7 from the continuous
// projector coordinates and the reprojection residual of its solve.  The argument checks are subpixel_check_args
// (sl3d_subpixel.h, which tests/native/subpixel_check.cpp compiles without HIP); the kernels are sl3d_subpixel.hip.
#include "sl3d_capi_internal.h"
#include "sl3d_subpixel.h"

static_assert(SL3D_E_INVALID_ARG == -1 && SL3D_E_STATE == -4, "subpixel_check_args returns these values");

extern "C" int sl3d_triangulate_subpixel(sl3d_ctx *x, int first_view, int n_views, double max_residual, uint32_t *counts)
try {
    if (!x) return SL3D_E_INVALID_ARG;
    const int status = subpixel_check_args(first_view, n_views, x->cfg.max_views, x->keep, x->have_cal, max_residual);
    if (status) {  // (nothing has been touched; in the words of every stage entry point)
        int rc = check_view(x, first_view, n_views);
        if (rc || (rc = need_keep(x))) return rc;
        if (status == SL3D_E_STATE) return fail(x, status, "sl3d_set_calibration has not been called");
        if (max_residual > 0.0) return fail(x, status, "view index out of range");  // (an n_views check_view's own sum cannot hold)
        return fail(x, status, "triangulate_subpixel: max_residual must be positive (+infinity: no pixel is rejected)");
    }
    if (x->one_axis >= 0) {  // the exactly determined solve: no residual, so nothing to reject by; counts = (triangulated, 0)
        if (subpixel_rejects(max_residual))  // (nothing has been touched)
            return fail(x, SL3D_E_UNSUPPORTED, "triangulate_subpixel: a SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL context has no residual to reject "
                                               "by: pass +infinity");
        ON_DEVICE(x);
        if (counts) {
            int rc = ensure_plane(x, &x->d_subpixel_counts, (size_t)x->cfg.max_views * 2);
            if (!rc) rc = ensure_plane(x, &x->d_subpixel_partials, (size_t)x->cfg.max_views * subpixel_blocks(x->P));
            if (rc) return rc;
        }
        int rc = launched(x, launch_subpixel_one(x->P, x->C, x->one_axis, first_view, n_views, counts ? x->d_subpixel_partials : nullptr, x->d_subpixel_counts,
                                                 x->anchor, x->stream));
        if (rc) return rc;
        x->dense_ran = true;
        if (counts) {
            HIPCHK(x, hipMemcpyAsync(counts, x->d_subpixel_counts, 2 * (size_t)n_views * sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
            SYNC_FOR_CALLER(x);
        }
        return SL3D_OK;
    }
    ON_DEVICE(x);
    const size_t plane = (size_t)x->cfg.max_views * x->P.px_view_stride;
    if (!x->d_residual) {  // NaN everywhere: the views no call has triangulated yet
        int rc = ensure_plane(x, &x->d_residual, plane);
        if (rc) return rc;
        HIPCHK(x, hipMemsetAsync(x->d_residual, 0xff, plane * sizeof(float), x->stream));
    }
    if (counts) {
        int rc = ensure_plane(x, &x->d_subpixel_counts, (size_t)x->cfg.max_views * 2);
        if (!rc) rc = ensure_plane(x, &x->d_subpixel_partials, (size_t)x->cfg.max_views * subpixel_blocks(x->P));
        if (rc) return rc;
    }
    unsigned *cnt = x->d_subpixel_counts;
    int rc = launched(x, launch_subpixel(x->P, x->C, first_view, n_views, max_residual, x->d_residual, counts ? x->d_subpixel_partials : nullptr, cnt, x->anchor, x->stream));
    if (rc) return rc;
    x->residual_ready = x->dense_ran = true;
    if (counts) {
        HIPCHK(x, hipMemcpyAsync(counts, cnt, 2 * (size_t)n_views * sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
        SYNC_FOR_CALLER(x);
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

extern "C" int sl3d_get_residuals(sl3d_ctx *x, int view, float *out, size_t stride)
try {
    int rc = check_view(x, view);
    if (rc) return rc;
    if (!out) return fail(x, SL3D_E_INVALID_ARG, "null output");
    if (x->one_axis >= 0)
        return fail(x, SL3D_E_UNSUPPORTED, "get_residuals: a SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL context has no residuals: three equations "
                                           "determine the three unknowns exactly");
    if (!x->d_residual || !x->residual_ready)
        return fail(x, SL3D_E_STATE, x->subpixel && !x->keep ? "no residuals: sl3d_run has not been called on this SL3D_FLAG_SUBPIXEL context"
                                     : x->subpixel         ? "no residuals: neither sl3d_run nor sl3d_triangulate_subpixel has been called"
                                                           : "no residuals: sl3d_triangulate_subpixel has not been called");
    return download_plane(x, x->d_residual + (size_t)view * x->P.px_view_stride, 1, out, stride);
}
SL3D_CATCH(x)

extern "C" int sl3d_get_correspondences_subpixel(sl3d_ctx *x, int view, double *xy, size_t stride)
try {
    int rc = check_view(x, view);
    if (rc || (rc = need_keep(x))) return rc;
    if (!xy) return fail(x, SL3D_E_INVALID_ARG, "null output");
    if (stride < (size_t)x->P.W) return fail(x, SL3D_E_INVALID_ARG, "output stride too small");
    ON_DEVICE(x);
    if ((rc = ensure_plane(x, &x->d_subpixel_xy, 2 * x->P.px_view_stride))) return rc;
    if (x->one_axis >= 0) rc = launched(x, launch_subpixel_coords_one(x->P, x->one_axis, view, x->d_subpixel_xy, x->anchor, x->stream));
    else rc = launched(x, launch_subpixel_coords(x->P, view, x->d_subpixel_xy, x->anchor, x->stream));
    if (rc) return rc;
    return download_plane(x, x->d_subpixel_xy, 2, xy, 2 * stride);
}
SL3D_CATCH(x)
