// sl3d_capi_filter.cpp -- the radius outlier filter of the dense result (the rule: include/sl3d_filter.h; the kernels: sl3d_outlier.hip, their
// arithmetic: sl3d_outlier.h): sl3d_filter_outliers edits the points / valid planes of its views in place, so every consumer of a dense
// result (the getters, the compactions, the registration, the meshes) sees the filtered scan; sl3d_get_support hands out the support plane.
#include "sl3d_capi_internal.h"
#include "../../include/sl3d_filter.h"
#include "sl3d_outlier.h"

static_assert(SL3D_FILTER_MAX_RADIUS == SL3D_OUTLIER_MAX_RADIUS, "the header's bound is the kernels'");

// Two launches on the context's stream behind the launch lanes (ON_DEVICE): k_outlier_support over the planes as they are, then --
// unless nothing can be rejected and nobody asks for the counts -- k_outlier_apply, in front of it the memset of the views' count words.
// Every refusal comes before the first allocation.  Like sl3d_compact_views the call asks nothing of the views but that they exist: the
// planes are there, and zeroed, from sl3d_create on.
extern "C" int sl3d_filter_outliers(sl3d_ctx *x, int first_view, int n_views, int radius, float max_dist, int min_neighbours, uint32_t *counts)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (radius < 1 || radius > SL3D_FILTER_MAX_RADIUS) return fail(x, SL3D_E_INVALID_ARG, "filter_outliers: radius must be 1 .. SL3D_FILTER_MAX_RADIUS");
    if (!(max_dist > 0.0f)) return fail(x, SL3D_E_INVALID_ARG, "filter_outliers: max_dist must be > 0 (+infinity is allowed, NaN is not)");
    if (min_neighbours < 0 || min_neighbours > outlier_max_support(radius))
        return fail(x, SL3D_E_INVALID_ARG, "filter_outliers: min_neighbours must be 0 .. (2 * radius + 1)^2 - 1");
    const KParams &P = x->P;
    ON_DEVICE(x);
    if ((rc = ensure_plane(x, &x->d_support, (size_t)x->cfg.max_views * P.px_view_stride)) ||
        (rc = ensure_plane(x, &x->d_outlier_counts, 2 * (size_t)x->cfg.max_views)))
        return rc;
    x->support_written.resize((size_t)x->cfg.max_views, 0);
    rc = launched(x, launch_outlier_support(P, first_view, n_views, radius, max_dist, x->d_support, x->stream));
    if (rc) return rc;
    for (int v = first_view; v < first_view + n_views; v++) x->support_written[(size_t)v] = 1;
    if (min_neighbours == 0 && !counts) return SL3D_OK;  // nothing to reject, nothing to count
    unsigned *words = x->d_outlier_counts + 2 * (size_t)first_view;
    HIPCHK(x, hipMemsetAsync(words, 0, 2 * (size_t)n_views * sizeof(unsigned), x->stream));
    rc = launched(x, launch_outlier_apply(P, first_view, n_views, min_neighbours, x->d_support, words, x->stream));
    if (rc || !counts) return rc;
    HIPCHK(x, hipMemcpyAsync(counts, words, 2 * (size_t)n_views * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// the support plane the last sl3d_filter_outliers over `view` left: a byte per window pixel, 0xFF where the pixel was no sample
extern "C" int sl3d_get_support(sl3d_ctx *x, int view, uint8_t *out, size_t stride)
try {
    int rc = check_view(x, view);
    if (rc) return rc;
    if (!out || stride < (size_t)x->P.W) return fail(x, SL3D_E_INVALID_ARG, "get_support: null output or stride < width");
    if (!x->d_support || !x->support_written[(size_t)view]) return fail(x, SL3D_E_STATE, "get_support: no sl3d_filter_outliers has written this view");
    return download_plane(x, x->d_support + (size_t)view * x->P.px_view_stride, 1, out, stride);
}
SL3D_CATCH(x)
