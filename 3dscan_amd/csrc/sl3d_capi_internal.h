// sl3d_capi_internal.h -- what the translation units behind include/sl3d.h share (not part of the ABI; every symbol is hidden):
//   sl3d_capi_context.cpp  errors, sl3d_create / sl3d_destroy, calibration (T0 and the per-calibration tables), stream helpers
//   sl3d_capi_inputs.cpp   selection masks (prepared now or deferred to the launch: H0 / S3b / S3d) and frames in, [col][row] layouts
//   sl3d_capi_run.cpp      the per-stage entry points, every fused launch (run_fused, by fused_route below), getters, the host-buffer pipeline
//   sl3d_capi_clouds.cpp   O1 / N2 / N3: ordered clouds, their consumers, colour, registration
//   sl3d_capi_next.cpp     N1 / N4: patterns, synthetic captures, cvUndistort2, plain device copies
//   sl3d_capi_period.cpp   the period repair between stage 4 and stage 5 (sl3d_repair_periods)
//   sl3d_capi_subpixel.cpp stage 7 from the continuous correspondences, its residual plane (sl3d_triangulate_subpixel and its getters)
//   sl3d_capi_filter.cpp   the radius outlier filter of the dense result (include/sl3d_filter.h: sl3d_filter_outliers, sl3d_get_support)
//   sl3d_capi_voxel.cpp    the voxel grid over a cloud (include/sl3d_voxel.h: sl3d_voxel_grid, sl3d_get_voxel_grid)
//   sl3d_capi_align.cpp    the turntable refinement (include/sl3d_align.h: sl3d_align_sums, sl3d_align_solve, sl3d_refine_turntable, sl3d_get_align_camera)
//   sl3d_capi_align_plane.cpp  its point-to-plane form (include/sl3d_align_plane.h: sl3d_align_normals, sl3d_get_align_normals, sl3d_align_plane_sums,
//                          sl3d_align_plane_solve, sl3d_refine_turntable_plane)
//   sl3d_capi_tsdf.cpp     the TSDF volume (include/sl3d_tsdf.h: sl3d_tsdf_reset, sl3d_tsdf_integrate, sl3d_tsdf_extract and the two getters)
//   sl3d_capi_align.h      what those three share beyond this header: the camera hand-over, the checks, one pass and one loop over an AlignForm
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "sl3d_ctx.h"

#define SL3D_INTERNAL __attribute__((visibility("hidden")))

template <typename T>
inline int dev_alloc(sl3d_ctx *c, T **p, size_t count)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T));
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? SL3D_E_NOMEM : SL3D_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    c->allocs.push_back(q);
    *p = (T *)q;
    return SL3D_OK;
}

// allocates what a scratch of `counts` counts (and as many scanned offsets) and `totals` totals still lacks: a set-up that failed half way
// goes on from there at the next call, nothing is allocated twice
inline int ensure_scratch(sl3d_ctx *c, CompactScratch &s, size_t counts, size_t totals)
{
    int rc = SL3D_OK;
    if (!s.cnt) rc = dev_alloc(c, &s.cnt, counts);
    if (!rc && !s.off) rc = dev_alloc(c, &s.off, counts);
    if (!rc && !s.tot) rc = dev_alloc(c, &s.tot, totals);
    return rc;
}

// allocates a plane of `count` elements unless an earlier attempt already has
template <typename T>
inline int ensure_plane(sl3d_ctx *c, T **p, size_t count)
{
    return *p ? SL3D_OK : dev_alloc(c, p, count);
}

// a plane of at least `count` elements: *cap of them are there; one that is too small is freed (the device is idle then: hipFree
// waits) and allocated again
template <typename T>
inline int grow_plane(sl3d_ctx *c, T **p, size_t *cap, size_t count)
{
    if (*p && *cap >= count) return SL3D_OK;
    if (*p) {
        (void)hipFree(*p);
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)*p), c->allocs.end());
        *p = nullptr;
        *cap = 0;
    }
    const int rc = dev_alloc(c, p, count);
    if (!rc) *cap = count;
    return rc;
}

SL3D_INTERNAL int launched(sl3d_ctx *x, int hip_err);   // a launch's hipError_t -> status (+ the context's error text)
SL3D_INTERNAL int need_keep(sl3d_ctx *x);               // SL3D_E_STATE unless the context keeps the stage planes
SL3D_INTERNAL int check_view(sl3d_ctx *x, int view, int n = 1);
// a per-stage call `call` on `axis`: SL3D_E_UNSUPPORTED on the axis a one-axis context does not code (sl3d_capi_run.cpp)
SL3D_INTERNAL int one_axis_serves(sl3d_ctx *x, int axis, const char *call);
// what kind of memory `p` is: 0 = pageable host, 1 = pinned host, 2 = device (*device = its ordinal)
SL3D_INTERNAL int memory_kind(const void *p, int *device = nullptr);
SL3D_INTERNAL bool is_pinned_host(const void *p);
SL3D_INTERNAL int ensure_colrow(sl3d_ctx *x, size_t bytes);
SL3D_INTERNAL void turntable_R4(float theta_deg, float R4[4]);  // the turntable's rotation by theta (sl3d_capi_next.cpp)

// the part of the mask plane that holds source pixels: the window + 2-pixel halo, clipped to the frame
struct MaskRegion {
    int gx0, gx1, gy0, gy1;
};
SL3D_INTERNAL MaskRegion mask_region(const KParams &P, MaskSrc &S);
// selected quads of a view as its last preparation counted them / are all views of a launch known to be sparsely selected
SL3D_INTERNAL bool quads_known(const sl3d_ctx *x, int view, unsigned *quads);
SL3D_INTERNAL bool sparse_views(const sl3d_ctx *x, int first, int n);
// deferred masks (sl3d_capi_inputs.cpp): prepare what is still deferred of views [first_view, first_view + n_views) (callers_only: only
// masks that lie in the CALLER's memory); drop / prepare what a new mask of those views supersedes; drain the stream for the caller
SL3D_INTERNAL int flush_masks(sl3d_ctx *x, int first_view, int n_views, bool callers_only = false);
SL3D_INTERNAL int supersede_masks(sl3d_ctx *x, int first_view, int n_views, int slots);
SL3D_INTERNAL int sync_for_caller(sl3d_ctx *x);
#define SYNC_FOR_CALLER(x)                     \
    do {                                       \
        const int rc_ = sync_for_caller(x);    \
        if (rc_) return rc_;                   \
    } while (0)

// the window of one view's plane (`comps` elements per pixel, rows P.pitch pixels apart, at src) into the caller's rows (out: not
// NULL), then the wait
template <typename T>
inline int download_plane(sl3d_ctx *x, const T *src, int comps, T *out, size_t out_stride_elems)
{
    const KParams &P = x->P;
    if (out_stride_elems < (size_t)P.W * comps) return fail(x, SL3D_E_INVALID_ARG, "output stride too small");
    ON_DEVICE(x);
    HIPCHK(x, hipMemcpy2DAsync(out, out_stride_elems * sizeof(T), src, (size_t)P.pitch * comps * sizeof(T), (size_t)P.W * comps * sizeof(T),
                               P.H, hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}

// THE routing decision of a context: what a fused launch of it -- every one goes through run_fused (sl3d_capi_run.cpp) -- puts on the device.
// run_fused launches by it; own_kernel_name, sl3d_fused_kernel_name, sl3d_last_fused_kernel_name and sl3d_camera_table_bytes_per_pixel report
// by it.  Whichever route a flag set takes, sl3d_run leaves the same scan with and without SL3D_FLAG_KEEP_STAGES.
enum FusedRoute {
    ROUTE_K_FUSED,  // neither SL3D_FLAG_SUBPIXEL nor SL3D_FLAG_REPAIR_PERIODS: a k_fused instantiation alone (run_k_fused: on the stream or a lane)
    // SL3D_FLAG_KEEP_STAGES with one of the two, both axes against the inverse planes: the parity k_fused; with the repair one pass of the
    // staged repair over every axis that has Gray planes, stage 5 again and stage 7 over the repaired phases; with SL3D_FLAG_SUBPIXEL k_subpixel
    // (+infinity, no counts) last, in place of stage 7
    ROUTE_K_FUSED_THEN_STAGES,
    // SL3D_FLAG_KEEP_STAGES on a one-axis (SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL) or a SL3D_FLAG_DIRECT_GRAY context: never the parity k_fused,
    // which reads both axes and the inverse planes.  Per view k_wrap and stage 4 (launch_stage4) of every coded axis and stage 5 (k_corr, or
    // k_corr_one), then the sub-pixel launch over the views (k_subpixel, or k_subpixel_one)
    ROUTE_STAGED,
    // no SL3D_FLAG_KEEP_STAGES: ONE launch of the context's own kernel (sl3d_quad.h) per call, on the context's stream behind the preparation of
    // the views' deferred masks -- no k_fused instantiation, no lanes, no camera table.  SL3D_FLAG_ANCHOR_PERIODS: the first three's anchored form
    ROUTE_SUBPIXEL_FUSED,  // SL3D_FLAG_SUBPIXEL: k_subpixel_fused
    ROUTE_ONE_AXIS,        // ... with a one-axis flag: k_one_axis
    ROUTE_DIRECT_GRAY,     // ... with SL3D_FLAG_DIRECT_GRAY, with or without a one-axis flag: k_direct_gray, its one-axis or its two-axis form
    ROUTE_REPAIR_FUSED     // SL3D_FLAG_REPAIR_PERIODS: k_repair_fused, with the sub-pixel ending if the context has SL3D_FLAG_SUBPIXEL too
};
inline FusedRoute fused_route(const sl3d_ctx *x)
{
    if (!x->subpixel && !x->repair) return ROUTE_K_FUSED;
    if (x->keep) return x->one_axis >= 0 || x->direct_gray ? ROUTE_STAGED : ROUTE_K_FUSED_THEN_STAGES;
    if (x->repair) return ROUTE_REPAIR_FUSED;  // (never with a one-axis flag or SL3D_FLAG_DIRECT_GRAY: sl3d_create refuses)
    if (x->direct_gray) return ROUTE_DIRECT_GRAY;
    return x->one_axis >= 0 ? ROUTE_ONE_AXIS : ROUTE_SUBPIXEL_FUSED;
}
inline bool own_kernel(FusedRoute r) { return r == ROUTE_SUBPIXEL_FUSED || r == ROUTE_ONE_AXIS || r == ROUTE_DIRECT_GRAY || r == ROUTE_REPAIR_FUSED; }
// stage 4 of one axis of a view on the context's stream: by the direct rule on a SL3D_FLAG_DIRECT_GRAY context (k_unwrap itself is untouched)
inline int launch_stage4(const sl3d_ctx *x, int view, int axis)
{
    return x->direct_gray ? launch_unwrap_direct(x->P, view, axis, x->stream) : launch_unwrap(x->P, view, axis, x->stream);
}
inline const char *own_kernel_name(const sl3d_ctx *x)  // (of a context whose route is an own_kernel)
{
    switch (fused_route(x)) {
    case ROUTE_DIRECT_GRAY: return SL3D_DIRECT_GRAY_NAME(x->one_axis >= 0 ? x->one_axis : 2, x->anchor);
    case ROUTE_ONE_AXIS: return SL3D_ONE_AXIS_NAME(x->one_axis, x->anchor);
    case ROUTE_REPAIR_FUSED: return x->subpixel ? SL3D_REPAIR_FUSED_SUB_NAME : SL3D_REPAIR_FUSED_NAME;
    default: return x->anchor ? SL3D_SUBPIXEL_FUSED_ANCHOR_NAME : SL3D_SUBPIXEL_FUSED_NAME;
    }
}
// the launches of sl3d_repair_periods (sl3d_capi_period.cpp): one pass over one axis of one view behind whatever the stream holds; the
// counts are added to the view's and the axis's two words of d_period_counts, which the caller has cleared if it reads them
SL3D_INTERNAL int period_repair_enqueue(sl3d_ctx *x, int view, int axis, int radius);
SL3D_INTERNAL bool maskin_launch(const sl3d_ctx *x, int first_view, int n_views, bool keep);
SL3D_INTERNAL int small_launch_overlaps(sl3d_ctx *x, int first_view, int n_views, bool *overlap);
SL3D_INTERNAL int run_fused(sl3d_ctx *x, int first_view, int n_views, bool keep, int cmode, bool may_overlap = false);
