// sl3d_capi_align_plane.cpp -- the point-to-plane turntable refinement (the rule: include/sl3d_align_plane.h; the kernels: sl3d_align_plane.hip,
// their arithmetic and the solve: sl3d_align_plane.h): sl3d_align_normals / sl3d_get_align_normals are the views' dense normals,
// sl3d_align_plane_sums the normals of the target views and one pass, sl3d_align_plane_solve the Gauss-Newton solve over its words,
// sl3d_refine_turntable_plane the loop.  The calls read the points / valid planes and write nothing but the context's own normal planes and
// records.  The checks, the pass and the loop are those of sl3d_capi_align.h over this form.
#include "sl3d_capi_align.h"
#include "../../include/sl3d_align_plane.h"
#include "sl3d_align_plane.h"

static_assert(SL3D_ALIGN_PLANE_WORDS == ALIGN_PLANE_WORDS && SL3D_ALIGN_PLANE_STEPS == ALIGN_PLANE_STEPS, "the header's constants are the kernel's");

// every refusal of the normals of n_views >= 1 views, in front of the first allocation
static int normals_refusal(sl3d_ctx *x, int first_view, int n_views, float normal_edge, const std::string &who)
{
    if (n_views < 1) return fail(x, SL3D_E_INVALID_ARG, who + "n_views must be >= 1");
    const int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!positive_finite(normal_edge)) return fail(x, SL3D_E_INVALID_ARG, who + "normal_edge must be finite and > 0");
    if (!x->dense_ran) return fail(x, SL3D_E_STATE, who + "no dense result yet (sl3d_run)");
    return SL3D_OK;
}

static float *normal_plane(sl3d_ctx *x, int view) { return x->d_align_nrm + 3 * (size_t)(view - x->align_nrm_lo) * x->P.px_view_stride; }

// k_align_normals over the views on the context's stream (the caller holds ON_DEVICE).  The block spans every view asked for so far; a call
// that widens the span allocates anew, and the normals computed before are gone
static int normals_pass(sl3d_ctx *x, int first_view, int n_views, float normal_edge)
{
    const bool any = x->align_nrm_hi > x->align_nrm_lo;
    const int lo = any ? std::min(x->align_nrm_lo, first_view) : first_view, hi = any ? std::max(x->align_nrm_hi, first_view + n_views) : first_view + n_views;
    if (!any || lo != x->align_nrm_lo || hi != x->align_nrm_hi) {
        x->align_nrm_lo = x->align_nrm_hi = 0;
        x->align_nrm_ready.assign((size_t)x->cfg.max_views, 0);
        const int rc = grow_plane(x, &x->d_align_nrm, &x->align_nrm_cap, 3 * (size_t)(hi - lo) * x->P.px_view_stride);
        if (rc) return rc;
        x->align_nrm_lo = lo, x->align_nrm_hi = hi;
    }
    const int rc = launched(x, launch_align_normals(x->P, first_view, n_views, normal_edge, normal_plane(x, first_view), x->stream));
    if (rc) return rc;
    for (int v = first_view; v < first_view + n_views; v++) x->align_nrm_ready[(size_t)v] = 1;
    return SL3D_OK;
}

// k_align_plane_pass over normals that are there
static int launch_pass(sl3d_ctx *x, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, unsigned long long *record)
{
    return launch_align_plane_pass(x->P, first_view, n_pairs, window, cam, a, normal_plane(x, first_view), record, x->stream);
}
static const AlignForm PLANE = {1, ALIGN_PLANE_WORDS, 16, [](float range) { return align_plane_Q(range); }, launch_pass, align_plane_solve};

extern "C" int sl3d_align_normals(sl3d_ctx *x, int first_view, int n_views, float normal_edge)
try {
    if (!x) return SL3D_E_INVALID_ARG;
    const int rc = normals_refusal(x, first_view, n_views, normal_edge, "align_normals: ");
    if (rc) return rc;
    ON_DEVICE(x);
    return normals_pass(x, first_view, n_views, normal_edge);
}
SL3D_CATCH(x)

extern "C" int sl3d_get_align_normals(sl3d_ctx *x, int view, float *dst, size_t row_stride_bytes)
try {
    if (!x || !dst) return fail(x, SL3D_E_INVALID_ARG, "get_align_normals: null argument");
    const int rc = check_view(x, view);
    if (rc) return rc;
    if (row_stride_bytes % sizeof(float)) return fail(x, SL3D_E_INVALID_ARG, "get_align_normals: the row stride must be a multiple of 4");
    if (!x->d_align_nrm || view < x->align_nrm_lo || view >= x->align_nrm_hi || !x->align_nrm_ready[(size_t)view])
        return fail(x, SL3D_E_STATE, "get_align_normals: the view's normals have not been computed (sl3d_align_normals)");
    return download_plane(x, (const float *)normal_plane(x, view), 3, dst, row_stride_bytes / sizeof(float));
}
SL3D_CATCH(x)

extern "C" int sl3d_align_plane_sums(sl3d_ctx *x, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist,
                                     float normal_edge, int window, int64_t *sums)
try {
    int rc = align_refusal(x, first_view, n_views, range, max_dist, &normal_edge, window, "align_plane_sums");
    if (rc) return rc;
    if (!est || !finite4(est) || !std::isfinite(ox) || !std::isfinite(oz)) return fail(x, SL3D_E_INVALID_ARG, "align_plane_sums: a null or non-finite estimate or centre");
    ON_DEVICE(x);
    if ((rc = normals_pass(x, first_view, n_views - 1, normal_edge))) return rc;
    return align_pass(x, PLANE, first_view, n_views, est, ox, oz, range, max_dist, window, sums);
}
SL3D_CATCH(x)

extern "C" int sl3d_align_plane_solve(const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4],
                                      double stats[4])
try {
    return align_solve_checked(PLANE, sums, n_pairs, range, ox, oz, est_in, est_out, stats);
}
SL3D_CATCH(nullptr)

extern "C" int sl3d_refine_turntable_plane(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range,
                                           float max_dist, float normal_edge, int window, int iterations, sl3d_turntable *out,
                                           sl3d_align_iteration *log, int *n_done)
try {
    int rc = refine_refusal(x, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, &normal_edge, window, iterations, out, "refine_turntable_plane");
    if (rc) return rc;
    ON_DEVICE(x);
    if ((rc = normals_pass(x, first_view, n_views - 1, normal_edge))) return rc;
    return align_refine(x, PLANE, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, window, iterations, out, log, n_done);
}
SL3D_CATCH(x)
