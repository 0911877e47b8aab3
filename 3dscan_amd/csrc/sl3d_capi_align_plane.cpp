// sl3d_capi_align_plane.cpp -- the point-to-plane turntable refinement (the rule: include/sl3d_align_plane.h; the kernels: sl3d_align_plane.hip,
// their arithmetic and the solve: sl3d_align_plane.h): sl3d_align_normals / sl3d_get_align_normals are the views' dense normals,
// sl3d_align_plane_sums the normals of the target views and one pass, sl3d_align_plane_solve the Gauss-Newton solve over its words,
// sl3d_refine_turntable_plane the loop.  The calls read the points / valid planes and write nothing but the context's own normal planes and
// records.
#include "sl3d_capi_internal.h"
#include "../../include/sl3d_align_plane.h"
#include "sl3d_align_plane.h"

static_assert(SL3D_ALIGN_PLANE_WORDS == ALIGN_PLANE_WORDS && SL3D_ALIGN_PLANE_STEPS == ALIGN_PLANE_STEPS, "the header's constants are the kernel's");

static bool positive_finite(float v) { return v > 0.0f && !std::isinf(v); }  // (false for NaN)
static bool finite4(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3]); }

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

// ... and of a pass: those of sl3d_align.h and the normal_edge
static int plane_refusal(sl3d_ctx *x, int first_view, int n_views, float range, float max_dist, float normal_edge, int window, const char *call)
{
    if (!x) return SL3D_E_INVALID_ARG;
    const std::string who = std::string(call) + ": ";
    if (n_views < 2) return fail(x, SL3D_E_INVALID_ARG, who + "n_views must be >= 2 (a pair is two consecutive views)");
    const int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!positive_finite(range) || !positive_finite(max_dist)) return fail(x, SL3D_E_INVALID_ARG, who + "range and max_dist must be finite and > 0");
    if (max_dist > range) return fail(x, SL3D_E_INVALID_ARG, who + "max_dist must not exceed range");
    if (!positive_finite(normal_edge)) return fail(x, SL3D_E_INVALID_ARG, who + "normal_edge must be finite and > 0");
    if (window < 0 || window > SL3D_ALIGN_MAX_WINDOW) return fail(x, SL3D_E_INVALID_ARG, who + "window must be 0 .. SL3D_ALIGN_MAX_WINDOW");
    if (!x->have_cal) return fail(x, SL3D_E_STATE, who + "sl3d_set_calibration has not been called");
    if (!x->dense_ran) return fail(x, SL3D_E_STATE, who + "no dense result yet (sl3d_run)");
    if ((int64_t)x->P.W * x->P.H >= ALIGN_MAX_PIXELS) return fail(x, SL3D_E_UNSUPPORTED, who + "width * height must stay below 2^25 (the words are exact int64 sums)");
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

static int ensure_records(sl3d_ctx *x)
{
    const size_t cap = (size_t)(x->cfg.max_views - 1) * ALIGN_PLANE_WORDS;
    const int rc = ensure_plane(x, &x->d_align_plane_rec, cap);
    if (rc) return rc;
    if (!x->h_align_plane_words) HIPCHK(x, hipHostMalloc((void **)&x->h_align_plane_words, cap * sizeof(long long), hipHostMallocDefault));
    return SL3D_OK;
}

// The memset of the pairs' records and k_align_plane_pass on the context's stream over normals that are there (the caller holds
// ON_DEVICE); words != NULL: their download through the pinned block and the wait.
static int plane_pass(sl3d_ctx *x, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist, int window,
                      int64_t *words)
{
    const size_t n = (size_t)(n_views - 1) * ALIGN_PLANE_WORDS;
    AlignCam cam;
    memcpy(cam.Rc, x->S.Rc, sizeof cam.Rc);
    memcpy(cam.tc, x->S.tc, sizeof cam.tc);
    memcpy(cam.Kc, x->Kc_raw, sizeof cam.Kc);
    memcpy(cam.dc, x->dc_raw, sizeof cam.dc);
    const AlignPass a{est[0], est[1], est[2], est[3], ox, oz, align_plane_Q(range), align_thr2(max_dist)};
    const int rc = launched(x, launch_align_plane_pass(x->P, first_view, n_views - 1, window, cam, a, normal_plane(x, first_view), x->d_align_plane_rec, x->stream));
    if (rc || !words) return rc;
    HIPCHK(x, hipMemcpyAsync(x->h_align_plane_words, x->d_align_plane_rec, n * sizeof(long long), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    memcpy(words, x->h_align_plane_words, n * sizeof(long long));
    return SL3D_OK;
}

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
    int rc = plane_refusal(x, first_view, n_views, range, max_dist, normal_edge, window, "align_plane_sums");
    if (rc) return rc;
    if (!est || !finite4(est) || !std::isfinite(ox) || !std::isfinite(oz)) return fail(x, SL3D_E_INVALID_ARG, "align_plane_sums: a null or non-finite estimate or centre");
    ON_DEVICE(x);
    if ((rc = ensure_records(x))) return rc;
    if ((rc = normals_pass(x, first_view, n_views - 1, normal_edge))) return rc;
    return plane_pass(x, first_view, n_views, est, ox, oz, range, max_dist, window, sums);
}
SL3D_CATCH(x)

extern "C" int sl3d_align_plane_solve(const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4],
                                      double stats[4])
try {
    if (!sums || !est_in || !est_out || !stats || n_pairs < 1 || !positive_finite(range) || !std::isfinite(ox) || !std::isfinite(oz) || !finite4(est_in))
        return SL3D_E_INVALID_ARG;
    align_plane_solve(sums, n_pairs, align_plane_Q(range), ox, oz, est_in, est_out, stats);
    return SL3D_OK;
}
SL3D_CATCH(nullptr)

extern "C" int sl3d_refine_turntable_plane(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range,
                                           float max_dist, float normal_edge, int window, int iterations, sl3d_turntable *out,
                                           sl3d_align_iteration *log, int *n_done)
try {
    int rc = plane_refusal(x, first_view, n_views, range, max_dist, normal_edge, window, "refine_turntable_plane");
    if (rc) return rc;
    if (iterations < 1 || iterations > SL3D_ALIGN_MAX_ITERATIONS) return fail(x, SL3D_E_INVALID_ARG, "refine_turntable_plane: iterations must be 1 .. 64");
    if (!out) return fail(x, SL3D_E_INVALID_ARG, "refine_turntable_plane: null output");
    if (!std::isfinite(tx) || !std::isfinite(ty) || !std::isfinite(tz) || !std::isfinite(rot_step))
        return fail(x, SL3D_E_INVALID_ARG, "refine_turntable_plane: a non-finite estimate");
    ON_DEVICE(x);
    if ((rc = ensure_records(x))) return rc;
    if ((rc = normals_pass(x, first_view, n_views - 1, normal_edge))) return rc;
    const double ox = (double)tx, oz = (double)tz, Qp = align_plane_Q(range);
    const double angle = rot_step * 22.0 / 7.0 / 180.0;  // turntable_R4's conversion
    double est[4] = {cos(angle), sin(angle), ox, oz}, stats[4] = {0.0, 0.0, 0.0, 1.0};
    const size_t n = (size_t)(n_views - 1) * ALIGN_PLANE_WORDS;
    std::vector<int64_t> words(n), before(n);
    int64_t sources = 0;
    int done = 0;
    for (int i = 0; i < iterations; i++) {
        if ((rc = plane_pass(x, first_view, n_views, est, ox, oz, range, max_dist, window, words.data()))) return rc;
        double next[4];
        align_plane_solve(words.data(), n_views - 1, Qp, ox, oz, est, next, stats);
        sources = 0;
        for (int j = 0; j < n_views - 1; j++) sources += words[(size_t)j * ALIGN_PLANE_WORDS + 16];
        if (log) {
            memcpy(log[i].est, est, sizeof est);
            log[i].n = (int64_t)stats[0], log[i].sources = sources, log[i].rms_xz = stats[1], log[i].rms_y = stats[2];
        }
        done = i + 1;
        if (stats[3] != 0.0) break;
        memcpy(est, next, sizeof est);
        if (i > 0 && words == before) break;
        before.swap(words);
    }
    out->tx = (float)est[2], out->ty = ty, out->tz = (float)est[3];
    out->rot_step = (float)(atan2(est[1], est[0]) * 180.0 * 7.0 / 22.0);
    memcpy(out->est, est, sizeof est);
    out->n = (int64_t)stats[0], out->sources = sources, out->rms_xz = stats[1], out->rms_y = stats[2];
    out->degenerate = stats[3] != 0.0, out->reserved = 0;
    if (n_done) *n_done = done;
    return SL3D_OK;
}
SL3D_CATCH(x)
