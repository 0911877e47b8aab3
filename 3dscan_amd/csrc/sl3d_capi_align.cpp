// sl3d_capi_align.cpp -- the turntable refinement (the rule: include/sl3d_align.h; the kernel: sl3d_align.hip, its arithmetic and the solve:
// sl3d_align.h): sl3d_align_sums is one correspondence pass over consecutive views' dense planes, sl3d_align_solve the closed-form solve
// over its words, sl3d_refine_turntable the loop of the two, sl3d_get_align_camera the camera the pass projects with.  The calls read the
// points / valid planes and write nothing but the context's own records.  Also what this form shares with the point-to-plane one
// (sl3d_capi_align.h): the checks, the pass and the loop over an AlignForm.
#include "sl3d_capi_align.h"

static_assert(SL3D_ALIGN_WORDS == ALIGN_WORDS && SL3D_ALIGN_MAX_WINDOW == ALIGN_MAX_WINDOW, "the header's constants are the kernel's");

void align_camera(const sl3d_ctx *x, AlignCam *m)
{
    memcpy(m->Rc, x->S.Rc, sizeof m->Rc);
    memcpy(m->tc, x->S.tc, sizeof m->tc);
    memcpy(m->Kc, x->Kc_raw, sizeof m->Kc);
    memcpy(m->dc, x->dc_raw, sizeof m->dc);
}

int align_refusal(sl3d_ctx *x, int first_view, int n_views, float range, float max_dist, const float *normal_edge, int window, const char *call)
{
    if (!x) return SL3D_E_INVALID_ARG;
    const std::string who = std::string(call) + ": ";
    if (n_views < 2) return fail(x, SL3D_E_INVALID_ARG, who + "n_views must be >= 2 (a pair is two consecutive views)");
    const int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!positive_finite(range) || !positive_finite(max_dist)) return fail(x, SL3D_E_INVALID_ARG, who + "range and max_dist must be finite and > 0");
    if (max_dist > range) return fail(x, SL3D_E_INVALID_ARG, who + "max_dist must not exceed range");
    if (normal_edge && !positive_finite(*normal_edge)) return fail(x, SL3D_E_INVALID_ARG, who + "normal_edge must be finite and > 0");
    if (window < 0 || window > SL3D_ALIGN_MAX_WINDOW) return fail(x, SL3D_E_INVALID_ARG, who + "window must be 0 .. SL3D_ALIGN_MAX_WINDOW");
    if (!x->have_cal) return fail(x, SL3D_E_STATE, who + "sl3d_set_calibration has not been called");
    if (!x->dense_ran) return fail(x, SL3D_E_STATE, who + "no dense result yet (sl3d_run)");
    if ((int64_t)x->P.W * x->P.H >= ALIGN_MAX_PIXELS) return fail(x, SL3D_E_UNSUPPORTED, who + "width * height must stay below 2^25 (the words are exact int64 sums)");
    return SL3D_OK;
}

int refine_refusal(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range, float max_dist,
                   const float *normal_edge, int window, int iterations, const sl3d_turntable *out, const char *call)
{
    const int rc = align_refusal(x, first_view, n_views, range, max_dist, normal_edge, window, call);
    if (rc) return rc;
    const std::string who = std::string(call) + ": ";
    static_assert(SL3D_ALIGN_MAX_ITERATIONS == 64, "the text below names it");
    if (iterations < 1 || iterations > SL3D_ALIGN_MAX_ITERATIONS) return fail(x, SL3D_E_INVALID_ARG, who + "iterations must be 1 .. 64");
    if (!out) return fail(x, SL3D_E_INVALID_ARG, who + "null output");
    if (!std::isfinite(tx) || !std::isfinite(ty) || !std::isfinite(tz) || !std::isfinite(rot_step)) return fail(x, SL3D_E_INVALID_ARG, who + "a non-finite estimate");
    return SL3D_OK;
}

int align_pass(sl3d_ctx *x, const AlignForm &f, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist,
               int window, int64_t *words)
{
    sl3d_ctx::AlignRecord &r = x->align_rec[f.record];
    const size_t cap = (size_t)(x->cfg.max_views - 1) * f.words, n = (size_t)(n_views - 1) * f.words;
    int rc = ensure_plane(x, &r.dev, cap);
    if (rc) return rc;
    if (!r.host) HIPCHK(x, hipHostMalloc((void **)&r.host, cap * sizeof(long long), hipHostMallocDefault));
    AlignCam cam;
    align_camera(x, &cam);
    const AlignPass a{est[0], est[1], est[2], est[3], ox, oz, f.Q(range), align_thr2(max_dist)};
    rc = launched(x, f.launch(x, first_view, n_views - 1, window, cam, a, r.dev));
    if (rc || !words) return rc;
    HIPCHK(x, hipMemcpyAsync(r.host, r.dev, n * sizeof(long long), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    memcpy(words, r.host, n * sizeof(long long));
    return SL3D_OK;
}

int align_refine(sl3d_ctx *x, const AlignForm &f, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range,
                 float max_dist, int window, int iterations, sl3d_turntable *out, sl3d_align_iteration *log, int *n_done)
{
    const double ox = (double)tx, oz = (double)tz, Q = f.Q(range);
    const double angle = rot_step * 22.0 / 7.0 / 180.0;  // turntable_R4's conversion
    double est[4] = {cos(angle), sin(angle), ox, oz}, stats[4] = {0.0, 0.0, 0.0, 1.0};
    const size_t n = (size_t)(n_views - 1) * f.words;
    std::vector<int64_t> words(n), before(n);
    int64_t sources = 0;
    int done = 0;
    for (int i = 0; i < iterations; i++) {
        const int rc = align_pass(x, f, first_view, n_views, est, ox, oz, range, max_dist, window, words.data());
        if (rc) return rc;
        double next[4];
        f.solve(words.data(), n_views - 1, Q, ox, oz, est, next, stats);
        sources = 0;
        for (int j = 0; j < n_views - 1; j++) sources += words[(size_t)j * f.words + f.sources_word];
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

int align_solve_checked(const AlignForm &f, const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4],
                        double stats[4])
{
    if (!sums || !est_in || !est_out || !stats || n_pairs < 1 || !positive_finite(range) || !std::isfinite(ox) || !std::isfinite(oz) || !finite4(est_in))
        return SL3D_E_INVALID_ARG;
    f.solve(sums, n_pairs, f.Q(range), ox, oz, est_in, est_out, stats);
    return SL3D_OK;
}

// ---- the point-to-point form --------------------------------------------------------------------------------------------------------------
static int launch_pass(sl3d_ctx *x, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, unsigned long long *record)
{
    return launch_align_pass(x->P, first_view, n_pairs, window, cam, a, record, x->stream);
}
static const AlignForm POINT = {0, ALIGN_WORDS, 11, [](float range) { return align_Q(range); }, launch_pass, align_solve};

extern "C" int sl3d_align_sums(sl3d_ctx *x, int first_view, int n_views, const double est[4], double ox, double oz, float range, float max_dist, int window,
                               int64_t *sums)
try {
    const int rc = align_refusal(x, first_view, n_views, range, max_dist, nullptr, window, "align_sums");
    if (rc) return rc;
    if (!est || !finite4(est) || !std::isfinite(ox) || !std::isfinite(oz)) return fail(x, SL3D_E_INVALID_ARG, "align_sums: a null or non-finite estimate or centre");
    ON_DEVICE(x);
    return align_pass(x, POINT, first_view, n_views, est, ox, oz, range, max_dist, window, sums);
}
SL3D_CATCH(x)

extern "C" int sl3d_align_solve(const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4], double est_out[4], double stats[4])
try {
    return align_solve_checked(POINT, sums, n_pairs, range, ox, oz, est_in, est_out, stats);
}
SL3D_CATCH(nullptr)

extern "C" int sl3d_refine_turntable(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range, float max_dist,
                                     int window, int iterations, sl3d_turntable *out, sl3d_align_iteration *log, int *n_done)
try {
    const int rc = refine_refusal(x, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, nullptr, window, iterations, out, "refine_turntable");
    if (rc) return rc;
    ON_DEVICE(x);
    return align_refine(x, POINT, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, window, iterations, out, log, n_done);
}
SL3D_CATCH(x)

extern "C" int sl3d_get_align_camera(sl3d_ctx *x, double cam[26])
try {
    if (!x || !cam) return fail(x, SL3D_E_INVALID_ARG, "get_align_camera: null argument");
    if (!x->have_cal) return fail(x, SL3D_E_STATE, "sl3d_set_calibration has not been called");
    AlignCam m;
    align_camera(x, &m);
    static_assert(sizeof m == 26 * sizeof(double), "Rc, tc, Kc, dc back to back");
    memcpy(cam, &m, sizeof m);
    return SL3D_OK;
}
SL3D_CATCH(x)
