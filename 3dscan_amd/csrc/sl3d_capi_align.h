// sl3d_capi_align.h -- what the host units of the turntable code share (not part of the ABI; defined in sl3d_capi_align.cpp): the camera
// hand-over (sl3d_capi_tsdf.cpp takes it too), the argument checks, and -- over a description of the form, point-to-point
// (sl3d_capi_align.cpp) or point-to-plane (sl3d_capi_align_plane.cpp) -- one pass with its download and the refinement loop.
#pragma once
#include "sl3d_capi_internal.h"
#include "../../include/sl3d_align.h"
#include "sl3d_align.h"

inline bool positive_finite(float v) { return v > 0.0f && !std::isinf(v); }  // (false for NaN)
inline bool finite4(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3]); }

// the camera as a pass and an integration project with it: what sl3d_get_align_camera hands out
SL3D_INTERNAL void align_camera(const sl3d_ctx *x, AlignCam *m);

// one form of the refinement: which of the context's records (sl3d_ctx::align_rec) its passes fill, the words of a pair and the one that
// counts the sources, the scale of its lengths, the launch of a pass on the context's stream (the launcher clears the record) and the solve
struct AlignForm {
    int record, words, sources_word;
    double (*Q)(float range);
    int (*launch)(sl3d_ctx *x, int first_view, int n_pairs, int window, const AlignCam &cam, const AlignPass &a, unsigned long long *record);
    void (*solve)(const int64_t *sums, int n_pairs, double Q, double ox, double oz, const double *est_in, double *est_out, double *stats);
};

// every refusal of a pass, in front of the first allocation; `call` names the entry point in the text.  normal_edge: NULL for the
// point-to-point form
SL3D_INTERNAL int align_refusal(sl3d_ctx *x, int first_view, int n_views, float range, float max_dist, const float *normal_edge, int window,
                                const char *call);
// ... and of a refinement: those, then the iterations, the output and the start
SL3D_INTERNAL int refine_refusal(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range, float max_dist,
                                 const float *normal_edge, int window, int iterations, const sl3d_turntable *out, const char *call);
// The memset of the pairs' records and the form's pass on the context's stream (the caller holds ON_DEVICE); words != NULL: their download
// through the pinned block and the wait.
SL3D_INTERNAL int align_pass(sl3d_ctx *x, const AlignForm &f, int first_view, int n_views, const double est[4], double ox, double oz, float range,
                             float max_dist, int window, int64_t *words);
// the loop of pass and solve behind refine_refusal (the caller holds ON_DEVICE; the plane form's normals are there)
SL3D_INTERNAL int align_refine(sl3d_ctx *x, const AlignForm &f, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float range,
                               float max_dist, int window, int iterations, sl3d_turntable *out, sl3d_align_iteration *log, int *n_done);
// the host-only solve of a form behind its argument check
SL3D_INTERNAL int align_solve_checked(const AlignForm &f, const int64_t *sums, int n_pairs, float range, double ox, double oz, const double est_in[4],
                                      double est_out[4], double stats[4]);
