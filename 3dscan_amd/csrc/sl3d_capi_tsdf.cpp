// sl3d_capi_tsdf.cpp -- the TSDF volume (the rule: include/sl3d_tsdf.h; the kernels: sl3d_tsdf.hip, their arithmetic: sl3d_tsdf.h):
// sl3d_tsdf_reset defines and clears the volume, sl3d_tsdf_integrate adds views of the dense result to it, sl3d_tsdf_extract leaves the
// oriented points of its zero level on the device; sl3d_get_tsdf and sl3d_get_tsdf_surface hand the planes and the surface out.  The calls
// read the points / valid planes and write nothing but the context's own volume, surface and words.
#include "sl3d_capi_align.h"  // align_camera
#include "../../include/sl3d_tsdf.h"
#include "sl3d_tsdf.h"

// the arrays of the context that grow with the volume or the surface, in the order of sl3d_ctx::tsdf_cap
enum { TSDF_SUM, TSDF_WEIGHT, TSDF_CNT, TSDF_OFF, TSDF_XYZ, TSDF_NRM, TSDF_EDGE, TSDF_DEPTH };

static int64_t tsdf_voxels(const int32_t *d) { return (int64_t)d[0] * d[1] * d[2]; }

static TsdfVolume tsdf_volume(const sl3d_ctx *x)
{
    TsdfVolume v;
    for (int a = 0; a < 3; a++) v.o[a] = (double)x->tsdf_origin[a], v.n[a] = x->tsdf_dims[a];
    v.L = (double)x->tsdf_voxel, v.T = (double)x->tsdf_trunc;
    return v;
}

extern "C" int sl3d_tsdf_reset(sl3d_ctx *x, const sl3d_tsdf_volume *vol)
try {
    if (!x) return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: null context");
    if (!vol) return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: null volume");
    if (!(vol->voxel > 0.0f) || std::isinf(vol->voxel) || !(vol->trunc > 0.0f) || std::isinf(vol->trunc))
        return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: voxel and trunc must be finite and > 0");
    if (!std::isfinite(vol->origin[0]) || !std::isfinite(vol->origin[1]) || !std::isfinite(vol->origin[2]))
        return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: a non-finite origin");
    if (vol->dims[0] < 1 || vol->dims[1] < 1 || vol->dims[2] < 1) return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: every dim must be >= 1");
    if ((int64_t)vol->dims[0] * vol->dims[1] > TSDF_MAX_VOXELS || tsdf_voxels(vol->dims) > TSDF_MAX_VOXELS)
        return fail(x, SL3D_E_INVALID_ARG, "tsdf_reset: more than 2^28 voxels");
    ON_DEVICE(x);
    const size_t n = (size_t)tsdf_voxels(vol->dims);
    x->tsdf_dims[0] = 0, x->tsdf_m = -1;  // (from here on the last volume and its surface are gone)
    int rc = grow_plane(x, &x->d_tsdf_sum, &x->tsdf_cap[TSDF_SUM], n);
    if (!rc) rc = grow_plane(x, &x->d_tsdf_weight, &x->tsdf_cap[TSDF_WEIGHT], n);
    if (!rc) rc = ensure_plane(x, &x->d_tsdf_words, (size_t)TSDF_WORDS);
    if (!rc) rc = ensure_plane(x, &x->d_tsdf_turns, 2 * (size_t)x->cfg.max_views);
    if (rc) return rc;
    HIPCHK(x, hipMemsetAsync(x->d_tsdf_sum, 0, n * sizeof(int32_t), x->stream));
    HIPCHK(x, hipMemsetAsync(x->d_tsdf_weight, 0, n * sizeof(uint32_t), x->stream));
    HIPCHK(x, hipMemsetAsync(x->d_tsdf_words, 0, TSDF_WORDS * sizeof(unsigned long long), x->stream));
    memcpy(x->tsdf_origin, vol->origin, sizeof x->tsdf_origin);
    x->tsdf_voxel = vol->voxel, x->tsdf_trunc = vol->trunc;
    memcpy(x->tsdf_dims, vol->dims, sizeof x->tsdf_dims);
    x->tsdf_views = 0;
    return SL3D_OK;
}
SL3D_CATCH(x)

// The upload of the views' rotations, the memset of the call's words, k_tsdf_depth and k_tsdf_integrate on the context's stream behind the launch
// lanes (ON_DEVICE).  Every refusal comes before the first allocation.
extern "C" int sl3d_tsdf_integrate(sl3d_ctx *x, int first_view, int n_views, int first_step, const double est[4], int64_t counts[2])
try {
    if (!x) return fail(x, SL3D_E_INVALID_ARG, "tsdf_integrate: null context");
    if (n_views < 1) return fail(x, SL3D_E_INVALID_ARG, "tsdf_integrate: n_views must be >= 1");
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (first_step < 0 || (int64_t)first_step + n_views > TSDF_MAX_STEPS)
        return fail(x, SL3D_E_INVALID_ARG, "tsdf_integrate: first_step must be >= 0 and first_step + n_views <= 65535");
    if (!est || !finite4(est)) return fail(x, SL3D_E_INVALID_ARG, "tsdf_integrate: a null or non-finite estimate");
    if (!x->have_cal) return fail(x, SL3D_E_STATE, "tsdf_integrate: sl3d_set_calibration has not been called");
    if (!x->dense_ran) return fail(x, SL3D_E_STATE, "tsdf_integrate: no dense result yet (sl3d_run)");
    if (!x->tsdf_dims[0]) return fail(x, SL3D_E_STATE, "tsdf_integrate: no sl3d_tsdf_reset has defined a volume");
    if (x->tsdf_views + n_views > TSDF_MAX_STEPS)
        return fail(x, SL3D_E_UNSUPPORTED, "tsdf_integrate: more than 65535 views since the last sl3d_tsdf_reset (sum is an int32)");
    ON_DEVICE(x);
    rc = grow_plane(x, &x->d_tsdf_depth, &x->tsdf_cap[TSDF_DEPTH], (size_t)n_views * x->P.px_view_stride);
    if (rc) return rc;
    // the rotations: the recurrence from index 0 up to the last index of the call
    std::vector<TsdfTurn> turns((size_t)n_views);
    TsdfTurn t = {1.0, 0.0};
    for (int m = 0; m < first_step + n_views; m++) {
        if (m >= first_step) turns[(size_t)(m - first_step)] = t;
        t = tsdf_next_turn(t, est[0], est[1]);
    }
    static_assert(sizeof(TsdfTurn) == 2 * sizeof(double), "c, s back to back");
    // (pageable memory: it has been read when the copy returns)
    HIPCHK(x, hipMemcpyAsync(x->d_tsdf_turns, turns.data(), turns.size() * sizeof(TsdfTurn), hipMemcpyHostToDevice, x->stream));
    AlignCam cam;
    align_camera(x, &cam);
    rc = launched(x, launch_tsdf_integrate(x->P, first_view, n_views, cam, tsdf_volume(x), est[2], est[3], (const TsdfTurn *)x->d_tsdf_turns, x->d_tsdf_depth, x->d_tsdf_sum,
                                           x->d_tsdf_weight, x->d_tsdf_words, x->stream));
    if (rc) return rc;
    x->tsdf_views += n_views;
    if (!counts) return SL3D_OK;  // (the next call's copy into the table is ordered behind this kernel on the stream)
    unsigned long long w[2];
    HIPCHK(x, hipMemcpyAsync(w, x->d_tsdf_words + TSDF_WORD_SAMPLES, sizeof w, hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    counts[0] = (int64_t)w[0], counts[1] = (int64_t)w[1];
    return SL3D_OK;
}
SL3D_CATCH(x)

// the surface arrays for m crossings (> 0)
static int ensure_tsdf_surface(sl3d_ctx *x, size_t m)
{
    int rc = grow_plane(x, &x->d_tsdf_xyz, &x->tsdf_cap[TSDF_XYZ], 3 * m);
    if (!rc) rc = grow_plane(x, &x->d_tsdf_nrm, &x->tsdf_cap[TSDF_NRM], 3 * m);
    if (!rc) rc = grow_plane(x, &x->d_tsdf_edge, &x->tsdf_cap[TSDF_EDGE], m);
    return rc;
}

// k_tsdf_count and k_compact_scan, the download of the total (the surface arrays are sized by it: the call synchronises), k_tsdf_scatter
extern "C" int sl3d_tsdf_extract(sl3d_ctx *x, int64_t min_weight, sl3d_tsdf_surface *device_out, int64_t counts[3])
try {
    if (!x) return fail(x, SL3D_E_INVALID_ARG, "tsdf_extract: null context");
    if (min_weight < 1) return fail(x, SL3D_E_INVALID_ARG, "tsdf_extract: min_weight must be >= 1");
    if (!x->tsdf_dims[0]) return fail(x, SL3D_E_STATE, "tsdf_extract: no sl3d_tsdf_reset has defined a volume");
    ON_DEVICE(x);
    const TsdfVolume vol = tsdf_volume(x);
    const int64_t n = tsdf_voxels(x->tsdf_dims);
    const size_t nb = (size_t)((n + 1023) / 1024);
    x->tsdf_m = -1;  // (from here on the last surface is gone)
    int rc = grow_plane(x, &x->tsdf_s.cnt, &x->tsdf_cap[TSDF_CNT], nb);
    if (!rc) rc = grow_plane(x, &x->tsdf_s.off, &x->tsdf_cap[TSDF_OFF], nb);
    if (rc) return rc;
    const TsdfPlanes planes = {x->d_tsdf_sum, x->d_tsdf_weight, (unsigned long long)min_weight};
    rc = launched(x, launch_tsdf_count(planes, vol, x->tsdf_s, x->d_tsdf_words, x->stream));
    if (rc) return rc;
    unsigned long long w[2];
    HIPCHK(x, hipMemcpyAsync(w, x->d_tsdf_words + TSDF_WORD_KNOWN, sizeof w, hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    const int64_t m = (int64_t)w[1];
    if (m > 0) {
        rc = ensure_tsdf_surface(x, (size_t)m);
        if (!rc) rc = launched(x, launch_tsdf_scatter(planes, vol, x->tsdf_s, x->d_tsdf_xyz, x->d_tsdf_nrm, x->d_tsdf_edge, x->stream));
        if (rc) return rc;
    }
    x->tsdf_m = m;
    if (device_out) *device_out = sl3d_tsdf_surface{m ? x->d_tsdf_xyz : nullptr, m ? x->d_tsdf_nrm : nullptr, m ? x->d_tsdf_edge : nullptr};
    if (counts) counts[0] = n, counts[1] = (int64_t)w[0], counts[2] = m;
    return SL3D_OK;
}
SL3D_CATCH(x)

// the planes of the volume: size then fill
extern "C" int sl3d_get_tsdf(sl3d_ctx *x, int32_t *sum, uint32_t *weight, int64_t capacity, int64_t *n)
try {
    if (!x || !n || capacity < 0) return fail(x, SL3D_E_INVALID_ARG, "get_tsdf: null argument or capacity < 0");
    if (!x->tsdf_dims[0]) return fail(x, SL3D_E_STATE, "get_tsdf: no sl3d_tsdf_reset has defined a volume");
    ON_DEVICE(x);
    const int64_t total = tsdf_voxels(x->tsdf_dims), m = total < capacity ? total : capacity;
    if (m > 0) {
        if (sum) HIPCHK_DRAIN(x, hipMemcpyAsync(sum, x->d_tsdf_sum, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
        if (weight) HIPCHK_DRAIN(x, hipMemcpyAsync(weight, x->d_tsdf_weight, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    }
    SYNC_FOR_CALLER(x);
    *n = total;
    return SL3D_OK;
}
SL3D_CATCH(x)

// the surface the last sl3d_tsdf_extract left: size then fill
extern "C" int sl3d_get_tsdf_surface(sl3d_ctx *x, float *xyz, float *normals, int32_t *edge, int64_t capacity, int64_t *n)
try {
    if (!x || !n || capacity < 0) return fail(x, SL3D_E_INVALID_ARG, "get_tsdf_surface: null argument or capacity < 0");
    if (x->tsdf_m < 0) return fail(x, SL3D_E_STATE, "get_tsdf_surface: no sl3d_tsdf_extract has run since the last sl3d_tsdf_reset");
    ON_DEVICE(x);
    const int64_t total = x->tsdf_m, m = total < capacity ? total : capacity;
    if (m > 0) {
        if (xyz) HIPCHK_DRAIN(x, hipMemcpyAsync(xyz, x->d_tsdf_xyz, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        if (normals) HIPCHK_DRAIN(x, hipMemcpyAsync(normals, x->d_tsdf_nrm, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        if (edge) HIPCHK_DRAIN(x, hipMemcpyAsync(edge, x->d_tsdf_edge, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
    }
    SYNC_FOR_CALLER(x);
    *n = total;
    return SL3D_OK;
}
SL3D_CATCH(x)
