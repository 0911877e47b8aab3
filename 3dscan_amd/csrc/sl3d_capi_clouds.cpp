// sl3d_capi_clouds.cpp -- O1 / N2 / N3: ordered clouds straight from the fused kernel (segmented), their consumers (contiguous copy, host
// downloads, registration), the compaction of a dense result with colour, turntable registration, the mesh over a dense result.
// Device side: sl3d_clouds.hip (sl3d_mesh.hip for the faces and the cell pass, sl3d_mesh_normals.hip for the normals,
// sl3d_mesh_components.hip for the components, sl3d_mesh_smooth.hip for the smoothing, sl3d_mesh_lod.hip for the level-of-detail mesh, sl3d_mesh_holes.hip for the hole filling).  Every consumer of a dense result keeps its
// counts, their scan and the totals in a CompactScratch: ensure_scratch (sl3d_capi_internal.h) allocates one, ensure_plane a plane
// beside it, read_totals brings its totals to the host.
#include "sl3d_capi_internal.h"
#include "sl3d_mesh_lod.h"  // LOD_MAX_STEP

typedef sl3d_ctx::Scan Scan;

// ---- compacted clouds straight from the fused kernel ----------------------------------------------------------------
static int ensure_cloud_buffers(sl3d_ctx *x)
{
    // one flag, set at the very end: a set-up that failed half way (out of memory on a later buffer) is retried by the next
    // call instead of being mistaken for a finished one (every step below skips what an earlier attempt already allocated)
    if (x->clouds_ready) return SL3D_OK;
    KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views;
    int rc = SL3D_OK;
    if (!x->d_clouds) rc = dev_alloc(x, &x->d_clouds, mv * P.px_view_stride * 3);
    if (!rc) rc = ensure_scratch(x, x->blk_all, mv * compact_blocks(P), mv);
    if (rc) return rc;
    P.n_tiles = fused_tiles(P);
    P.n_segs = 4 * P.n_tiles;
    if (!x->d_seg_counts) rc = dev_alloc(x, &x->d_seg_counts, mv * (size_t)P.n_segs);
    if (!rc && !x->d_seg_offsets) rc = dev_alloc(x, &x->d_seg_offsets, mv * (size_t)P.n_segs);
    if (rc) return rc;
    // a wave of the last tile that owns no row never stores its count: zero once, for good
    HIPCHK(x, hipMemsetAsync(x->d_seg_counts, 0, mv * (size_t)P.n_segs * sizeof(unsigned), x->stream));
    HIPCHK(x, hipMemsetAsync(x->d_seg_offsets, 0, mv * (size_t)P.n_segs * sizeof(unsigned long long), x->stream));
    P.seg_counts = x->d_seg_counts;
    P.seg_offsets = x->d_seg_offsets;
    P.clouds = x->d_clouds;
    // the per-view counts live in pinned HOST memory the scan kernel writes directly (one 8-byte store per view):
    // sl3d_get_cloud_counts then only has to wait for the stream, no device-to-host copy in the launch -> counts path
    if (!x->h_counts) {
        HIPCHK(x, hipHostMalloc((void **)&x->h_counts, mv * sizeof(unsigned long long), hipHostMallocMapped));
        memset(x->h_counts, 0, mv * sizeof(unsigned long long));
    }
    void *mapped = nullptr;
    HIPCHK(x, hipHostGetDevicePointer(&mapped, x->h_counts, 0));
    P.cloud_totals = (unsigned long long *)mapped;
    x->scan_state.assign(mv, Scan::DONE);
    x->clouds_ready = true;
    return SL3D_OK;
}

// The fused kernel with the compaction of 8/save_point_cloud.cpp:85-104 inside it (k_fused<..., CMODE = 2>: segmented ordered
// clouds): one launch reads every frame byte once and writes the valid map and the compacted points of every view -- no dense xyz
// plane, no second pass over the results -- then one small scan launch turns the segment counts into offsets and totals.
extern "C" int sl3d_run_clouds(sl3d_ctx *x, int first_view, int n_views)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!x->have_cal) return fail(x, SL3D_E_STATE, "sl3d_set_calibration has not been called");
    if (x->keep) return fail(x, SL3D_E_STATE, "sl3d_run_clouds is the timed mode: create the context without SL3D_FLAG_KEEP_STAGES");
    if (x->subpixel) return fail(x, SL3D_E_UNSUPPORTED, "sl3d_run_clouds has no sub-pixel form (SL3D_FLAG_SUBPIXEL): use sl3d_run + sl3d_compact_views");
    if (x->repair) return fail(x, SL3D_E_UNSUPPORTED, "sl3d_run_clouds has no period-repaired form (SL3D_FLAG_REPAIR_PERIODS): use sl3d_run + sl3d_compact_views");
    ON_DEVICE_QUIET(x);
    // (a small launch goes beside the one before it, sl3d_ctx.h: launch lanes -- once the cloud buffers exist; its consumers join)
    bool overlap = false;
    if (x->lanes_ok && x->clouds_ready && n_views <= LanePolicy::MAX_VIEWS) rc = small_launch_overlaps(x, first_view, n_views, &overlap);
    else rc = sl3d_lanes_join(x);
    if (rc) return rc;
    rc = ensure_cloud_buffers(x);
    if (rc) return rc;
    rc = run_fused(x, first_view, n_views, false, 2, overlap);
    if (rc) return rc;
    // A launch of a few views (the reference's one scan per call) leaves the scan of the segment counts to whoever consumes the
    // clouds: the gap-closing kernel adds up the counts in front of its segments itself, so there is no scan launch -- 4.8 us + a
    // kernel boundary behind a 26-us kernel -- between the fused kernel and its consumer; a consumer that wants the offsets as an
    // array (sl3d_get_cloud_segments) gets the scan then.  Large launches scan here, as before: one launch for all views.
    if (n_views <= SL3D_SMALL_LAUNCH_VIEWS) {
        std::fill_n(x->scan_state.begin() + first_view, n_views, Scan::PENDING);
        return SL3D_OK;
    }
    std::fill_n(x->scan_state.begin() + first_view, n_views, Scan::DONE);
    return launched(x, launch_seg_scan(x->P, first_view, n_views, x->stream));
}
SL3D_CATCH(x)

// offsets and totals of views [first_view, first_view + n_views) are (being) computed: k_seg_scan for the views that still lack them
static int ensure_scanned(sl3d_ctx *x, int first_view, int n_views)
{
    for (int v = first_view; v < first_view + n_views;) {
        if (x->scan_state[v] == Scan::DONE) { v++; continue; }
        int e = v;
        while (e < first_view + n_views && x->scan_state[e] != Scan::DONE) x->scan_state[e++] = Scan::DONE;
        const int rc = launched(x, launch_seg_scan(x->P, v, e - v, x->stream));
        if (rc) return rc;
        v = e;
    }
    return SL3D_OK;
}

static int ensure_packed(sl3d_ctx *x)
{
    if (x->d_packed) return SL3D_OK;
    return dev_alloc(x, &x->d_packed, (size_t)x->cfg.max_views * x->P.px_view_stride * 3);
}

// a scanning consumer (k_seg_close<.., SCAN>) over these views has drained: their totals, and what that leaves of their scan state
static void read_scanned_totals(sl3d_ctx *x, int first_view, int n_views, int64_t *counts)
{
    for (int v = first_view; v < first_view + n_views; v++) {
        counts[v - first_view] = x->cloud_total(v);
        if (x->scan_state[v] == Scan::PENDING) x->scan_state[v] = Scan::TOTAL_ONLY;
    }
}

// where a kernel may store straight into the caller's host buffer (pinned memory mapped into the device), or NULL: pageable memory, or
// SL3D_ZEROCOPY=0 in the environment
static float *mapped_destination(float *xyz)
{
    void *mapped = nullptr;
    const char *zc = getenv("SL3D_ZEROCOPY");
    if (!(zc && atoi(zc) == 0) && is_pinned_host(xyz) && hipHostGetDevicePointer(&mapped, xyz, 0) == hipSuccess && mapped) return (float *)mapped;
    (void)hipGetLastError();
    return nullptr;
}

// Host copy of per-view device arrays of `elem`-byte elements (12: points, faces, normals; 4: labels, ids), `stride` elements apart, back
// to back: view v's first counts[v] elements, at most `capacity` in all (negative or used up: nothing more is copied; the counts stay the
// caller's to report in full).  host == NULL: nothing.  Enqueued only -- the caller synchronises
static int download_clamped(sl3d_ctx *x, void *host, const void *dev, size_t stride, int n_views, const int64_t *counts, int64_t capacity,
                            size_t elem = 12)
{
    int64_t off = 0;
    for (int v = 0; v < n_views && host; v++) {
        const int64_t n = std::min<int64_t>(counts[v], capacity - off);
        if (n <= 0) continue;
        HIPCHK_DRAIN(x, hipMemcpyAsync((char *)host + elem * off, (const char *)dev + elem * (size_t)v * stride, (size_t)n * elem, hipMemcpyDeviceToHost, x->stream));
        off += n;
    }
    return SL3D_OK;
}

// The totals a launch over views [first_view, first_view + n_views) left in tot (k per view: tot[k * v + j]) reach the host: word 0 of
// view first_view + v widened into n0[v], word 1 (k == 2) into n1[v].  Synchronises for the caller
static int read_totals(sl3d_ctx *x, const unsigned long long *tot, int k, int first_view, int n_views, int64_t *n0, int64_t *n1 = nullptr)
{
    std::vector<unsigned long long> t((size_t)k * (size_t)n_views);
    HIPCHK(x, hipMemcpyAsync(t.data(), tot + (size_t)k * first_view, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    for (int v = 0; v < n_views; v++) {
        n0[v] = (int64_t)t[(size_t)k * v];
        if (n1) n1[v] = (int64_t)t[(size_t)k * v + 1];
    }
    return SL3D_OK;
}

// counts (and the device address) of the clouds the last sl3d_run_clouds over these views produced; synchronises
extern "C" int sl3d_get_cloud_counts(sl3d_ctx *x, int first_view, int n_views, const float **device_xyz, size_t *view_stride_points, int64_t *counts)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!counts) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (!x->clouds_ready) return fail(x, SL3D_E_STATE, "sl3d_run_clouds has not been called");
    ON_DEVICE(x);
    bool unscanned = false, no_total = false;
    for (int v = first_view; v < first_view + n_views; v++) {
        unscanned |= x->scan_state[v] != Scan::DONE;
        no_total |= x->scan_state[v] == Scan::PENDING;
    }
    // unscanned views whose contiguous copy is wanted: the gap-closing kernel that makes it scans on entry and leaves the totals too --
    // ONE launch, one wait.  Otherwise the counts first: the scan kernel (or a scanning consumer) stored them into pinned host memory itself
    const bool scan_on_entry = device_xyz && unscanned;
    if (!scan_on_entry) {
        if (no_total && (rc = ensure_scanned(x, first_view, n_views))) return rc;
        SYNC_FOR_CALLER(x);
        for (int v = 0; v < n_views; v++) counts[v] = x->cloud_total(first_view + v);
    }
    if (device_xyz) {  // the contiguous copy is made now, by one gap-closing launch over these views
        rc = ensure_packed(x);
        if (rc) return rc;
        float *dst = x->d_packed + 3 * (size_t)first_view * x->P.px_view_stride;
        rc = launched(x, launch_seg_close(x->P, first_view, n_views, SegClose{dst, x->P.px_view_stride, scan_on_entry, ~0ull}, x->stream));
        if (rc) return rc;
        // the copy is handed to consumers on OTHER streams too (a group's communication stream, a caller's RCCL stream):
        // like the counts, it is complete when this call returns
        SYNC_FOR_CALLER(x);
        if (scan_on_entry) read_scanned_totals(x, first_view, n_views, counts);
        *device_xyz = dst;
    }
    if (view_stride_points) *view_stride_points = x->P.px_view_stride;
    return SL3D_OK;
}
SL3D_CATCH(x)

extern "C" int sl3d_get_cloud_segments(sl3d_ctx *x, int first_view, int n_views, sl3d_cloud_segments *out, int64_t *counts)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!out) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (!x->clouds_ready) return fail(x, SL3D_E_STATE, "sl3d_run_clouds has not been called");
    {   // this consumer wants the offsets as an array: the scan runs now if the launch left it out
        ON_DEVICE(x);
        rc = ensure_scanned(x, first_view, n_views);
        if (rc) return rc;
    }
    if (counts) {
        rc = sl3d_get_cloud_counts(x, first_view, n_views, nullptr, nullptr, counts);
        if (rc) return rc;
    }
    const KParams &P = x->P;
    out->xyz = x->d_clouds + 3 * (size_t)first_view * P.px_view_stride;
    out->counts = x->d_seg_counts + (size_t)first_view * P.n_segs;
    out->offsets = (const uint64_t *)(x->d_seg_offsets + (size_t)first_view * P.n_segs);
    out->n_segments = P.n_segs;
    out->segment_points = SL3D_SEG_POINTS;
    out->view_stride_points = P.px_view_stride;
    out->view_stride_segments = (size_t)P.n_segs;
    return SL3D_OK;
}
SL3D_CATCH(x)

// The host copy of the clouds of the last sl3d_run_clouds, back to back (8/save_point_cloud.cpp:85-104 fills a host cloud).
// Segmented clouds + pinned destination: the gap-closing kernel stores straight into the (mapped) host buffer -- the PCIe link is
// the bound either way, so closing the gaps costs nothing; pageable destination: a contiguous device copy goes down by DMA.
extern "C" int sl3d_download_clouds(sl3d_ctx *x, int first_view, int n_views, float *xyz, int64_t capacity, int64_t *counts)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!counts) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (!x->clouds_ready) return fail(x, SL3D_E_STATE, "sl3d_run_clouds has not been called");
    if (n_views == 1 && xyz && capacity > 0 && x->scan_state[first_view] != Scan::DONE) {
        // ONE unscanned view into pinned host memory -- the reference's own consumer (8/save_point_cloud.cpp:85-104 fills a host cloud
        // per scan): the gap-closing kernel scans on entry, stores straight into the mapped host buffer (clamped to its capacity)
        // and leaves the count -- fused kernel, this kernel, one wait; no scan launch, no wait for the count in between
        ON_DEVICE(x);
        if (float *mapped = mapped_destination(xyz)) {
            rc = launched(x, launch_seg_close(x->P, first_view, 1, SegClose{mapped, 0, true, (unsigned long long)capacity}, x->stream));
            if (rc) return rc;
            SYNC_FOR_CALLER(x);
            read_scanned_totals(x, first_view, 1, counts);
            return SL3D_OK;
        }
    }
    rc = sl3d_get_cloud_counts(x, first_view, n_views, nullptr, nullptr, counts);
    if (rc || !xyz) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    int64_t total = 0;
    for (int v = 0; v < n_views; v++) total += counts[v];
    if (float *mapped = total <= capacity ? mapped_destination(xyz) : nullptr) {
        rc = ensure_scanned(x, first_view, n_views);  // (k_seg_close reads the offsets array)
        if (rc) return rc;
        int64_t off = 0;
        for (int v = 0; v < n_views; v++) {
            if (counts[v] > 0) {
                rc = launched(x, launch_seg_close(P, first_view + v, 1, SegClose{mapped + 3 * off, 0}, x->stream));
                if (rc) return rc;
            }
            off += counts[v];
        }
    } else {
        const float *dev = nullptr;
        size_t stride = 0;
        rc = sl3d_get_cloud_counts(x, first_view, n_views, &dev, &stride, counts);
        if (rc || (rc = download_clamped(x, xyz, dev, stride, n_views, counts, capacity))) return rc;
    }
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

extern "C" int sl3d_compact(sl3d_ctx *x, int view, const float **device_xyz, int64_t *count)
try {
    int rc = check_view(x, view);
    if (rc) return rc;
    if (!count) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    ON_DEVICE(x);
    const bool tex = x->d_texture && view < (int)x->have_texture.size() && x->have_texture[view];
    rc = launched(x, launch_compact_views(x->P, view, 1, x->blk_one, x->d_cloud, tex ? x->d_texture + (size_t)view * x->P.px_view_stride * 3 : nullptr,
                                          x->d_cloud_rgb, x->stream));
    if (rc) return rc;
    rc = read_totals(x, x->blk_one.tot, 1, view, 1, count);
    if (rc) return rc;
    if (device_xyz) *device_xyz = x->d_cloud;
    return SL3D_OK;
}
SL3D_CATCH(x)

// sl3d_get_cloud / sl3d_get_cloud_rgb behind their argument checks: the row-major scan over the valid pixels only (8/save_point_cloud.cpp:
// 85-104), compacted on the device; at most `capacity` points (and their r,g,b) reach the host
static int get_compacted(sl3d_ctx *x, int view, float *xyz, uint8_t *rgb, int64_t capacity, int64_t *count)
{
    ON_DEVICE(x);
    const float *dev = nullptr;
    int rc = sl3d_compact(x, view, &dev, count);
    if (rc) return rc;
    const int64_t n = *count < capacity ? *count : capacity;
    if (n > 0 && (xyz || rgb)) {
        if (xyz) HIPCHK(x, hipMemcpyAsync(xyz, dev, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        if (rgb) HIPCHK_DRAIN(x, hipMemcpyAsync(rgb, x->d_cloud_rgb, (size_t)n * 3, hipMemcpyDeviceToHost, x->stream));
        SYNC_FOR_CALLER(x);
    }
    return SL3D_OK;
}

extern "C" int sl3d_get_cloud(sl3d_ctx *x, int view, float *xyz, int64_t capacity, int64_t *count)
try {
    if (!x || !count) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    return get_compacted(x, view, xyz, nullptr, capacity, count);
}
SL3D_CATCH(x)

// The compaction of a whole batch of views in three launches and one read-back: what a pipeline that goes from
// device-resident frames to compacted clouds runs after sl3d_run (bench.py reports it as `to_compacted_clouds`).
extern "C" int sl3d_compact_views(sl3d_ctx *x, int first_view, int n_views, const float **device_xyz, size_t *view_stride_points, int64_t *counts)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!counts) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    ON_DEVICE(x);
    const KParams &P = x->P;
    rc = ensure_cloud_buffers(x);
    if (rc) return rc;
    rc = ensure_packed(x);  // (the region sl3d_run_clouds writes is left alone)
    if (rc) return rc;
    rc = launched(x, launch_compact_views(P, first_view, n_views, x->blk_all, x->d_packed + 3 * (size_t)first_view * P.px_view_stride, nullptr, nullptr,
                                          x->stream));
    if (rc) return rc;
    rc = read_totals(x, x->blk_all.tot, 1, first_view, n_views, counts);
    if (rc) return rc;
    if (device_xyz) *device_xyz = x->d_packed + 3 * (size_t)first_view * P.px_view_stride;
    if (view_stride_points) *view_stride_points = P.px_view_stride;
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy of the batched compaction: the clouds of the views back to back in xyz (at most `capacity` points in all)
extern "C" int sl3d_get_clouds(sl3d_ctx *x, int first_view, int n_views, float *xyz, int64_t capacity, int64_t *counts)
try {
    if (!x) return SL3D_E_INVALID_ARG;
    ON_DEVICE(x);
    const float *dev = nullptr;
    size_t stride = 0;
    int rc = sl3d_compact_views(x, first_view, n_views, &dev, &stride, counts);
    if (rc || (rc = download_clamped(x, xyz, dev, stride, n_views, counts, capacity))) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// the colour image save_point_cloud() takes the r,g,b of every valid pixel from (8/save_point_cloud.cpp:46-52: cvLoadImage
// of Point_cloud/texture.bmp, split into blue / green / red planes)
extern "C" int sl3d_set_texture(sl3d_ctx *x, int view, const uint8_t *bgr, size_t stride)
try {
    int rc = check_view(x, view);
    if (rc) return rc;
    const KParams &P = x->P;
    if (!bgr || stride < (size_t)P.W * 3) return fail(x, SL3D_E_INVALID_ARG, "texture: null or stride < 3*width");
    ON_DEVICE(x);
    if (!x->d_texture) {
        rc = dev_alloc(x, &x->d_texture, (size_t)x->cfg.max_views * P.px_view_stride * 3);
        if (rc) return rc;
        rc = dev_alloc(x, &x->d_cloud_rgb, P.px_view_stride * 3);
        if (rc) return rc;
        x->have_texture.assign((size_t)x->cfg.max_views, 0);
    }
    SYNC_FOR_CALLER(x);
    HIPCHK(x, hipMemcpy2D(x->d_texture + (size_t)view * P.px_view_stride * 3, (size_t)P.pitch * 3, bgr, stride, (size_t)P.W * 3, (size_t)P.H,
                          hipMemcpyHostToDevice));
    x->have_texture[view] = 1;
    return SL3D_OK;
}
SL3D_CATCH(x)

extern "C" int sl3d_get_cloud_rgb(sl3d_ctx *x, int view, float *xyz, uint8_t *rgb, int64_t capacity, int64_t *count)
try {
    if (!x || !count) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (!x->d_texture || view < 0 || view >= (int)x->have_texture.size() || !x->have_texture[view])
        return fail(x, SL3D_E_INVALID_ARG, "no texture set for this view (sl3d_set_texture)");
    return get_compacted(x, view, xyz, rgb, capacity, count);
}
SL3D_CATCH(x)

// ---- N3: register_point_clouds(), 9/register_point_clouds.cpp:23-155, without the PLY files ---------------------------------------
static int ensure_reg(sl3d_ctx *x)
{
    if (x->d_reg) return SL3D_OK;
    return dev_alloc(x, &x->d_reg, (size_t)x->cfg.max_views * x->P.px_view_stride * 3);
}

// The loop over the views (:83-145): view k, of counts[k] points, is rotated about Y by theta_k around (tx,ty,tz) into d_reg behind the
// views in front of it -- launch_view(k, counts[k], its place in d_reg, R4) enqueues that; theta_0 = 0, theta_{k+1} = theta_k + rot_step
// in float (:145).  *total: the points of all views.  No host sync between the launches
template <typename LaunchView>
static int register_each(sl3d_ctx *x, int n_views, const int64_t *counts, float rot_step, int64_t *total, LaunchView launch_view)
{
    float theta = 0.0f;
    *total = 0;
    for (int k = 0; k < n_views; k++) {
        float R4[4];
        turntable_R4(theta, R4);
        const int rc = launched(x, launch_view(k, counts[k], x->d_reg + 3 * *total, R4));
        if (rc) return rc;
        *total += counts[k];
        theta += rot_step;
    }
    return SL3D_OK;
}

// the clouds are the compacted clouds of the resident views' dense results: one batched compaction (three launches, one read-back), then
// one transform launch per view
extern "C" int sl3d_register_views(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float *xyz,
                                   int64_t capacity, int64_t *total)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!total) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    ON_DEVICE(x);
    rc = ensure_reg(x);
    if (rc) return rc;
    std::vector<int64_t> counts((size_t)n_views);
    const float *clouds = nullptr;
    size_t stride = 0;
    rc = sl3d_compact_views(x, first_view, n_views, &clouds, &stride, counts.data());
    if (rc) return rc;
    int64_t off = 0;
    rc = register_each(x, n_views, counts.data(), rot_step, &off, [&](int k, int64_t n, float *out, const float *R4) {
        return launch_register(clouds + 3 * (size_t)k * stride, out, (long)n, R4, tx, ty, tz, x->stream);
    });
    if (rc) return rc;
    x->reg_total = off;  // (sl3d_voxel_grid over the registered cloud)
    SYNC_FOR_CALLER(x);
    *total = off;
    const int64_t m = off < capacity ? off : capacity;
    if (xyz && m > 0) {
        HIPCHK(x, hipMemcpyAsync(xyz, x->d_reg, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        SYNC_FOR_CALLER(x);
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// register_point_clouds() on the clouds of the last sl3d_run_clouds: the segments of view k are rotated by theta_k while they are
// concatenated (k_seg_close<REG>), so neither a dense plane nor a separate compaction nor a gap-closing pass is needed.
extern "C" int sl3d_register_clouds(sl3d_ctx *x, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float *xyz,
                                    int64_t capacity, int64_t *total)
try {
    int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!total) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    std::vector<int64_t> counts((size_t)n_views);
    if (!x->clouds_ready) return fail(x, SL3D_E_STATE, "sl3d_run_clouds has not been called");
    {   // (k_seg_close<REG> reads the offsets array: the scan runs now if the launch left it out)
        ON_DEVICE(x);
        rc = ensure_scanned(x, first_view, n_views);
        if (rc) return rc;
    }
    rc = sl3d_get_cloud_counts(x, first_view, n_views, nullptr, nullptr, counts.data());
    if (rc) return rc;
    ON_DEVICE(x);
    rc = ensure_reg(x);
    if (rc) return rc;
    int64_t off = 0;
    rc = register_each(x, n_views, counts.data(), rot_step, &off, [&](int k, int64_t n, float *out, const float *R4) {
        return n > 0 ? launch_seg_close(x->P, first_view + k, 1, SegClose{out, 0, false, 0, R4, tx, ty, tz}, x->stream) : 0;
    });
    if (rc) return rc;
    x->reg_total = off;
    *total = off;
    const int64_t m = off < capacity ? off : capacity;
    if (xyz && m > 0) HIPCHK(x, hipMemcpyAsync(xyz, x->d_reg, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- the mesh over a dense result (sl3d_mesh.h: the definition; sl3d_mesh.hip: the kernels) ---------------------------------------
static int ensure_mesh_buffers(sl3d_ctx *x)
{
    if (x->mesh_ready) return SL3D_OK;  // (one flag, set at the very end: ensure_cloud_buffers)
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views;
    x->mesh_face_stride = mesh_face_stride(P);
    int rc = ensure_scratch(x, x->chk_mesh, mv * 2 * (size_t)mesh_chunks(P), mv * 2);
    if (!rc) rc = ensure_scratch(x, x->blk_mesh, mv * compact_blocks(P), mv);
    if (!rc) rc = ensure_plane(x, &x->d_mesh_xyz, mv * P.px_view_stride * 3);
    if (!rc) rc = ensure_plane(x, &x->d_mesh_faces, mv * x->mesh_face_stride * 3);
    if (rc) return rc;
    x->mesh_ready = true;
    return SL3D_OK;
}

// (n_faces: a call without face counts passes n_vertices twice)
static int check_mesh_args(sl3d_ctx *x, int first_view, int n_views, float max_edge, const int64_t *n_vertices, const int64_t *n_faces)
{
    const int rc = check_view(x, first_view, n_views);
    if (rc) return rc;
    if (!n_vertices || !n_faces) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (!(max_edge > 0.0f)) return fail(x, SL3D_E_INVALID_ARG, "max_edge must be > 0 (+inf: no edge-length test)");
    return SL3D_OK;
}

// Vertices: the batched compaction as it stands, into the mesh's own cloud buffer.  Faces: count, scan (k_compact_scan over the 2
// count arrays of every view), emit.  Six launches, one read-back of the 2 totals per view.
extern "C" int sl3d_mesh_views(sl3d_ctx *x, int first_view, int n_views, float max_edge, sl3d_mesh *device_mesh, int64_t *n_vertices,
                               int64_t *n_faces)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    rc = ensure_mesh_buffers(x);
    if (rc) return rc;
    float *xyz = x->d_mesh_xyz + 3 * (size_t)first_view * P.px_view_stride;
    rc = launched(x, launch_compact_views(P, first_view, n_views, x->blk_mesh, xyz, nullptr, nullptr, x->stream));
    if (rc) return rc;
    rc = launched(x, launch_mesh_views(P, first_view, n_views, max_edge, x->chk_mesh, x->d_mesh_faces, x->mesh_face_stride, x->stream));
    if (!rc) rc = read_totals(x, x->chk_mesh.tot, 2, first_view, n_views, n_vertices, n_faces);
    if (rc) return rc;
    if (device_mesh) {
        device_mesh->xyz = xyz;
        device_mesh->faces = x->d_mesh_faces + 3 * (size_t)first_view * x->mesh_face_stride;
        device_mesh->view_stride_points = P.px_view_stride;
        device_mesh->view_stride_faces = x->mesh_face_stride;
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: the clouds of the views back to back in xyz, their faces back to back in faces (ids relative to the view's own cloud)
extern "C" int sl3d_get_meshes(sl3d_ctx *x, int first_view, int n_views, float max_edge, float *xyz, int64_t vertex_capacity, int32_t *faces,
                               int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    sl3d_mesh m;
    rc = sl3d_mesh_views(x, first_view, n_views, max_edge, &m, n_vertices, n_faces);
    if (rc) return rc;
    rc = download_clamped(x, xyz, m.xyz, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, faces, m.faces, m.view_stride_faces, n_views, n_faces, face_capacity);
    if (rc) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- vertex normals of those meshes (sl3d_mesh.h: the definition; sl3d_mesh_normals.hip: the kernels) -----------------------------
static int ensure_normal_buffers(sl3d_ctx *x)
{
    if (x->normals_ready) return SL3D_OK;  // (one flag, set at the very end: ensure_cloud_buffers)
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views;
    int rc = ensure_scratch(x, x->chk_nrm, mv * (size_t)mesh_chunks(P), mv);
    if (!rc) rc = ensure_plane(x, &x->d_normals, mv * P.px_view_stride * 3);
    if (rc) return rc;
    x->normals_ready = true;
    return SL3D_OK;
}

// Count, scan (k_compact_scan over the count array of every view), gather: three launches, one read-back of the total per view.  Reads the
// dense result only: nothing the mesh call or the compactions handed out is touched.
extern "C" int sl3d_mesh_normals(sl3d_ctx *x, int first_view, int n_views, float max_edge, const float **device_normals, size_t *view_stride_points,
                                 int64_t *n_vertices)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_vertices);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    rc = ensure_normal_buffers(x);
    if (rc) return rc;
    rc = launched(x, launch_mesh_normals(P, first_view, n_views, max_edge, x->chk_nrm, x->d_normals, P.px_view_stride, x->stream));
    if (!rc) rc = read_totals(x, x->chk_nrm.tot, 1, first_view, n_views, n_vertices);
    if (rc) return rc;
    if (device_normals) *device_normals = x->d_normals + 3 * (size_t)first_view * P.px_view_stride;
    if (view_stride_points) *view_stride_points = P.px_view_stride;
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: the normals of the views back to back
extern "C" int sl3d_get_mesh_normals(sl3d_ctx *x, int first_view, int n_views, float max_edge, float *normals, int64_t vertex_capacity,
                                     int64_t *n_vertices)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_vertices);
    if (rc) return rc;
    ON_DEVICE(x);
    const float *dev = nullptr;
    size_t stride = 0;
    rc = sl3d_mesh_normals(x, first_view, n_views, max_edge, &dev, &stride, n_vertices);
    if (rc || (rc = download_clamped(x, normals, dev, stride, n_views, n_vertices, vertex_capacity))) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- connected components of those meshes, and the meshes without the small ones (sl3d_mesh_components.h: the definition and the
// union-find; sl3d_mesh_components.hip: the kernels) -----------------------------------------------------------------------------------
static int ensure_cc_buffers(sl3d_ctx *x)
{
    if (x->cc_ready) return SL3D_OK;  // (one flag, set at the very end: ensure_cloud_buffers)
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views, px = mv * P.px_view_stride;
    CcBuffers &b = x->cc;
    int rc = ensure_plane(x, &b.cells, px);
    if (!rc) rc = ensure_plane(x, &b.labels, px);
    if (!rc) rc = ensure_plane(x, &b.vid, px);
    if (!rc) rc = ensure_plane(x, &b.sizes, px);
    if (!rc) rc = ensure_plane(x, &x->d_cc_labels, px);
    // (the totals: the whole CcTotals array, whose first part is this scratch's)
    if (!rc) rc = ensure_scratch(x, b.s, mv * (size_t)mesh_chunks(P), CcTotals{nullptr, mv}.words());
    if (rc) return rc;
    b.stat = CcTotals{b.s.tot, mv}.stat(0);
    x->cc_ready = true;
    return SL3D_OK;
}

// (behind ensure_cc_buffers: the filter's totals are the `kept` part of the components' CcTotals array, so that a call reads both back at once)
static int ensure_ccf_buffers(sl3d_ctx *x)
{
    if (x->ccf_ready) return SL3D_OK;
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views, px = mv * P.px_view_stride;
    CcFiltered &f = x->ccf;
    if (!x->cc_ready) return fail(x, SL3D_E_INTERNAL, "the filter's buffers are set up behind the components'");
    f.face_stride = mesh_face_stride(P);
    f.s.tot = CcTotals{x->cc.s.tot, mv}.kept(0);  // (set: ensure_scratch allocates no totals of its own)
    int rc = ensure_plane(x, &f.keep, px);
    if (!rc) rc = ensure_scratch(x, f.s, mv * 2 * (size_t)mesh_chunks(P), 0);
    if (!rc) rc = ensure_plane(x, &f.xyz, 3 * px);
    if (!rc) rc = ensure_plane(x, &f.ids, px);
    if (!rc) rc = ensure_plane(x, &f.faces, mv * f.face_stride * 3);
    if (rc) return rc;
    x->ccf_ready = true;
    return SL3D_OK;
}

// The one read-back of a components or filter call: the CcTotals array whole, t: its host copy.  A failure word set by a kernel -- an
// iteration bound ran out: a logic error -- ends the call as SL3D_E_INTERNAL.  Synchronises for the caller
static int read_cc_totals(sl3d_ctx *x, int first_view, int n_views, std::vector<unsigned long long> &words, CcTotals &t)
{
    words.resize(CcTotals{nullptr, (size_t)x->cfg.max_views}.words());
    t = CcTotals{words.data(), (size_t)x->cfg.max_views};
    HIPCHK(x, hipMemcpyAsync(words.data(), x->cc.s.tot, sizeof(unsigned long long) * words.size(), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    for (int v = first_view; v < first_view + n_views; v++)
        if (t.stat(v)[1])
            return fail(x, SL3D_E_INTERNAL, "mesh components: a label walk of view " + std::to_string(v) + " ran out of its iteration bound");
    return SL3D_OK;
}

// Five launches (cells, scan, union, flatten, labels), one read-back.  Reads the dense result only and writes buffers of its own.
extern "C" int sl3d_mesh_components(sl3d_ctx *x, int first_view, int n_views, float max_edge, const int32_t **device_labels,
                                    size_t *view_stride_points, int64_t *n_vertices, int64_t *n_components)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_components);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    rc = ensure_cc_buffers(x);
    if (rc) return rc;
    CcBuffers b = x->cc;
    b.labels_out = x->d_cc_labels;
    rc = launched(x, launch_mesh_components(P, first_view, n_views, max_edge, b, x->stream));
    std::vector<unsigned long long> words;
    CcTotals t;
    if (!rc) rc = read_cc_totals(x, first_view, n_views, words, t);
    if (rc) return rc;
    for (int k = 0; k < n_views; k++) {
        n_vertices[k] = (int64_t)t.vertices(first_view + k)[0];
        n_components[k] = (int64_t)t.stat(first_view + k)[0];
    }
    if (device_labels) *device_labels = x->d_cc_labels + (size_t)first_view * P.px_view_stride;
    if (view_stride_points) *view_stride_points = P.px_view_stride;
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: the labels of the views back to back
extern "C" int sl3d_get_mesh_components(sl3d_ctx *x, int first_view, int n_views, float max_edge, int32_t *labels, int64_t vertex_capacity,
                                        int64_t *n_vertices, int64_t *n_components)
try {
    int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_components);
    if (rc) return rc;
    ON_DEVICE(x);
    const int32_t *dev = nullptr;
    size_t stride = 0;
    rc = sl3d_mesh_components(x, first_view, n_views, max_edge, &dev, &stride, n_vertices, n_components);
    if (rc || (rc = download_clamped(x, labels, dev, stride, n_views, n_vertices, vertex_capacity, 4))) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

static int check_filter_args(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices, const int64_t *n_vertices,
                             const int64_t *n_faces)
{
    const int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_faces);
    if (rc) return rc;
    if (min_vertices < 1) return fail(x, SL3D_E_INVALID_ARG, "min_vertices must be >= 1 (1: the mesh itself)");
    return SL3D_OK;
}

// Seven launches (cells, scan, union, flatten, keep, scan, emit), one read-back
extern "C" int sl3d_mesh_views_filtered(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices,
                                        sl3d_mesh_filtered *device_mesh, int64_t *n_vertices, int64_t *n_faces)
try {
    int rc = check_filter_args(x, first_view, n_views, max_edge, min_vertices, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    rc = ensure_cc_buffers(x);
    if (!rc) rc = ensure_ccf_buffers(x);
    if (rc) return rc;
    CcBuffers b = x->cc;
    b.labels_out = nullptr;
    rc = launched(x, launch_mesh_components(P, first_view, n_views, max_edge, b, x->stream));
    // (a component has fewer vertices than INT_MAX: every larger bar keeps nothing, as INT_MAX does)
    if (!rc) rc = launched(x, launch_mesh_filter(P, first_view, n_views, (int)std::min<int64_t>(min_vertices, INT32_MAX), b, x->ccf, x->stream));
    std::vector<unsigned long long> words;
    CcTotals t;
    if (!rc) rc = read_cc_totals(x, first_view, n_views, words, t);
    if (rc) return rc;
    for (int k = 0; k < n_views; k++) {
        n_vertices[k] = (int64_t)t.kept(first_view + k)[0];
        n_faces[k] = (int64_t)t.kept(first_view + k)[1];
    }
    if (device_mesh) {
        device_mesh->xyz = x->ccf.xyz + 3 * (size_t)first_view * P.px_view_stride;
        device_mesh->faces = x->ccf.faces + 3 * (size_t)first_view * x->ccf.face_stride;
        device_mesh->vertex_ids = x->ccf.ids + (size_t)first_view * P.px_view_stride;
        device_mesh->view_stride_points = P.px_view_stride;
        device_mesh->view_stride_faces = x->ccf.face_stride;
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: the kept points of the views back to back in xyz, their original ids in vertex_ids, the kept faces in faces
extern "C" int sl3d_get_meshes_filtered(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices, float *xyz,
                                        int32_t *vertex_ids, int64_t vertex_capacity, int32_t *faces, int64_t face_capacity, int64_t *n_vertices,
                                        int64_t *n_faces)
try {
    int rc = check_filter_args(x, first_view, n_views, max_edge, min_vertices, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    sl3d_mesh_filtered m;
    rc = sl3d_mesh_views_filtered(x, first_view, n_views, max_edge, min_vertices, &m, n_vertices, n_faces);
    if (rc) return rc;
    rc = download_clamped(x, xyz, m.xyz, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, vertex_ids, m.vertex_ids, m.view_stride_points, n_views, n_vertices, vertex_capacity, 4);
    if (!rc) rc = download_clamped(x, faces, m.faces, m.view_stride_faces, n_views, n_faces, face_capacity);
    if (rc) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- smoothed vertices of those meshes, and their normals (sl3d_mesh_smooth.h: the definition, the ring and the step;
// sl3d_mesh_smooth.hip: the kernels) ---------------------------------------------------------------------------------------------------
static int ensure_smooth_buffers(sl3d_ctx *x, bool normals)
{
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views, px = mv * P.px_view_stride;
    int rc = normals ? ensure_plane(x, &x->d_smooth_normals, 3 * px) : SL3D_OK;
    if (rc || x->smooth_ready) return rc;  // (one flag, set at the very end: ensure_cloud_buffers)
    SmoothBuffers &b = x->smooth;
    if (!rc) rc = ensure_plane(x, &b.cells, px);
    if (!rc) rc = ensure_plane(x, &b.rings, px);
    if (!rc) rc = ensure_plane(x, &b.plane[0], 3 * px);
    if (!rc) rc = ensure_plane(x, &b.plane[1], 3 * px);
    if (!rc) rc = ensure_scratch(x, b.s, mv * (size_t)mesh_chunks(P), mv);
    if (rc) return rc;
    x->smooth_ready = true;
    return SL3D_OK;
}

static int check_smooth_args(sl3d_ctx *x, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu, unsigned flags,
                             const int64_t *n_vertices)
{
    const int rc = check_mesh_args(x, first_view, n_views, max_edge, n_vertices, n_vertices);
    if (rc) return rc;
    if (iterations < 1 || iterations > 1024) return fail(x, SL3D_E_INVALID_ARG, "iterations must lie in [1, 1024]");
    if (!(lambda > 0.0f && lambda <= 1.0f)) return fail(x, SL3D_E_INVALID_ARG, "lambda must lie in (0, 1]");        // (false for NaN)
    if (!(mu >= -1.0f && mu <= 0.0f)) return fail(x, SL3D_E_INVALID_ARG, "mu must lie in [-1, 0] (0: no second step)");
    if (flags & ~(SL3D_SMOOTH_FIX_BOUNDARY | SL3D_SMOOTH_NORMALS)) return fail(x, SL3D_E_INVALID_ARG, "unknown smoothing flag");
    return SL3D_OK;
}

// Cells, scan, rings, one launch per step, vertices out (and normals): 4 + steps (+ 1) launches, one read-back of the total per view.
// Reads the dense result only and writes buffers of its own.
extern "C" int sl3d_mesh_smooth(sl3d_ctx *x, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu, unsigned flags,
                                sl3d_mesh_smoothed *device_mesh, int64_t *n_vertices)
try {
    int rc = check_smooth_args(x, first_view, n_views, max_edge, iterations, lambda, mu, flags, n_vertices);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    const bool normals = flags & SL3D_SMOOTH_NORMALS;
    rc = ensure_smooth_buffers(x, normals);
    if (rc) return rc;
    SmoothBuffers b = x->smooth;
    b.normals = normals ? x->d_smooth_normals : nullptr;
    rc = launched(x, launch_mesh_smooth(P, first_view, n_views, max_edge, iterations, lambda, mu, flags & SL3D_SMOOTH_FIX_BOUNDARY, b, x->stream));
    if (!rc) rc = read_totals(x, b.s.tot, 1, first_view, n_views, n_vertices);
    if (rc) return rc;
    if (device_mesh) {
        device_mesh->xyz = b.plane[smooth_steps(iterations, mu) & 1] + 3 * (size_t)first_view * P.px_view_stride;
        device_mesh->normals = normals ? b.normals + 3 * (size_t)first_view * P.px_view_stride : nullptr;
        device_mesh->view_stride_points = P.px_view_stride;
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: the smoothed vertices of the views back to back, and their normals
extern "C" int sl3d_get_mesh_smoothed(sl3d_ctx *x, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu,
                                      unsigned flags, float *xyz, float *normals, int64_t vertex_capacity, int64_t *n_vertices)
try {
    int rc = check_smooth_args(x, first_view, n_views, max_edge, iterations, lambda, mu, flags, n_vertices);
    if (rc) return rc;
    ON_DEVICE(x);
    sl3d_mesh_smoothed m;
    rc = sl3d_mesh_smooth(x, first_view, n_views, max_edge, iterations, lambda, mu, flags, &m, n_vertices);
    if (rc) return rc;
    rc = download_clamped(x, xyz, m.xyz, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc && m.normals) rc = download_clamped(x, normals, m.normals, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (rc) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- the level-of-detail mesh: one vertex per step x step pixel block (include/sl3d.h: the definition; sl3d_mesh_lod.h: its arithmetic;
// sl3d_mesh_lod.hip: the block pass) ---------------------------------------------------------------------------------------------------
// the buffers of a call at `step` over the coarse grid C = lod_params(P, step, ..): every array at C's sizes, or larger from an earlier call
static int ensure_lod_buffers(sl3d_ctx *x, const KParams &C, bool normals, bool fine_scan)
{
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views, px = mv * C.px_view_stride, chunks = mv * (size_t)mesh_chunks(C), blocks = mv * compact_blocks(C);
    LodBuffers &b = x->lod;
    size_t *cap = x->lod_cap;
    const size_t face_stride = mesh_face_stride(C);
    int rc = grow_plane(x, &x->d_lod_valid, cap + 0, px);
    if (!rc) rc = grow_plane(x, &x->d_lod_points, cap + 1, 3 * px);
    if (!rc) rc = grow_plane(x, &b.ids, cap + 2, px);
    if (!rc) rc = grow_plane(x, &b.blk.cnt, cap + 3, blocks);
    if (!rc) rc = grow_plane(x, &b.blk.off, cap + 4, blocks);
    if (!rc) rc = grow_plane(x, &b.blk.tot, cap + 5, mv);
    if (!rc) rc = grow_plane(x, &b.chk.cnt, cap + 6, 2 * chunks);
    if (!rc) rc = grow_plane(x, &b.chk.off, cap + 7, 2 * chunks);
    if (!rc) rc = grow_plane(x, &b.chk.tot, cap + 8, 2 * mv);
    if (!rc) rc = grow_plane(x, &b.xyz, cap + 9, 3 * px);
    if (!rc) rc = grow_plane(x, &b.vertex_ids, cap + 10, px);
    if (!rc) rc = grow_plane(x, &b.faces, cap + 11, 3 * mv * face_stride);
    if (!rc && normals) {
        rc = grow_plane(x, &b.normals, cap + 12, 3 * px);
        if (!rc) rc = grow_plane(x, &b.nrm.cnt, cap + 13, chunks);
        if (!rc) rc = grow_plane(x, &b.nrm.off, cap + 14, chunks);
        if (!rc) rc = grow_plane(x, &b.nrm.tot, cap + 15, mv);
    }
    if (!rc && fine_scan) {  // (the fine window's sizes: the same at every step)
        const size_t fine_chunks = mv * (size_t)mesh_chunks(P);
        rc = grow_plane(x, &x->d_lod_cells, cap + 16, mv * P.px_view_stride);
        if (!rc) rc = grow_plane(x, &x->lod_fine.cnt, cap + 17, fine_chunks);
        if (!rc) rc = grow_plane(x, &x->lod_fine.off, cap + 18, fine_chunks);
        if (!rc) rc = grow_plane(x, &x->lod_fine.tot, cap + 19, mv);
    }
    if (rc) return rc;
    b.face_stride = face_stride;
    return SL3D_OK;
}

static int check_lod_args(sl3d_ctx *x, int first_view, int n_views, int step, float max_edge, int64_t min_vertices, float lod_edge, unsigned flags,
                          const int64_t *n_vertices, const int64_t *n_faces)
{
    const int rc = check_filter_args(x, first_view, n_views, max_edge, min_vertices, n_vertices, n_faces);
    if (rc) return rc;
    if (step < 1 || step > LOD_MAX_STEP) return fail(x, SL3D_E_INVALID_ARG, "step must lie in [1, 16]");
    if (!(lod_edge > 0.0f)) return fail(x, SL3D_E_INVALID_ARG, "lod_edge must be > 0 (+inf: no edge-length test)");  // (false for NaN)
    if (flags & ~(SL3D_LOD_MEAN | SL3D_LOD_NORMALS)) return fail(x, SL3D_E_INVALID_ARG, "unknown level-of-detail flag");
    return SL3D_OK;
}

// min_vertices == 1: cells and scan (for the ids), blocks, the compaction's three and the mesh's three launches over the coarse grid, ids
// (+ the normals' three): 10 (13) launches.  min_vertices > 1: the components' four launches and the keep bytes in place of the first two.
// One read-back of the 2 totals per view (and, behind the components, of their failure words)
extern "C" int sl3d_mesh_views_lod(sl3d_ctx *x, int first_view, int n_views, int step, float max_edge, int64_t min_vertices, float lod_edge,
                                   unsigned flags, sl3d_mesh_lod *device_mesh, int64_t *n_vertices, int64_t *n_faces)
try {
    int rc = check_lod_args(x, first_view, n_views, step, max_edge, min_vertices, lod_edge, flags, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    const bool normals = flags & SL3D_LOD_NORMALS, filtered = min_vertices > 1;
    KParams C = lod_params(P, step, nullptr, nullptr);
    rc = ensure_lod_buffers(x, C, normals, !filtered);
    if (!rc && filtered) rc = ensure_cc_buffers(x);
    if (!rc && filtered) rc = ensure_ccf_buffers(x);
    if (rc) return rc;
    C.valid = x->d_lod_valid, C.points = x->d_lod_points;
    LodSource src{};
    if (filtered) {
        CcBuffers b = x->cc;
        b.labels_out = nullptr;
        rc = launched(x, launch_mesh_components(P, first_view, n_views, max_edge, b, x->stream));
        if (!rc) rc = launched(x, launch_mesh_keep(P, first_view, n_views, (int)std::min<int64_t>(min_vertices, INT32_MAX), b, x->ccf, x->stream));
        src = LodSource{x->ccf.keep, nullptr, x->cc.vid};
    } else {
        const MeshLaunch L = mesh_launch(P, first_view, n_views);
        const CompactScratch c = L.sliced(x->lod_fine, 1);
        rc = launched(x, launch_mesh_cells(P, L, max_edge, x->d_lod_cells, nullptr, nullptr, nullptr, c, x->stream));
        src = LodSource{P.valid, c.off, nullptr};
    }
    if (!rc) rc = launched(x, launch_mesh_lod(P, C, first_view, n_views, step, lod_edge, flags & SL3D_LOD_MEAN, src, x->lod, normals, x->stream));
    if (!rc) rc = read_totals(x, x->lod.chk.tot, 2, first_view, n_views, n_vertices, n_faces);
    if (!rc && filtered) {
        std::vector<unsigned long long> words;
        CcTotals t;
        rc = read_cc_totals(x, first_view, n_views, words, t);
    }
    if (rc) return rc;
    if (device_mesh) {
        device_mesh->xyz = x->lod.xyz + 3 * (size_t)first_view * C.px_view_stride;
        device_mesh->faces = x->lod.faces + 3 * (size_t)first_view * x->lod.face_stride;
        device_mesh->vertex_ids = x->lod.vertex_ids + (size_t)first_view * C.px_view_stride;
        device_mesh->normals = normals ? x->lod.normals + 3 * (size_t)first_view * C.px_view_stride : nullptr;
        device_mesh->view_stride_points = C.px_view_stride;
        device_mesh->view_stride_faces = x->lod.face_stride;
        device_mesh->grid_width = C.W;
        device_mesh->grid_height = C.H;
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: vertices, original ids and normals of the views back to back, their faces back to back
extern "C" int sl3d_get_meshes_lod(sl3d_ctx *x, int first_view, int n_views, int step, float max_edge, int64_t min_vertices, float lod_edge,
                                   unsigned flags, float *xyz, int32_t *vertex_ids, float *normals, int64_t vertex_capacity, int32_t *faces,
                                   int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces)
try {
    int rc = check_lod_args(x, first_view, n_views, step, max_edge, min_vertices, lod_edge, flags, n_vertices, n_faces);
    if (rc) return rc;
    ON_DEVICE(x);
    sl3d_mesh_lod m;
    rc = sl3d_mesh_views_lod(x, first_view, n_views, step, max_edge, min_vertices, lod_edge, flags, &m, n_vertices, n_faces);
    if (rc) return rc;
    rc = download_clamped(x, xyz, m.xyz, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, vertex_ids, m.vertex_ids, m.view_stride_points, n_views, n_vertices, vertex_capacity, 4);
    if (!rc && m.normals) rc = download_clamped(x, normals, m.normals, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, faces, m.faces, m.view_stride_faces, n_views, n_faces, face_capacity);
    if (rc) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)

// ---- the hole filling: small interior holes of a view's candidate map filled from their rims (include/sl3d.h: the definition;
// sl3d_mesh_holes.h: its arithmetic and the union-find; sl3d_mesh_holes.hip: the kernels) ------------------------------------------------
static int ensure_hole_buffers(sl3d_ctx *x, bool normals, bool fine_scan)
{
    const KParams &P = x->P;
    const size_t mv = (size_t)x->cfg.max_views, px = mv * P.px_view_stride, chunks = mv * (size_t)mesh_chunks(P), blocks = mv * compact_blocks(P);
    HoleBuffers &b = x->holes;
    int rc = SL3D_OK;
    if (!x->holes_ready) {
        b.face_stride = mesh_face_stride(P);
        rc = ensure_plane(x, &x->d_hole_valid, px);
        if (!rc) rc = ensure_plane(x, &x->d_hole_points, 3 * px);
        if (!rc) rc = ensure_plane(x, &b.labels, px);
        if (!rc) rc = ensure_plane(x, &b.sizes, px);
        if (!rc) rc = ensure_plane(x, &b.ids, px);
        if (!rc) rc = ensure_plane(x, &x->d_hole_tot, 5 * mv);
        if (!rc) rc = ensure_plane(x, &b.hol.cnt, 2 * chunks);
        if (!rc) rc = ensure_plane(x, &b.hol.off, 2 * chunks);
        if (!rc) rc = ensure_plane(x, &b.blk.cnt, blocks);
        if (!rc) rc = ensure_plane(x, &b.blk.off, blocks);
        if (!rc) rc = ensure_plane(x, &b.blk.tot, mv);
        if (!rc) rc = ensure_plane(x, &b.chk.cnt, 2 * chunks);
        if (!rc) rc = ensure_plane(x, &b.chk.off, 2 * chunks);
        if (!rc) rc = ensure_plane(x, &b.xyz, 3 * px);
        if (!rc) rc = ensure_plane(x, &b.vertex_ids, px);
        if (!rc) rc = ensure_plane(x, &b.faces, 3 * mv * b.face_stride);
        if (rc) return rc;
        b.chk.tot = x->d_hole_tot, b.hol.tot = x->d_hole_tot + 2 * mv, b.failed = x->d_hole_tot + 4 * mv;
        x->holes_ready = true;
    }
    if (normals && !x->holes_normals_ready) {
        rc = ensure_plane(x, &b.normals, 3 * px);
        if (!rc) rc = ensure_scratch(x, b.nrm, chunks, mv);
        if (rc) return rc;
        x->holes_normals_ready = true;
    }
    if (fine_scan && !x->holes_fine_ready) {
        rc = ensure_plane(x, &x->d_hole_cells, px);
        if (!rc) rc = ensure_scratch(x, x->hole_fine, chunks, mv);
        if (rc) return rc;
        x->holes_fine_ready = true;
    }
    return SL3D_OK;
}

static int check_hole_args(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices, int64_t max_hole, float fill_edge,
                           unsigned flags, const int64_t *n_vertices, const int64_t *n_faces, const int64_t *n_holes, const int64_t *n_filled)
{
    const int rc = check_filter_args(x, first_view, n_views, max_edge, min_vertices, n_vertices, n_faces);
    if (rc) return rc;
    if (!n_holes || !n_filled) return fail(x, SL3D_E_INVALID_ARG, "null argument");
    if (max_hole < 0) return fail(x, SL3D_E_INVALID_ARG, "max_hole must be >= 0 (0: nothing is filled)");
    if (!(fill_edge > 0.0f)) return fail(x, SL3D_E_INVALID_ARG, "fill_edge must be > 0 (+inf: every span is usable)");  // (false for NaN)
    if (flags & ~SL3D_FILL_NORMALS) return fail(x, SL3D_E_INVALID_ARG, "unknown hole-filling flag");
    return SL3D_OK;
}

// min_vertices == 1: cells and scan (for the ids), the four hole kernels and the scan of their counts, the compaction's three and the
// mesh's three launches over the filled grid, ids (+ the normals' three): 15 (18) launches.  min_vertices > 1: the components' four launches and the keep bytes in place
// of the first two.  One read-back of the totals and the hole words (and, behind the components, one of their failure words)
extern "C" int sl3d_mesh_fill_holes(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices, int64_t max_hole, float fill_edge,
                                    unsigned flags, sl3d_mesh_holes *device_mesh, int64_t *n_vertices, int64_t *n_faces, int64_t *n_holes,
                                    int64_t *n_filled)
try {
    int rc = check_hole_args(x, first_view, n_views, max_edge, min_vertices, max_hole, fill_edge, flags, n_vertices, n_faces, n_holes, n_filled);
    if (rc) return rc;
    ON_DEVICE(x);
    const KParams &P = x->P;
    const bool normals = flags & SL3D_FILL_NORMALS, filtered = min_vertices > 1;
    rc = ensure_hole_buffers(x, normals, !filtered);
    if (!rc && filtered) rc = ensure_cc_buffers(x);
    if (!rc && filtered) rc = ensure_ccf_buffers(x);
    if (rc) return rc;
    KParams F = P;
    F.valid = x->d_hole_valid, F.points = x->d_hole_points;
    LodSource src{};
    if (filtered) {
        CcBuffers b = x->cc;
        b.labels_out = nullptr;
        rc = launched(x, launch_mesh_components(P, first_view, n_views, max_edge, b, x->stream));
        if (!rc) rc = launched(x, launch_mesh_keep(P, first_view, n_views, (int)std::min<int64_t>(min_vertices, INT32_MAX), b, x->ccf, x->stream));
        src = LodSource{x->ccf.keep, nullptr, x->cc.vid};
    } else {
        const MeshLaunch L = mesh_launch(P, first_view, n_views);
        const CompactScratch c = L.sliced(x->hole_fine, 1);
        rc = launched(x, launch_mesh_cells(P, L, max_edge, x->d_hole_cells, nullptr, nullptr, nullptr, c, x->stream));
        src = LodSource{P.valid, c.off, nullptr};
    }
    if (!rc)
        rc = launched(x, launch_mesh_holes(P, F, first_view, n_views, max_edge, (int)std::min<int64_t>(max_hole, INT32_MAX), fill_edge, src, x->holes, normals,
                                           x->stream));
    if (rc) return rc;
    const size_t mv = (size_t)x->cfg.max_views;
    std::vector<unsigned long long> t(5 * mv);
    HIPCHK(x, hipMemcpyAsync(t.data(), x->d_hole_tot, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    for (int k = 0; k < n_views; k++) {
        const size_t v = (size_t)first_view + k;
        if (t[4 * mv + v])
            return fail(x, SL3D_E_INTERNAL, "hole filling: a walk of view " + std::to_string(v) + " ran out of its iteration bound");
        n_vertices[k] = (int64_t)t[2 * v], n_faces[k] = (int64_t)t[2 * v + 1];
        n_holes[k] = (int64_t)t[2 * mv + 2 * v], n_filled[k] = (int64_t)t[2 * mv + 2 * v + 1];
    }
    if (filtered) {
        std::vector<unsigned long long> words;
        CcTotals ct;
        rc = read_cc_totals(x, first_view, n_views, words, ct);
        if (rc) return rc;
    }
    if (device_mesh) {
        const size_t v0 = (size_t)first_view * P.px_view_stride;
        device_mesh->xyz = x->holes.xyz + 3 * v0;
        device_mesh->faces = x->holes.faces + 3 * (size_t)first_view * x->holes.face_stride;
        device_mesh->vertex_ids = x->holes.vertex_ids + v0;
        device_mesh->normals = normals ? x->holes.normals + 3 * v0 : nullptr;
        device_mesh->view_stride_points = P.px_view_stride;
        device_mesh->view_stride_faces = x->holes.face_stride;
    }
    return SL3D_OK;
}
SL3D_CATCH(x)

// host copy: vertices, ids and normals of the views back to back, their faces back to back
extern "C" int sl3d_get_meshes_holes_filled(sl3d_ctx *x, int first_view, int n_views, float max_edge, int64_t min_vertices, int64_t max_hole,
                                            float fill_edge, unsigned flags, float *xyz, int32_t *vertex_ids, float *normals, int64_t vertex_capacity,
                                            int32_t *faces, int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces, int64_t *n_holes,
                                            int64_t *n_filled)
try {
    int rc = check_hole_args(x, first_view, n_views, max_edge, min_vertices, max_hole, fill_edge, flags, n_vertices, n_faces, n_holes, n_filled);
    if (rc) return rc;
    ON_DEVICE(x);
    sl3d_mesh_holes m;
    rc = sl3d_mesh_fill_holes(x, first_view, n_views, max_edge, min_vertices, max_hole, fill_edge, flags, &m, n_vertices, n_faces, n_holes, n_filled);
    if (rc) return rc;
    rc = download_clamped(x, xyz, m.xyz, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, vertex_ids, m.vertex_ids, m.view_stride_points, n_views, n_vertices, vertex_capacity, 4);
    if (!rc && m.normals) rc = download_clamped(x, normals, m.normals, m.view_stride_points, n_views, n_vertices, vertex_capacity);
    if (!rc) rc = download_clamped(x, faces, m.faces, m.view_stride_faces, n_views, n_faces, face_capacity);
    if (rc) return rc;
    SYNC_FOR_CALLER(x);
    return SL3D_OK;
}
SL3D_CATCH(x)
