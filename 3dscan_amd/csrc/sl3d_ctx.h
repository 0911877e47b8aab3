// sl3d_ctx.h -- the context behind the opaque sl3d_ctx handle, shared by the C-ABI translation units
// (sl3d_capi_*.cpp: single-GPU entry points; sl3d_group.cpp: row-stripe groups over several GPUs).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/sl3d.h"
#include "sl3d_direct_gray.h"
#include "sl3d_internal.h"
#include "sl3d_lanes.h"

using namespace sl3d;

struct sl3d_ctx {
    sl3d_config cfg{};
    KParams P{};
    DevCal C{};
    SynthParams S{};  // extrinsics kept for the synthetic-capture generator
    bool have_cal = false;
    int rig = 0;
    bool keep = false;
    // SL3D_FLAG_SUBPIXEL: sl3d_run leaves the sub-pixel scan.  Which launch that takes is fused_route (sl3d_capi_internal.h)
    bool subpixel = false;
    // SL3D_FLAG_REPAIR_PERIODS: sl3d_run leaves the scan with the 2*Pi period jumps of both axes repaired (radius 4, one pass).  Which
    // launches that takes is fused_route (sl3d_capi_internal.h)
    bool repair = false;
    // SL3D_FLAG_ANCHOR_PERIODS (only with subpixel, never with repair: sl3d_create): the sub-pixel solve and
    // sl3d_get_correspondences_subpixel take the anchored coordinates (sl3d_anchor.h)
    bool anchor = false;
    // SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL (only with subpixel, never with repair: sl3d_create): the coded axis, 0 or 1, of a
    // one-axis context (sl3d_one_axis.h) -- no frame and no stage plane of the other axis is read, there is no residual plane; -1 otherwise
    int one_axis = -1;
    // SL3D_FLAG_DIRECT_GRAY (only with subpixel, never with repair: sl3d_create): stage 4 thresholds a Gray frame against the fringe mean
    // (sl3d_direct_gray.h) -- no inverse Gray plane is read or uploaded
    bool direct_gray = false;
    bool own_kernel_ran = false;  // an own_kernel route (fused_route): a launch has gone out (sl3d_last_fused_kernel_name)
    bool own_stream = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Launch lanes (sl3d_lanes.h: the policy; sl3d_capi_run.cpp turns its plans into events and waits): consecutive small launches of a
    // LONG series run on two internal streams in turn, the tail of one under the ramp of the next.  Every other entry point first makes
    // the context's stream wait for both lanes (ON_DEVICE), so the one-stream ordering the ABI promises holds for everything a caller
    // can observe.  Only on a stream the context created itself.
    bool lanes_ok = false;
    hipStream_t lane[2] = {nullptr, nullptr};
    hipEvent_t ev_lane[2] = {nullptr, nullptr}, ev_main = nullptr;
    LanePolicy lp;
    long long launches_on_stream = 0, launches_on_lanes = 0;  // sl3d_launch_counts
    std::vector<void *> allocs;
    std::string err;
    uint8_t *d_frames = nullptr, *d_mask = nullptr, *d_valid = nullptr, *d_band = nullptr;
    uint8_t *d_mask_raw = nullptr;            // sl3d_set_mask(s): the caller's bytes (window + halo) of mask_raw_slots views, staged for
    int mask_raw_slots = 0;                   // k_mask_prepare; zero outside the copied region (the kernel relies on that)
    // quads with a valid pixel, per view: every block of k_mask_prepare stores {seq, count} into this host array (mapped into the
    // device: d_quad_part is the same memory as the kernels address it); the host adds a view's blocks up on demand and treats the
    // view as unknown until every block carries the sequence number of the view's last preparation (quads_known, sl3d_capi_inputs.cpp)
    volatile unsigned long long *h_quad_part = nullptr;
    unsigned long long *d_quad_part = nullptr;
    int quad_blocks = 0;                      // blocks per view
    std::vector<unsigned> quad_seq;           // [max_views] sequence number of the view's last preparation (0 = never set)
    std::vector<int> quad_src;                // [max_views] the view whose blocks hold this view's count (sl3d_copy_view duplicates masks)
    mutable std::vector<unsigned> quad_sum_seq, quad_sum;  // [max_views] the sum once it was complete, and the preparation it belongs to
    mutable std::vector<unsigned> quad_last;               // [max_views] the last sum that WAS complete, of whichever preparation (~0u: none yet):
                                                           // what routes a launch while the current count is still on its way (sparse_views)
    unsigned mask_seq = 0;
    // Deferred masks (sl3d_set_mask(s) of at most SL3D_SMALL_LAUNCH_VIEWS views on a timed context, unless SL3D_FLAG_EAGER_MASK): the
    // view's selection has been handed over but not prepared -- the next small launch over such views evaluates it inside the fused
    // kernel (a MASKIN launch, sl3d_fused.h), every other consumer of the view's planes prepares it first (flush_masks, sl3d_capi_inputs.cpp).
    struct PendingMask {
        bool pending = false;
        bool ours = false;     // the source is the context's staging plane (else the CALLER's device memory: prepared at the next synchronising call at the latest)
        uintptr_t origin = 0;  // MaskSrc::origin of this view
        size_t stride = 0;
        int lo = 0, hi = 0;    // plane bytes of a row that may be read (MaskIn)
    };
    std::vector<PendingMask> pend;            // [max_views]
    int n_pending = 0;
    bool eager_mask = false;
    volatile unsigned *h_mi_part = nullptr;   // MASKIN launches: per view and wave {seq << 8 | quads with a valid pixel} (mapped host memory)
    unsigned *d_mi_part = nullptr;
    unsigned mi_part_stride = 0, mi_part_words = 0;
    std::vector<uint8_t> quad_kind;           // [max_views] whose words hold the view's count: 0 = k_mask_prepare's blocks, 1 = a MASKIN launch's waves
    // the instantiation the fused launch made last on this context RAN (launch_fused; nmax == 0: none yet)
    FusedKey last_fused;
    float *d_points = nullptr;
    CompactScratch blk_one{};                 // compaction scratch of sl3d_compact (one view at a time)
    float *d_cloud = nullptr;                 // compacted cloud of one view (capacity = window pixels)
    float *d_reg = nullptr;                   // registered clouds of all views (allocated on first use)
    uint8_t *d_raw = nullptr;  // sl3d_set_frames_raw: the raw planes of one axis + the camera's undistortion map
    bool raw_map_valid = false;
    double Kc_raw[9] = {0}, dc_raw[5] = {0};  // the camera intrinsics the raw path undistorts with (set_calibration)
    uint8_t *d_und = nullptr;  // cvUndistort2 scratch: maps, source image, result (grown on demand)
    size_t und_bytes = 0;
    double und_key[16] = {0};  // K, dist, width, height of the map held in d_und (the 46 frames of a view share one map)
    bool und_map_valid = false;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;   // sl3d_process_views: upload and download run beside the compute stream
    std::vector<hipEvent_t> ev_up, ev_done, ev_down;  // per view slot: frames landed / kernel finished / results copied out
    float *d_clouds = nullptr;                // the segmented clouds sl3d_run_clouds writes: px_view_stride point slots per view (first use)
    CompactScratch blk_all{};                 // compaction scratch of sl3d_compact_views (the batch goes to d_packed)
    unsigned *d_seg_counts = nullptr;         // sl3d_run_clouds (segmented clouds): [view][n_segs] counts, their exclusive scan,
    unsigned long long *d_seg_offsets = nullptr;
    float *d_packed = nullptr;                // and the contiguous copy made on demand (also the output of sl3d_compact_views)
    enum class Scan : uint8_t {
        DONE,        // k_seg_scan has run: offsets and total valid
        PENDING,     // not scanned: a launch of a few views leaves the scan to the consumer (k_seg_close<.., SCAN>)
        TOTAL_ONLY,  // a scanning consumer has left the total, the offsets are still unset
    };
    std::vector<Scan> scan_state;             // per view, after sl3d_run_clouds
    // sl3d_mesh_views (all allocated on first use): the chunk scratch in its mesh form (CompactScratch, sl3d_internal.h); the faces:
    // [max_views][mesh_face_stride][3] vertex ids into the view's cloud in d_mesh_xyz ([max_views][px_view_stride][3], written by
    // launch_compact_views with block scratch of its own: nothing another call handed out is overwritten)
    CompactScratch chk_mesh{};
    CompactScratch blk_mesh{};                // the block scratch of that compaction
    int32_t *d_mesh_faces = nullptr;
    float *d_mesh_xyz = nullptr;
    size_t mesh_face_stride = 0;
    bool mesh_ready = false;                  // ensure_mesh_buffers ran to its end
    // sl3d_mesh_normals (all allocated on first use, nothing shared with the mesh call): the chunk scratch in its normals form; the
    // normals: [max_views][px_view_stride][3], a view's in the order of its cloud
    CompactScratch chk_nrm{};
    float *d_normals = nullptr;
    bool normals_ready = false;               // ensure_normal_buffers ran to its end
    // sl3d_mesh_components / sl3d_mesh_views_filtered (all allocated on first use, nothing shared with the mesh or the normals call):
    // the planes and scratch of the union-find (CcBuffers, sl3d_internal.h; cc.labels_out is set per call) and the labels handed out;
    // the filtered meshes (CcFiltered).  cc.s.tot is ONE array a call reads back whole, its layout CcTotals (sl3d_internal.h): cc.s.tot,
    // ccf.s.tot and cc.stat point at its three parts
    CcBuffers cc{};
    int32_t *d_cc_labels = nullptr;
    bool cc_ready = false;                    // ensure_cc_buffers ran to its end
    CcFiltered ccf{};
    bool ccf_ready = false;                   // ensure_ccf_buffers ran to its end
    // sl3d_mesh_smooth (all allocated on first use, nothing shared with the calls above): cell and ring bytes, the two planes of the
    // steps, the chunk scratch (SmoothBuffers, sl3d_internal.h; smooth.normals is set per call) and, from the first call that asks for
    // them, the normals of the smoothed mesh
    SmoothBuffers smooth{};
    float *d_smooth_normals = nullptr;
    bool smooth_ready = false;                // ensure_smooth_buffers ran to its end
    // sl3d_mesh_views_lod (all allocated on first use for the step asked, grown when a later call needs more; the outputs share nothing
    // with the calls above): the coarse valid / point planes the block pass writes and everything launched over them (LodBuffers,
    // sl3d_internal.h); for min_vertices == 1 the cell bytes and the chunk scratch of the cell pass that gives the ids.  lod_cap: the
    // elements every one of those arrays holds, in the order ensure_lod_buffers names them
    uint8_t *d_lod_valid = nullptr;
    float *d_lod_points = nullptr;
    LodBuffers lod{};
    uint8_t *d_lod_cells = nullptr;
    CompactScratch lod_fine{};
    size_t lod_cap[20] = {0};
    // sl3d_mesh_fill_holes (all allocated on first use; the outputs share nothing with the calls above): the filled grid's valid / point
    // planes and everything launched over them (HoleBuffers, sl3d_internal.h); hole_tot: the call's one read-back -- [max_views][2] the
    // mesh totals (holes.chk.tot), [max_views][2] holes and filled pixels (holes.hol.tot), [max_views] holes.failed; for min_vertices == 1 the cell bytes and the chunk scratch of the
    // cell pass that gives the ids
    uint8_t *d_hole_valid = nullptr;
    float *d_hole_points = nullptr;
    HoleBuffers holes{};
    unsigned long long *d_hole_tot = nullptr;
    uint8_t *d_hole_cells = nullptr;
    CompactScratch hole_fine{};
    bool holes_ready = false, holes_normals_ready = false, holes_fine_ready = false;
    // sl3d_repair_periods (allocated on first use): the jump plane of one view, the wide plane beside it for an axis of 8 or more Gray
    // planes, and [max_views][2][2] words: repaired and unrepairable pixels of the last pass over a view's axis
    int8_t *d_period_jump = nullptr;
    int *d_period_wide = nullptr;
    unsigned *d_period_counts = nullptr;
    // sl3d_triangulate_subpixel (allocated on first use): the residual plane [max_views][px_view_stride]; for a caller that wants the
    // counts a word per block of the launch and [max_views][2] words, the triangulated and the rejected pixels of the call's views;
    // sl3d_get_correspondences_subpixel: (xs, ys) of one view.  A SL3D_FLAG_SUBPIXEL context allocates the residual plane when it is
    // created; residual_ready: a call has written residuals (sl3d_get_residuals refuses before)
    float *d_residual = nullptr;
    bool residual_ready = false;
    unsigned *d_subpixel_partials = nullptr, *d_subpixel_counts = nullptr;
    double *d_subpixel_xy = nullptr;
    // sl3d_fuse_exposures (allocated on the first fusion): the exposure maps [max_views][px_view_stride] bytes, the SL3D_EXPOSURE_COUNTS
    // words a launch adds its counts to, and which views' maps a fusion has written (sl3d_get_exposure_map refuses the others)
    uint8_t *d_exposure_map = nullptr;
    unsigned *d_exposure_counts = nullptr;
    std::vector<char> exposure_written;
    // sl3d_filter_outliers (allocated on the first call): the support planes [max_views][px_view_stride] bytes, [max_views][2] words a
    // call adds its views' counts to, and which views' planes a call has written (sl3d_get_support refuses the others)
    uint8_t *d_support = nullptr;
    unsigned *d_outlier_counts = nullptr;
    std::vector<char> support_written;
    // sl3d_voxel_grid (all allocated on first use and grown with the cloud, vox_cap: the elements each holds, in the order
    // sl3d_capi_voxel.cpp names them): the upload of a host cloud, the hash table (one allocation: key, first, count, sums), a slot word
    // per point, the block scratch (vox_s.tot is not used: the total is one of the call's words), the three outputs and the call's
    // words.  vox_n: the points of the last grid call, -1 before any (sl3d_get_voxel_grid refuses then).  reg_total: the points the last
    // sl3d_register_views / sl3d_register_clouds left in d_reg, -1 before any
    float *d_vox_in = nullptr;
    uint8_t *d_vox_table = nullptr;
    unsigned *d_vox_slot = nullptr;
    CompactScratch vox_s{};
    float *d_vox_xyz = nullptr;
    int32_t *d_vox_first = nullptr;
    unsigned *d_vox_count = nullptr;
    unsigned long long *d_vox_words = nullptr;
    size_t vox_cap[8] = {0};
    int64_t vox_n = -1, reg_total = -1;
    // The pairs' records of the two refinements (allocated on first use by align_pass, sl3d_capi_align.cpp; freed by sl3d_destroy): [0]
    // sl3d_align_sums / sl3d_refine_turntable, [max_views - 1][ALIGN_WORDS] words; [1] the point-to-plane form, [max_views - 1]
    // [ALIGN_PLANE_WORDS].  dev: the records on the device; host: the pinned block of the same size a pass's words are downloaded into.  Two
    // buffers: a call of one form leaves what the other has in flight alone.  dense_ran: a call that writes the dense planes (sl3d_run,
    // sl3d_process_views, sl3d_triangulate, sl3d_triangulate_subpixel) has gone out -- the passes refuse before
    struct AlignRecord {
        unsigned long long *dev = nullptr;
        long long *host = nullptr;
    } align_rec[2];
    bool dense_ran = false;
    // sl3d_align_normals / sl3d_align_plane_sums / sl3d_refine_turntable_plane (include/sl3d_align_plane.h; first use, sl3d_destroy): the
    // normal planes of the views [align_nrm_lo, align_nrm_hi) -- every view a call has asked for so far -- back to back, a view's laid out
    // like its points ([px_view_stride][3] floats, rows pitch pixels apart); align_nrm_ready[view]: its normals have been computed since the
    // block was last allocated
    float *d_align_nrm = nullptr;
    size_t align_nrm_cap = 0;
    int align_nrm_lo = 0, align_nrm_hi = 0;
    std::vector<char> align_nrm_ready;
    // sl3d_tsdf_reset / sl3d_tsdf_integrate / sl3d_tsdf_extract (include/sl3d_tsdf.h; first use, grown on demand, sl3d_destroy): the two
    // planes of the volume, the rotations and the depth planes of a call's views, the block scratch of an extraction (tsdf_s.tot is not used), its three
    // outputs and the calls' words; tsdf_cap: the elements each growing array holds, in the order sl3d_capi_tsdf.cpp names them.  The
    // volume as sl3d_tsdf_reset took it (tsdf_dims[0] == 0: no reset yet), the views integrated since, the crossings the last extraction
    // left (-1: none since the last reset)
    int32_t *d_tsdf_sum = nullptr;
    uint32_t *d_tsdf_weight = nullptr;
    double *d_tsdf_turns = nullptr;  // [max_views][2]: c_m, s_m
    double *d_tsdf_depth = nullptr;  // the depth planes of a call's views: [n_views][px_view_stride]
    CompactScratch tsdf_s{};
    float *d_tsdf_xyz = nullptr, *d_tsdf_nrm = nullptr;
    int32_t *d_tsdf_edge = nullptr;
    unsigned long long *d_tsdf_words = nullptr;
    size_t tsdf_cap[8] = {0};
    float tsdf_origin[3] = {0.0f, 0.0f, 0.0f}, tsdf_voxel = 0.0f, tsdf_trunc = 0.0f;
    int32_t tsdf_dims[3] = {0, 0, 0};
    int64_t tsdf_views = 0, tsdf_m = -1;
    bool clouds_ready = false;                // ensure_cloud_buffers ran to its end: every pointer sl3d_run_clouds needs is set
    unsigned long long *h_counts = nullptr;   // pinned + mapped: the per-view counts k_seg_scan stores, sl3d_get_cloud_counts reads
    // a view's total out of those words (the device stores them: read once the stream has drained)
    int64_t cloud_total(int view) const { return (int64_t)((volatile unsigned long long *)h_counts)[view]; }
    uint8_t *d_texture = nullptr;             // [view][row][pitch][3] BGR texture of save_point_cloud (allocated by sl3d_set_texture)
    uint8_t *d_cloud_rgb = nullptr;           // r,g,b of the compacted cloud of one view
    std::vector<char> have_texture;
    double *d_cam_tab = nullptr;              // timed mode: camera-side T1 table of the window (sl3d_set_calibration)
    size_t cam_tab_doubles = 0;
    float2 *d_proj_disp = nullptr;            // RIG 2: projector undistortion table (allocated when a distorted projector is set)
    RadEntry *d_proj_rad = nullptr;           // RIG 3: the projector's radial table, SL3D_RAD_COPIES copies
    uint8_t *d_pattern = nullptr, *d_profile = nullptr;  // projector pattern image + its 1-D profile (allocated on first use)
    size_t pattern_pitch = 0;
    uint8_t *d_colrow = nullptr;  // staging of one global in the reference's [col][row] layout (sl3d_get_global_colrow), and of a
    size_t colrow_bytes = 0;      // [col][row] selection mask on its way in (sl3d_set_mask_colrow)
    DevCal *d_cal = nullptr;  // device copy of C for the fused kernel (read through scalar loads)
    size_t mask_rows = 0;
    size_t dbg_words = 0;     // measurement builds (-DSL3D_TRACE): size of the phase-stamp buffer KParams::dbg
};

// records the message on the context (or, without one, as the thread's creation error) and returns `code`
__attribute__((visibility("hidden"))) int sl3d_fail(sl3d_ctx *c, int code, const std::string &msg);
#define fail sl3d_fail
// The exception barrier of the C ABI (no exceptions across the boundary).  Every extern "C" entry point that can allocate
// (new, std::vector, std::string ...) is a function-try-block whose handler ends in one of these: the exception in flight is
// classified (std::bad_alloc -> SL3D_E_NOMEM, anything else -> SL3D_E_INTERNAL), its text becomes the context's last error if that
// still can be stored, and the status is returned.  Nothing in here throws.
__attribute__((visibility("hidden"))) int sl3d_caught(sl3d_ctx *c, std::string *err_of_other_owner = nullptr) noexcept;
#define SL3D_CATCH(ctx) catch (...) { return sl3d_caught(ctx); }
#define SL3D_CATCH_RETURN(value) catch (...) { (void)sl3d_caught(nullptr); return value; }
#define SL3D_CATCH_VOID catch (...) { (void)sl3d_caught(nullptr); }
// sl3d_process_views in two halves (sl3d_capi_run.cpp), shared with sl3d_group_process_views
__attribute__((visibility("hidden"))) int sl3d_process_views_enqueue(sl3d_ctx *x, int n_views, const uint8_t *const *planes, size_t stride, float *xyz,
                                                                     size_t xyz_view_stride, uint8_t *valid, size_t valid_view_stride, size_t out_width);
__attribute__((visibility("hidden"))) int sl3d_process_views_wait(sl3d_ctx *x);

#define HIPCHK(c, call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail((c), SL3D_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
    } while (0)

// the same for asynchronous copies that touch CALLER memory in a loop: an error return first drains the stream, so that no copy
// enqueued earlier in the call is still running against buffers the caller is about to free
#define HIPCHK_DRAIN(c, call)                                                                       \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (void)hipStreamSynchronize((c)->stream);                                                \
            return fail((c), SL3D_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
        }                                                                                           \
    } while (0)

// Every entry point runs on the context's device and hands the caller's current device back on return: the caller may be a
// process that holds contexts on several GPUs, or a torch process whose current device differs.
struct DeviceGuard {
    int prev = -1, dev;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int d) : dev(d)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define ON_DEVICE_QUIET(x)                 \
    DeviceGuard dev_guard_((x)->cfg.device); \
    HIPCHK((x), dev_guard_.err)
// ... and whatever the call enqueues on the context's stream comes behind the launches the lanes hold (sl3d_run / sl3d_run_clouds
// and the hand-over of a device-resident deferred mask are the entry points that take the QUIET form and join only where they must)
__attribute__((visibility("hidden"))) int sl3d_lanes_join(sl3d_ctx *x);
#define ON_DEVICE(x)                                  \
    ON_DEVICE_QUIET(x);                               \
    do {                                              \
        const int join_rc_ = sl3d_lanes_join(x);      \
        if (join_rc_) return join_rc_;                \
    } while (0)

// the planes of a view a context reads, as runs [first[i], first[i] + count[i]) of planes_per_view; returns their number, 1 or 2.  All planes
// in one run, or those of a one-axis context's coded axis; on a SL3D_FLAG_DIRECT_GRAY context one run per coded axis, its F fringe and N Gray
// planes without the N inverse planes behind them
inline int frame_plane_runs(const sl3d_ctx *x, int first[2], int count[2])
{
    const sl3d::KParams &P = x->P;
    if (!x->direct_gray) {
        first[0] = x->one_axis == 1 ? P.F + 2 * P.Nv : 0;
        count[0] = x->one_axis == 0 ? P.F + 2 * P.Nv : x->one_axis == 1 ? P.F + 2 * P.Nh : P.planes_per_view;
        return 1;
    }
    int n = 0;
    for (int axis = 0; axis < 2; axis++) {
        if (x->one_axis >= 0 && x->one_axis != axis) continue;
        first[n] = axis == 0 ? 0 : P.F + 2 * P.Nv;
        count[n++] = direct_gray_planes(P.F, axis == 0 ? P.Nv : P.Nh);
    }
    return n;
}
// is plane p of planes_per_view one of them?
inline bool frame_plane_read(const sl3d_ctx *x, int p)
{
    int first[2], count[2];
    const int n = frame_plane_runs(x, first, count);
    for (int i = 0; i < n; i++)
        if (p >= first[i] && p < first[i] + count[i]) return true;
    return false;
}
