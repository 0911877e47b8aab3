/*
 * sl3d.h -- C ABI of the MI355X-native decode -> unwrap -> correspond -> triangulate path
 *           of the pranavkantgaur/3dscan structured-light scanner.
 *
 * This is the drop-in boundary for stages 3, 4, 5 and 7 of the reference.  Each entry point
 * names the reference interface it replaces (paths are relative to the reference tree).
 * The reference's own four entry points (C++ linkage, no arguments, global-array results) are
 * re-exported on top of this ABI by include/sl3d_shim.h / csrc/sl3d_shim.cpp.
 *
 * Conventions
 *   - plain C: opaque handle, int status codes (0 = ok, negative = error), no exceptions.
 *   - images are 8-bit single-channel row-major planes passed as (pointer, stride in bytes),
 *     which is exactly what an IplImage holds (imageData, widthStep) after
 *     cvLoadImage(..., CV_LOAD_IMAGE_GRAYSCALE)  [3/wrapped_phase.cpp:44, 4/phase_unwrap.cpp:78,84].
 *   - results are row-major planes; the shim transposes into the reference's [col][row] globals.
 *   - one context = one GPU + one HIP stream; all compute calls are asynchronous on that stream,
 *     getters synchronise.  Calls on one context must be serialised by the caller; different
 *     contexts are independent.
 *   - a context processes a WINDOW (width x height at col0,row0) of a camera frame of
 *     full_width x full_height: the whole frame on one GPU, or a row stripe per GPU.
 *   - the library needs a HIP device: there is no CPU fallback (SL3D_E_NO_DEVICE).
 */
#ifndef SL3D_H
#define SL3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL3D_VERSION_STRING "0.26.0"

typedef struct sl3d_ctx sl3d_ctx;

enum sl3d_status {
    SL3D_OK = 0,
    SL3D_E_INVALID_ARG = -1,
    SL3D_E_NO_DEVICE = -2,   /* no HIP device / runtime: the product path has no CPU fallback */
    SL3D_E_HIP = -3,         /* a HIP runtime call failed; see sl3d_last_error() */
    SL3D_E_STATE = -4,       /* call order violated (e.g. triangulate before set_calibration) */
    SL3D_E_UNSUPPORTED = -5,
    SL3D_E_NOMEM = -6,       /* device or host memory exhausted */
    SL3D_E_INTERNAL = -7     /* a C++ exception was stopped at the boundary (no exception ever crosses this C ABI); see sl3d_last_error() */
};

/* pattern_type of the reference: 0 = vertical stripes (encode the projector COLUMN),
 * 1 = horizontal stripes (encode the projector ROW)   [intermodule_dependencies.h:10,13] */
enum sl3d_axis { SL3D_AXIS_VERTICAL = 0, SL3D_AXIS_HORIZONTAL = 1 };

/* which valid map: valid_map_vertical / valid_map_horizontal / valid_map  [common_variables.h:18-21] */
enum sl3d_valid_which { SL3D_VALID_VERTICAL = 0, SL3D_VALID_HORIZONTAL = 1, SL3D_VALID_MERGED = 2 };

enum sl3d_flags {
    /* allocate the stage-boundary planes (wrapped/unwrapped phase, code, per-axis valid maps,
     * debug images, c_p_map, intersection_points).  Required for the per-stage entry points and
     * their getters; sl3d_run() then also stores them ("parity mode", +~70 B/px of traffic).
     * Without it only sl3d_run() and the point / valid getters are available (the timed mode). */
    SL3D_FLAG_KEEP_STAGES = 1u,
    /* sl3d_group_create only.  FORCE_RCCL: every stripe but the root's own travels by RCCL send/recv even when it shares the
     * root's GPU (exercises the RCCL path on a single-GPU box); NO_RCCL: (peer) device copies even across GPUs. */
    SL3D_FLAG_GROUP_FORCE_RCCL = 2u,
    SL3D_FLAG_GROUP_NO_RCCL = 4u,
    /* sl3d_group_create only, for tests on a box with fewer GPUs than stripes: every stripe gets its own communication side
     * (stream, event, communicator rank) even where devices repeat, so that the code paths of a stripe on ANOTHER GPU than the
     * root's -- peer copies, the waits between the sides' streams, an N-rank exchange -- run with all stripes on one device.
     * With RCCL this needs a communicator that accepts repeated devices (the test double bound through SL3D_RCCL_LIB). */
    SL3D_FLAG_GROUP_DISTINCT_SIDES = 16u,
    /* A context without KEEP_STAGES normally DEFERS the preparation of a selection mask handed over for at most 4 views: the next
     * sl3d_run / sl3d_run_clouds over exactly such views evaluates the selection inside the fused kernel itself (new mask + one view
     * = ONE launch, the reference's per-scan call shape), any other consumer prepares it first.  With this flag every mask is prepared
     * by its own kernel when it is set (the behaviour up to 0.4; A/B measurements). */
    SL3D_FLAG_EAGER_MASK = 32u,
    /* A context that created its own stream (config.stream == NULL) and has no KEEP_STAGES puts the sl3d_run / sl3d_run_clouds launches
     * of a LONG series of launches of at most 2 views (8 in a row, or fewer if the previous series was that long) on two internal
     * streams in turn, so that the tail of one launch runs under the ramp of the next when they work on different views (a launch over
     * a view a lane still works on goes behind it); every other call first makes the context's stream wait for both, so nothing a
     * caller can observe changes -- only the time: one view per launch from HBM, back to back, 25.8 -> 21.8 us per launch.  With this
     * flag every launch goes to the context's one stream (the behaviour up to 0.5; A/B measurements, and the time of a LONE launch). */
    SL3D_FLAG_SERIAL_LAUNCHES = 64u,
    /* (0.16.0) sl3d_run() -- and with it sl3d_run_timed, sl3d_process_views and the group calls built on them -- leaves the SUB-PIXEL
     * scan: after sl3d_run(ctx, first_view, n_views) the points and valid planes of those views and the residual plane hold, bit for
     * bit, what sl3d_compute_wrapped_phase + sl3d_unwrap_phase of both axes, sl3d_compute_c_p_map and sl3d_triangulate_subpixel(
     * first_view, n_views, +infinity, NULL) leave on a KEEP_STAGES context with the same configuration, calibration, masks and frames
     * (steps 1-4 and 6 at sl3d_triangulate_subpixel; nothing is rejected by the residual -- sl3d_get_residuals hands the plane out for
     * the caller to threshold).  May be combined with every other flag.
     *   Without KEEP_STAGES: ONE launch of a kernel of its own (k_subpixel_fused: frames in; points, valid and residuals out; no stage
     *   plane in between) on the context's stream -- such a context has no launch lanes -- behind the preparation of whatever masks
     *   of the views are still deferred.  sl3d_run_clouds has no sub-pixel form: SL3D_E_UNSUPPORTED (sl3d_run + sl3d_compact_views).
     *   The per-stage calls, sl3d_triangulate_subpixel and sl3d_get_correspondences_subpixel stay SL3D_E_STATE as on every timed context.
     *   With KEEP_STAGES: sl3d_run() launches what it always does (all stage planes, c_p_map) and sl3d_triangulate_subpixel's kernel
     *   behind it; sl3d_compute_c_p_map + sl3d_triangulate restores the integer result.
     * Every consumer of the dense planes (getters, compactions, colour, registration, meshes) sees the sub-pixel scan.  sl3d_group_create
     * hands the flag to its stripes.  A context without the flag behaves exactly as before. */
    SL3D_FLAG_SUBPIXEL = 128u,
    /* (0.17.0) sl3d_run() -- and with it sl3d_run_timed and sl3d_process_views -- leaves the scan with the 2*Pi period jumps of the
     * absolute phase REPAIRED: after sl3d_run(ctx, first_view, n_views) the points and valid planes of those views hold, bit for bit on
     * every pixel of the window (NaN patterns included), what this staged route leaves on a KEEP_STAGES context with the same
     * configuration, calibration, masks and frames: sl3d_compute_wrapped_phase + sl3d_unwrap_phase of both axes; sl3d_repair_periods(
     * view, axis, 4, NULL), one pass, for each axis that has Gray planes (an axis with n_gray == 0 is skipped: the staged call refuses
     * it); sl3d_compute_c_p_map; sl3d_triangulate.  With SL3D_FLAG_SUBPIXEL also set the last step is sl3d_triangulate_subpixel(
     * first_view, n_views, +infinity, NULL) instead, and the residual plane matches as well.
     *   The radius is fixed at 4.  Other radii, several passes and the repaired / unrepairable counts stay with sl3d_repair_periods.
     *   Without KEEP_STAGES: ONE launch of a kernel of its own (k_repair_fused: frames in; points, valid -- and residuals -- out; no
     *   stage plane in between; the block decodes the halo of its tile itself) on the context's stream -- such a context has no launch
     *   lanes, sl3d_launch_counts reports every launch as on-stream -- behind the preparation of whatever masks of the views are still
     *   deferred.  sl3d_fused_kernel_name / sl3d_last_fused_kernel_name give that kernel, sl3d_camera_table_bytes_per_pixel is 0.
     *   sl3d_run_clouds has no repaired form: SL3D_E_UNSUPPORTED (sl3d_run + sl3d_compact_views).  sl3d_repair_periods and the other
     *   per-stage calls stay SL3D_E_STATE as on every timed context.
     *   With KEEP_STAGES: sl3d_run() launches what it always does, then sl3d_repair_periods' launches for both axes at radius 4, then
     *   stage 5, then stage 7 (or sl3d_triangulate_subpixel's kernel): the stage getters show the repaired code and phase.
     * Every consumer of the dense planes sees the repaired scan.  sl3d_group_create refuses the flag (SL3D_E_UNSUPPORTED): a neighbourhood
     * is clipped to the context's window, so the horizontal axis of a row stripe would decide differently from the whole frame within 4
     * rows of every seam.  A context without the flag behaves exactly as before. */
    SL3D_FLAG_REPAIR_PERIODS = 256u,
    /* (0.18.0) The sub-pixel scan of a SL3D_FLAG_SUBPIXEL context takes ANCHORED projector coordinates: the period index of an axis is not
     * the Gray code itself but the fringe period nearest the centre of the pixel's Gray cell, and the fringe period is measured with pi,
     * not with the reference's Pi = 22/7 (its generator and decoder write 22/7 around a real cos / atan2: the Gray cell is fringe_width
     * projector pixels wide, the projected fringe has the period fringe_width * pi / (22/7)).  That takes out a scale error of
     * p * (22/7 - pi) / (22/7) = 4.0e-4 p pixels at projector coordinate p, and the period jumps in the band behind every Gray edge that
     * the drift of the phase's wrap against the edge leaves.  The definition, in IEEE double without contraction, in this order, so that
     * every route agrees bit for bit:
     *     P2 = (2.0 * 22.0) / 7.0    TWOPI = 2.0 * 3.141592653589793    INV = 0.15915494309189535
     *     c  = 0.0 for n_fringe == 3,  0.75 * (3.141592653589793 - 22.0 / 7.0) for n_fringe == 4
     *     w, code: what stage 4 leaves in the wrapped-phase plane (the float, Pi already added) and in the code plane
     *     a  = (double)w + c
     *     m  = rint((((double)code + 0.5) * P2 - a) * INV)            (round half to even)
     *     xs = (double)fringe_width * ((a + TWOPI * m) / P2)
     * on an axis of a pixel where stage 4's loop runs (frame columns 1..full_width-2 on the vertical axis, frame rows 1..full_height-2 on
     * the horizontal one) and only if that axis has n_gray > 0; everywhere else the coordinate stays the double stage 5 hands to lrint,
     * as without the flag.  The rule is pointwise: no neighbourhood, so windows and the stripes of a group agree with the whole frame.
     *   What changes: the (xs, ys) that the sub-pixel solve and sl3d_get_correspondences_subpixel use -- sl3d_run (the anchored
     *   instantiation of k_subpixel_fused on a timed context, of sl3d_triangulate_subpixel's kernel behind the parity launch with
     *   KEEP_STAGES) and sl3d_triangulate_subpixel itself, max_residual and counts as before; sl3d_fused_kernel_name /
     *   sl3d_last_fused_kernel_name report "sl3d::k_subpixel_fused<true>".  An anchored coordinate may lie a fraction of a pixel outside
     *   [0, proj_width - 1].
     *   What does not: the validity of a pixel -- the merged valid byte stays stage 5's, its range test on the integer c_p_map included --
     *   c_p_map, the wrapped and unwrapped phase planes, code and every other stage getter.
     *   Refused with SL3D_E_UNSUPPORTED by sl3d_create and sl3d_group_create before a device is touched: the flag without
     *   SL3D_FLAG_SUBPIXEL (the integer scan has no use for the coordinate), and together with SL3D_FLAG_REPAIR_PERIODS; and by
     *   sl3d_repair_periods on an anchored KEEP_STAGES context, which leaves every plane as it was.  The repair turns code from "Gray
     *   cell" into "fringe index": the pixel then sits at the edge of that cell, where anchoring to its centre is a coin flip.
     *   sl3d_run_clouds stays refused as on every SL3D_FLAG_SUBPIXEL context.  sl3d_group_create hands the flag to its stripes.
     * What remains: a tie band of relative width 4e-4 per cell in which two positions share one phase, and pixels whose Gray code itself
     * is wrong at an edge.  A context without the flag behaves exactly as before. */
    SL3D_FLAG_ANCHOR_PERIODS = 512u,
    /* (0.19.0) A ONE-AXIS scan: the sub-pixel scan of a SL3D_FLAG_SUBPIXEL context from ONE pattern direction.  A decoded projector column
     * (or row) is a plane in space and a camera pixel is a ray: three equations, three unknowns.  SL3D_FLAG_ONLY_VERTICAL codes axis a = 0
     * (the vertical-stripe patterns: the projector COLUMN), SL3D_FLAG_ONLY_HORIZONTAL axis a = 1 (the ROW); b is the other axis.  The
     * frame layout, planes_per_view and the setters do not change; planes of axis b may be set, but no frame of the other axis is read by
     * anything (sl3d_process_views and sl3d_group_process_views upload the planes of axis a alone, their contiguity test runs over those,
     * and the pointers of axis b may be NULL).  Per pixel of a view, in IEEE double, fma where written, nothing else contracted:
     *   1. sel = the valid byte of stage 3's boundary removal (the same byte for both axes).
     *   2. stages 3 and 4 of axis a as always: w_a, code_a, unw_a.
     *   3. stage 5: ok = the correspondence of axis a alone (the same lrint argument, FE_INVALID rule and range test); merged valid byte
     *      = sel && ok.  c_p_map[.][a] = the integer, c_p_map[.][b] = -1 where the pixel is valid; both 0 elsewhere.
     *   4. s = fringe_width_a * (unw_a / ((2.0 * 22.0) / 7.0)), the double stage 5 hands to lrint -- with SL3D_FLAG_ANCHOR_PERIODS the
     *      anchored coordinate of axis a where that flag's rule applies.
     *   5. f = Kp[0], c = Kp[2] (a = 0) or Kp[4], Kp[5] (a = 1):  t = fma(f, (s - c) * (1.0 / f), c)
     *   6. (u, v) = the undistorted camera point as in stage 7; Ac, Ap the 3 x 4 projection matrices:
     *        r0[j] = fma(-u, Ac[2][j], Ac[0][j])   f0 = fma(Ac[2][3], u, -Ac[0][3])        j = 0..2
     *        r1[j] = fma(-v, Ac[2][j], Ac[1][j])   f1 = fma(Ac[2][3], v, -Ac[1][3])
     *        r2[j] = fma(-t, Ap[2][j], Ap[a][j])   f2 = fma(Ap[2][3], t, -Ap[a][3])
     *        c0 = r1 x r2, c1 = r2 x r0, c2 = r0 x r1, where (p x q)[0] = fma(p[1], q[2], -(p[2] * q[1])), [1] = fma(p[2], q[0],
     *        -(p[0] * q[2])), [2] = fma(p[0], q[1], -(p[1] * q[0]))
     *        det = fma(r0[0], c0[0], fma(r0[1], c0[1], r0[2] * c0[2]))
     *        X[j] = fma(f0, c0[j], fma(f1, c1[j], f2 * c2[j])) * (1.0 / det);  det == 0: X = 0 and the valid byte stays, as in stage 7
     *      (X = adj(P) F / det(P) of the 3 x 3 system whose rows are r0, r1, r2)
     *   7. points = (float)X where valid, NaN and valid 0 elsewhere; intersection_points (KEEP_STAGES) = X where valid, 0 elsewhere.
     * An exactly determined solve has no residual: such a context has no residual plane, sl3d_get_residuals returns SL3D_E_UNSUPPORTED,
     * and so does sl3d_triangulate_subpixel with a finite max_residual (nothing changes); with +infinity it works, counts = (triangulated,
     * 0).  sl3d_get_correspondences_subpixel returns s in component a and NaN in component b, both NaN where the valid byte of axis a is
     * not 1.  sl3d_set_masks_modulated tests the modulation of axis a alone.
     *   Without KEEP_STAGES: ONE launch of a kernel of its own (k_one_axis<a, anchored>: the frames of axis a in; points and valid out) on
     *   the context's stream, behind the preparation of whatever masks are still deferred -- no launch lanes, every launch counts as
     *   on-stream, sl3d_camera_table_bytes_per_pixel is 0, sl3d_fused_kernel_name / sl3d_last_fused_kernel_name report
     *   "sl3d::k_one_axis<0, false>", "<0, true>", "<1, false>" or "<1, true>".  The result is bit for bit the staged route's.
     *   With KEEP_STAGES: sl3d_run() enqueues stages 3 and 4 of axis a, the one-axis stage 5 and the one-axis stage 7 per view (not the
     *   parity kernel, which reads both axes); sl3d_compute_c_p_map, sl3d_triangulate_subpixel and sl3d_get_correspondences_subpixel
     *   take their one-axis forms.  SL3D_E_UNSUPPORTED, nothing touched: sl3d_compute_wrapped_phase, sl3d_unwrap_phase and
     *   sl3d_repair_periods on axis b, and sl3d_triangulate (the integer solve).  The stage getters of axis b hand out planes that
     *   were never written.
     *   Refused with SL3D_E_UNSUPPORTED by sl3d_create and sl3d_group_create before a device is touched: both flags together; either
     *   without SL3D_FLAG_SUBPIXEL; either with SL3D_FLAG_REPAIR_PERIODS (the fused repair has no one-axis form).  By
     *   sl3d_set_calibration on such a context: a projector with any distortion coefficient != 0, or a Kp that is not plain (Kp[1],
     *   Kp[3], Kp[6], Kp[7] != 0 or Kp[8] != 1) -- with the other coordinate unknown a column is then a curve and not a line; the
     *   previous calibration stays in force.  sl3d_run_clouds stays refused as on every SL3D_FLAG_SUBPIXEL context.
     * sl3d_group_create hands the flag to its stripes; the rule is pointwise in frame coordinates, so stripes agree with the whole frame.
     * Where the baseline between camera and projector is horizontal the row carries almost no depth: SL3D_FLAG_ONLY_HORIZONTAL is for
     * rigs with a vertical baseline.  A context without these flags behaves exactly as before. */
    SL3D_FLAG_ONLY_VERTICAL = 1024u,
    SL3D_FLAG_ONLY_HORIZONTAL = 2048u,
    /* (0.20.0) The Gray decode against the FRINGE MEAN: a scan without the inverse Gray frames -- F + N frames per coded axis instead of
     * F + 2 N ("3 phase-shift + 10 Gray-code frames": 13 instead of 23 for one axis, 26 instead of 46 for two).  An extension: the
     * reference has no such mode.  Its fringe steps are Pi/2 apart (1/pattern_generator.cpp:302,342), so fringe frames 0 and 2 are half a
     * period apart and I0 + I2 is twice the pixel's mean intensity, the level halfway between a lit and a dark Gray stripe.  On such a
     * context bit i of stage 4's Gray decode of an axis is
     *   G_i = (2 * (int)gray_i - ((int)I0 + (int)I2) >= 0)        ties -> 1, as pos - inv >= 0 in 4/phase_unwrap.cpp:183
     * with gray_i the byte of Gray plane i and I0, I2 fringe bytes 0 and 2 of the same axis of the same view, as they sit in the frame
     * stack; the same rule for n_fringe 3 and 4 (with 5 nothing is valid, as always).  Everything after the bit is unchanged: the XOR
     * chain and code, the shifted wrapped phase, the absolute phase, stage 5, the anchored coordinate, the sub-pixel solves and the
     * residual.  The rule is pointwise: windows and the stripes of a group agree with the whole frame.
     *   The frame layout, planes_per_view, sl3d_device_buffers and the setters do not change: the inverse-Gray slots exist and nothing
     *   reads them.  sl3d_set_frames still takes F + 2 N planes; a caller without inverse frames uses sl3d_set_frames_range(view, axis,
     *   0, planes, F + N, stride).  sl3d_process_views and sl3d_group_process_views upload only the F + N planes of each coded axis,
     *   their contiguity test runs over those, and the pointers of the inverse planes may be NULL (with SL3D_FLAG_ONLY_VERTICAL /
     *   _HORIZONTAL so may all pointers of the other axis).  sl3d_synth_view, sl3d_get_frames, sl3d_copy_view, sl3d_set_masks_modulated
     *   and sl3d_get_modulation are unchanged.
     *   Without KEEP_STAGES: ONE launch of a kernel of its own (k_direct_gray<axes, anchored>, axes = 0: vertical only, 1: horizontal only,
     *   2: both axes) on the context's stream, behind the preparation of whatever masks are still deferred -- no launch lanes, every
     *   launch counts as on-stream, sl3d_camera_table_bytes_per_pixel is 0, sl3d_fused_kernel_name / sl3d_last_fused_kernel_name report
     *   "sl3d::k_direct_gray<0, false>" ... "sl3d::k_direct_gray<2, true>".  Per pixel, view and coded axis it reads F + N frame bytes.
     *   With both axes the residual plane is written as on any SL3D_FLAG_SUBPIXEL context; with one axis there is none.  Points, valid
     *   (and residuals) are bit for bit the staged route's.
     *   With KEEP_STAGES: sl3d_unwrap_phase decodes by the direct rule, the stage getters show the direct code, and sl3d_run() enqueues
     *   per view stage 3 and the direct stage 4 of each coded axis and stage 5, then one sub-pixel launch over the views (not the parity
     *   kernel, which reads the inverse planes).  sl3d_repair_periods works there as on any context: it touches the code and phase
     *   planes only.
     *   Refused with SL3D_E_UNSUPPORTED by sl3d_create and sl3d_group_create before a device is touched: the flag without
     *   SL3D_FLAG_SUBPIXEL (the integer scan's kernel reads the inverse frames: add SL3D_FLAG_SUBPIXEL); the flag with
     *   SL3D_FLAG_REPAIR_PERIODS (the fused repair has no direct form).  May be combined with SL3D_FLAG_KEEP_STAGES,
     *   SL3D_FLAG_ANCHOR_PERIODS, SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL, SL3D_FLAG_EAGER_MASK and SL3D_FLAG_SERIAL_LAUNCHES.
     *   sl3d_run_clouds stays refused as on every SL3D_FLAG_SUBPIXEL context.  sl3d_group_create hands the flag to its stripes.
     * On a lit pixel the two decodes agree (the mean sits between the stripe levels as the inverse frame does); on an unlit pixel under
     * noise both are noise and differ.  A context without the flag behaves exactly as before. */
    SL3D_FLAG_DIRECT_GRAY = 4096u
    /* (8u was SL3D_FLAG_CLOUDS_LOOKBACK until 0.3: contiguous clouds in one pass by a decoupled look-back between tiles.  Removed
     * in 0.4 -- every tile waited for its predecessors, 0.53 of the roofline against 0.67 for the segmented clouds; a consumer
     * that wants one contiguous device array asks sl3d_get_cloud_counts for it.) */
};

/* Replaces the compile-time macros and initialised globals of the reference:
 * PROJECT_GLOBAL/global_cv.h:49-53 (dimensions) and common_variables.h:6-10,23-24. */
typedef struct sl3d_config {
    int32_t width, height;            /* window processed by this context (pixels)                 */
    int32_t full_width, full_height;  /* Camera_imagewidth/height of the frame; 0 = same as window */
    int32_t col0, row0;               /* window origin inside the frame                            */
    int32_t proj_width, proj_height;  /* Projector_imagewidth / Projector_imageheight (fewer than 2^29 pixels) */
    int32_t n_fringe;                 /* number_of_patterns_fringe: 3 (or 4; 5 yields no valid pixel,
                                         exactly as 3/wrapped_phase.cpp:106-129 does)              */
    int32_t n_gray_v, n_gray_h;       /* number_of_patterns_binary_{vertical,horizontal}: 0..16; they need
                                         not be equal (the reference's own capture set is 6 / 5)   */
    int32_t fringe_width_v, fringe_width_h; /* fringe_width_pixels_{vertical,horizontal}           */
    int32_t n_codes_v, n_codes_h;     /* number_of_codes_* (stage-4 debug image only); 0 = ceil(P/fw) */
    int32_t max_views;                /* batch capacity: views resident in HBM at once (>= 1)      */
    int32_t device;                   /* HIP device ordinal                                        */
    uint32_t flags;                   /* sl3d_flags                                                */
    void *stream;                     /* hipStream_t to run on, or NULL: the context creates one   */
} sl3d_config;

/* Device-resident layout, for callers that produce frames / consume points on the GPU
 * (benchmarks, torch tensors, RCCL).  All pitches are in bytes unless noted. */
typedef struct sl3d_device_buffers {
    /* frames: view-major, then plane, then row.  Plane order inside a view:
     *   vertical   axis: fringe[0..F), gray[0..N_v), inverse_gray[0..N_v)
     *   horizontal axis: fringe[0..F), gray[0..N_h), inverse_gray[0..N_h)                         */
    uint8_t *frames;
    size_t frame_pitch;       /* bytes per row (multiple of 16, >= width)        */
    size_t plane_stride;      /* bytes per plane = frame_pitch * height          */
    size_t view_stride;       /* bytes per view  = planes_per_view * plane_stride */
    int32_t planes_per_view;  /* 2*F + 2*N_v + 2*N_h                              */
    /* selection mask with a 2-pixel halo; byte for window pixel (col,row) of a view is at
     * mask + view*mask_view_stride + (row + 2)*mask_pitch + 16 + col; bytes are 0 or 1.           */
    uint8_t *mask;
    size_t mask_pitch;
    size_t mask_view_stride;
    /* dense results of sl3d_run(): xyz as 3 consecutive floats per pixel (NaN where invalid);
     * pixel (col,row) of a view at points + view*points_view_stride + row*points_pitch + 12*col   */
    float *points;
    size_t points_pitch;        /* bytes per row = 12 * (frame_pitch)            */
    size_t points_view_stride;  /* bytes per view                                */
    uint8_t *valid;             /* merged valid map after stage 5, 0/1           */
    size_t valid_pitch;         /* bytes per row (= frame_pitch)                 */
    size_t valid_view_stride;   /* bytes per view                                */
} sl3d_device_buffers;

/* ---- library ------------------------------------------------------------------------------ */
const char *sl3d_version(void);
const char *sl3d_strerror(int status);
/* text of the last error on this context (HIP error string etc.); never NULL */
const char *sl3d_last_error(const sl3d_ctx *ctx);

/* ---- lifetime ----------------------------------------------------------------------------- */
/* Replaces the `new[]` allocations the reference performs inside every stage and never frees
 * (3/wrapped_phase.cpp:410-424, 4/phase_unwrap.cpp:282,300,373-376, 5/compute_correspondance.cpp:635-640,
 * 7/triangulation.cpp:1513): all buffers are owned by the context and released by sl3d_destroy. */
int sl3d_create(const sl3d_config *cfg, sl3d_ctx **out);
void sl3d_destroy(sl3d_ctx *ctx);

/* ---- inputs ------------------------------------------------------------------------------- */
/* The 8 calibration files read by read_parameters() 7/triangulation.cpp:149-180 and
 * compute_A() :1061-1126: intrinsics K (3x3 row-major), distortion (k1,k2,p1,p2,k3),
 * Rodrigues rotation vector and translation vector (world -> device) for camera and projector.
 * In the timed mode the call also builds, on the device, what the reference tabulates per scan (assign_3d_coordinates,
 * 7/triangulation.cpp:252-307, :352-378): the camera-side undistortion per window pixel and, for a distorted projector, either a
 * displacement per projector pixel or -- purely radial model, plain K: both projector calibrations the reference ships -- a 4-KB
 * table of the radial factor.  It synchronises the context's stream. */
int sl3d_set_calibration(sl3d_ctx *ctx,
                         const double Kc[9], const double dc[5], const double rc[3], const double tc[3],
                         const double Kp[9], const double dp[5], const double rp[3], const double tp[3]);

/* T0 as the library computed it from the last sl3d_set_calibration: the two 3x4 projection matrices A = K*[R|t] of compute_A()
 * (7/triangulation.cpp:1061-1126: cvRodrigues2 :1072,1080, [R|t] :1090-1099,1105-1114, cvMatMul :1101,1116), row-major doubles.
 * Host only.  With K = I the left 3x3 block is cvRodrigues2's matrix itself -- which is how tests/ compare the product's T0 with
 * the reference-held OpenCV answer (the two XML files under Triangulation/Relative_geometry, written by 6/system_calibration.cpp:1488-1516). */
int sl3d_get_projection_matrices(sl3d_ctx *ctx, double A_cam[12], double A_proj[12]);

/* selected_region of image_scissor() m_tech_project_console.cpp:146-238, handed over as a
 * FULL-FRAME row-major u8 plane (full_width x full_height); a pixel is selected iff byte == 1
 * (every consumer in the reference tests `== 1`).  The context copies its window plus a 2-pixel halo in ONE 2-D copy and
 * prepares it on the device (bytes normalised to 0/1, border band of the boundary removal evaluated by a kernel, the selected
 * quads counted -- a launch of a few sparsely selected views picks its kernel by that count): no host pass over the mask.  Pageable memory is consumed before the call returns; PINNED memory (sl3d_host_alloc) is read by
 * asynchronous DMA on the context's stream, so it must stay unchanged until the next synchronising call on the context
 * (any getter, sl3d_synchronize) -- the call then costs a copy and a launch (tens of microseconds at 1080p). */
int sl3d_set_mask(sl3d_ctx *ctx, int view, const uint8_t *full_frame_mask, size_t stride);

/* The same for n_views views [first_view, first_view + n_views) with ONE kernel launch: the mask of view first_view + k starts at
 * full_frame_masks + k * view_stride; view_stride == 0 hands every view the same mask (one copy, one launch).
 * The masks may also live in DEVICE memory of the context's GPU (an acquisition stage that segments on the GPU, a benchmark): with
 * 4-byte aligned rows (pointer, stride, view_stride, col0 and full_width multiples of 4) nothing is copied -- the kernels read the
 * caller's buffer, which must stay unchanged until the next synchronising call on the context (any getter, sl3d_synchronize),
 * like pinned host memory: with at most 4 views per call the selection is evaluated by the next launch over those views
 * (SL3D_FLAG_EAGER_MASK); otherwise the rows go through the staging plane by a device copy.  This is the per-scan device cost of image_scissor()'s result (m_tech_project_console.cpp:366) + stage
 * 3's boundary removal (3/wrapped_phase.cpp:253-279): bench.py `side.per_scan_device`. */
int sl3d_set_masks(sl3d_ctx *ctx, int first_view, int n_views, const uint8_t *full_frame_masks, size_t stride, size_t view_stride);

/* sl3d_set_masks with the fringe-modulation test that rejects shadow and background pixels (the criterion the reference wrote as
 * check_I_mod_criteria, 3/wrapped_phase.cpp:63-104, "another criteria to eliminate shadow+background", and left commented out).  Per
 * pixel and axis, from the three fringe bytes I0, I1, I2 of that axis as they sit in the view's frame stack:
 *     d = I0 - I2,  e = 2*I1 - I0 - I2,  gamma = sqrtf((float)(3*d*d + e*e)) / (float)(I0 + I1 + I2)     (float; I0 = I1 = I2 = 0: NaN)
 * and the view's selection is   (full_frame_masks == NULL || mask byte == 1) && (double)gamma_v > min_modulation && (double)gamma_h > min_modulation
 * (strict, in double, as 3/wrapped_phase.cpp:96; NaN never passes; the reference's default threshold is 0.01).  Stage 3's boundary
 * removal then runs on that selection exactly as on a lasso.  A deliberate difference from the reference: its (never run) code tests
 * each axis before that axis' own boundary removal; this library keeps ONE selection per view, so the two axes' tests are ANDed first.
 * The masks are handed over as for sl3d_set_masks (pageable, pinned or device memory, view_stride == 0: the same mask for every view;
 * the same lifetime rules) or not at all (NULL: every pixel is selected; stride and view_stride are then ignored), with one launch for
 * all views of the call.  Each view's selection is made from that view's frames as they are resident when the call is enqueued:
 * frames replaced afterwards do not change it -- set the frames first.  SL3D_E_UNSUPPORTED unless n_fringe == 3 and the window is the
 * whole frame (the 2-pixel halo of a window or row stripe lies in frames the context does not hold: derive the mask on a whole-frame
 * context with sl3d_get_modulation and hand it over with sl3d_set_mask / sl3d_group_set_mask); SL3D_E_INVALID_ARG for a NaN
 * threshold, bad views or strides.  A refused call leaves every view's previous selection as it was. */
int sl3d_set_masks_modulated(sl3d_ctx *ctx, int first_view, int n_views, double min_modulation, const uint8_t *full_frame_masks, size_t stride,
                             size_t view_stride);

/* gamma of one axis (0 = vertical, 1 = horizontal fringes) of one view as sl3d_set_masks_modulated computes it, window-sized row-major
 * floats (out[row * stride_elems + col], stride_elems >= width); NaN where I0 + I1 + I2 == 0.  Any window (gamma needs no halo);
 * n_fringe == 3 only (SL3D_E_UNSUPPORTED).  What a caller looks at to choose a threshold.  Synchronises. */
int sl3d_get_modulation(sl3d_ctx *ctx, int view, int axis, float *out, size_t stride_elems);

/* The captured frames of one axis of one view, window-sized planes in host memory: what
 * read_image() 3/wrapped_phase.cpp:29-58 (n_fringe planes) and read_captured_images()
 * 4/phase_unwrap.cpp:51-131 (n_gray planes + n_gray inverse planes) load.
 * planes[] order: fringe[0..F), gray[0..N), inverse_gray[0..N).  Planes that follow each other in host memory (plane i+1
 * at plane i + stride*height) go up as ONE 2-D copy per axis.  Pageable / pinned memory: as for sl3d_set_mask; planes in DEVICE
 * memory (another context's frame stack, sl3d_get_device_buffers) are copied device to device, asynchronously. */
int sl3d_set_frames(sl3d_ctx *ctx, int view, int axis, const uint8_t *const *planes, int n_planes, size_t stride);

/* selected_region exactly as the reference holds it: int [full_width][full_height], indexed [col][row]
 * (m_tech_project_console.cpp:146-238, common_variables.h), selected iff == 1.  The window's columns (+ halo) go up as one 2-D
 * copy and are transposed into the byte mask on the device; no pass of the host over the array. */
int sl3d_set_mask_colrow(sl3d_ctx *ctx, int view, const int32_t *selected_region);

/* n_planes planes of one axis starting at plane index first_plane of sl3d_set_frames' order (fringe[0..F), gray[0..N),
 * inverse_gray[0..N)): stage 3 loads only the F fringe frames (read_image, 3/wrapped_phase.cpp:29-58), stage 4 only the Gray /
 * inverse frames (read_captured_images, 4/phase_unwrap.cpp:51-131).  A SL3D_FLAG_DIRECT_GRAY context reads no inverse plane: first_plane 0
 * and n_planes F + N set all it needs. */
int sl3d_set_frames_range(sl3d_ctx *ctx, int view, int axis, int first_plane, const uint8_t *const *planes, int n_planes, size_t stride);

/* Device-to-device duplicate of one resident view (frame stack + mask) into another slot of the batch. */
int sl3d_copy_view(sl3d_ctx *ctx, int src_view, int dst_view);

/* (0.21.0) Exposure fusion on the device -- several exposures of one pattern set, one per view, fused into one ordinary view -- has a header
 * of its own, include/sl3d_fuse.h: the rule, SL3D_MAX_EXPOSURES and the two calls that work on a context of this header. */

/* (0.22.0) Outlier rejection of the dense scan on the device -- a radius filter over a view's points / valid planes, in place -- has a header
 * of its own, include/sl3d_filter.h: the rule, SL3D_FILTER_MAX_RADIUS and the two calls that work on a context of this header. */

/* (0.23.0) A voxel grid over the registered cloud (or any host cloud) on the device -- one point per occupied cell, its centroid -- has a
 * header of its own, include/sl3d_voxel.h: the rule, the two mode flags and the two calls that work on a context of this header. */

/* (0.24.0) The turntable's axis point and step angle -- the tx, ty, tz, rot_step of sl3d_register_views -- estimated from the scan itself, by
 * ICP with projective data association over consecutive views' dense planes, has a header of its own, include/sl3d_align.h: the rule of a
 * pass, the solve and the four calls. */

/* (0.25.0) The same refinement with the point-to-plane error metric -- the residual measured along the target's surface normal, which
 * removes the bias of the point-to-point form -- has a header of its own, include/sl3d_align_plane.h: dense normals of a view, the rule of
 * the pass, the solve and the five calls. */

/* (0.26.0) The views of a turntable scan fused into one oriented surface -- every view votes with a truncated signed distance into a
 * regular voxel volume on the device, the surface is the zero level of the averaged votes -- has a header of its own,
 * include/sl3d_tsdf.h: the rule of an integration, the rule of the extraction and the five calls. */

/* Synthetic capture generated on the device into view slot `view` (inputs for tests and benchmarks; the pattern
 * formulas are the reference generator's, 1/pattern_generator.cpp:80-105,302,313,497, Pi = 22/7): plane[3] = z0,a,b of
 * the scene plane Z = z0 + a*X + b*Y in the world frame of the calibration set with sl3d_set_calibration; camera
 * model I' = clamp(round(gain*I + offset + noise)), noise uniform in [-noise, noise] from a counter hash of
 * (seed, view_id, frame, row, col).  The mask is not touched. */
int sl3d_synth_view(sl3d_ctx *ctx, int view, const double plane[3], uint64_t seed, int view_id, int noise, float gain, float offset);
/* read the resident frames of one axis back (same plane order as sl3d_set_frames) */
int sl3d_get_frames(sl3d_ctx *ctx, int view, int axis, uint8_t *const *planes, int n_planes, size_t stride);

/* ---- the reference's four stage entry points (need SL3D_FLAG_KEEP_STAGES) ------------------- */
/* void compute_wrapped_phase(int pattern_type)   3/wrapped_phase.cpp:402   */
int sl3d_compute_wrapped_phase(sl3d_ctx *ctx, int view, int axis);
/* void unwrap_phase(int pattern_type)            4/phase_unwrap.cpp:367    (a SL3D_FLAG_DIRECT_GRAY context: the flag's Gray bit) */
int sl3d_unwrap_phase(sl3d_ctx *ctx, int view, int axis);
/* void compute_c_p_map()                         5/compute_correspondance.cpp:630 */
int sl3d_compute_c_p_map(sl3d_ctx *ctx, int view);
/* void triangulate()                             7/triangulation.cpp:1444  */
int sl3d_triangulate(sl3d_ctx *ctx, int view);

/* ---- 2*Pi period jumps of the absolute phase repaired (0.14.0; needs SL3D_FLAG_KEEP_STAGES) ----------------------------------------
 * The absolute phase is wrapped + Pi + 2*Pi*code (4/phase_unwrap.cpp:278-316), which is right only where the Gray-code period boundary
 * and the wrap of the fringe phase fall on the same camera pixel.  Defocus and the >= 0 tie rule of the Gray decode move the code edge by
 * a pixel or a few on a real rig: in that band the code is off by one, the correspondence by exactly fringe_width projector pixels.
 * This call takes whole periods out of one axis of one view, between stage 4 and stage 5, with no extra pattern.
 *   A SAMPLE of the axis is a pixel whose axis valid byte is 1 and that lies where stage 4 defines the absolute phase: window columns
 *   1..width-2 for the vertical axis, window rows 1..height-2 for the horizontal one.  The neighbourhood of a pixel is the 2*radius + 1
 *   pixels along the direction the axis encodes (the row for the vertical axis, the column for the horizontal one), the pixel included,
 *   clipped to the context's window.  For every sample p, from the planes as they were when the call was enqueued (every pixel decides
 *   from the same state, not from its neighbours' repairs):
 *     1. S = the absolute phases of the samples of its neighbourhood, n = |S|;  n < radius + 1: p is left as it is
 *     2. m = the lower median of S (element (n - 1) / 2 of S sorted ascending)
 *     3. j = (long)rint(((double)unwrapped_p - (double)m) / ((2.0 * 22.0) / 7.0)), half to even;  j == 0: p is left as it is
 *     4. k = code_p - j;  k < 0 or k >= 2^n_gray: p is left as it is and counted as unrepairable
 *     5. code_p = k, unwrapped_p = (float)((double)wrapped_p + (((double)k * 2.0) * 22.0) / 7.0) (stage 4's expression), counted as repaired
 *   The wrapped phase, the valid maps and the stage-4 debug image are not touched.  An integer correction and one recomputation by the
 *   reference's own formula: bit-for-bit reproducible.  A second call is a second pass over the result of the first.
 * Call order: sl3d_compute_wrapped_phase and sl3d_unwrap_phase of both axes, sl3d_repair_periods per axis, sl3d_compute_c_p_map,
 * sl3d_triangulate -- everything downstream (sl3d_get_points, the clouds, the meshes) then sees the repaired scan.  After sl3d_run on a
 * KEEP_STAGES context the same planes exist, so sl3d_repair_periods + sl3d_compute_c_p_map + sl3d_triangulate works there too.
 * counts[0] = repaired, counts[1] = unrepairable pixels of this pass; counts may be NULL (then the call stays asynchronous), otherwise the
 * call synchronises.  SL3D_E_INVALID_ARG for a bad view, an axis outside {0, 1} or a radius outside 1..8; SL3D_E_STATE without
 * SL3D_FLAG_KEEP_STAGES; SL3D_E_UNSUPPORTED if the axis has no Gray planes, on a SL3D_FLAG_ANCHOR_PERIODS context (see the flag), or on
 * the axis a SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL context does not code.  A refused call changes nothing. */
int sl3d_repair_periods(sl3d_ctx *ctx, int view, int axis, int radius, uint32_t counts[2]);

/* ---- sub-pixel triangulation with a reprojection residual (0.15.0; needs SL3D_FLAG_KEEP_STAGES -- the timed mode has it as SL3D_FLAG_SUBPIXEL) --
 * Stage 5 rounds every projector coordinate to an integer (lrint, 5/compute_correspondance.cpp:648,659) before stage 7 triangulates
 * from it: up to half a projector pixel per axis, which shows as depth terraces in every surface built on the scan.  This call is an
 * alternative to sl3d_triangulate, after sl3d_compute_c_p_map, that triangulates from the doubles lrint was handed instead.  c_p_map
 * and the parity contract are not touched.  All views of a call are triangulated by ONE launch.  For every window pixel of views
 * [first_view, first_view + n_views) whose merged valid byte is 1:
 *   1. xs = (double)fringe_width_v * ((double)unwrapped_v / ((2.0 * 22.0) / 7.0)), ys likewise from the horizontal axis: exactly the
 *      arguments of stage 5's lrint, so rint(xs), rint(ys) is the pixel's c_p_map entry
 *   2. (u, v) = the camera pixel, (u', v') = (xs, ys), each undistorted (the five iterations of cvUndistortPoints, the projector's at the
 *      continuous point) and re-projected by its K, as stage 7 does with the integers
 *   3. X = the least-squares point of stage 7's 4 x 3 system at (u, v, u', v'), with its rule X = 0 where the determinant is 0
 *   4. per device D with projection matrix A_D (sl3d_get_projection_matrices): h = A_D * (X, 1), e_D = (h0/h2 - u_D, h1/h2 - v_D);
 *      residual = (float)sqrt(e_cam . e_cam + e_proj . e_proj): the reprojection error in undistorted pixels, camera and projector
 *      together -- the one degree of freedom the system has to spare, a consistency measure of the two decoded axes.  (It does not see
 *      every wrong decode: a period error along the epipolar direction leaves it small.  It is no replacement for sl3d_repair_periods.)
 *   5. only if max_residual is finite: the pixel is rejected iff !((double)residual <= max_residual), decided on the stored float
 *   6. points = (float)X, intersection_points = X, the residual plane = residual; a rejected pixel gets merged valid 0, points NaN,
 *      intersection_points 0 and keeps its residual.  Every other pixel of those views gets points NaN, intersection_points 0, residual
 *      NaN, as after sl3d_triangulate.  c_p_map, the per-axis planes and the per-axis valid maps are not touched.
 * Everything that reads the dense result (sl3d_get_points, sl3d_compact_views, sl3d_get_cloud, the meshes and their consumers) then sees
 * the sub-pixel scan.  sl3d_compute_c_p_map undoes the rejections; sl3d_compute_c_p_map + sl3d_triangulate restores the integer result.
 * Works after sl3d_run on a KEEP_STAGES context, and after sl3d_repair_periods + sl3d_compute_c_p_map.
 * counts: NULL (the call stays asynchronous) or n_views pairs; counts[2k] = pixels of view first_view + k triangulated (merged valid 1 on
 * entry), counts[2k + 1] = those of them rejected; then a second small launch adds them up and the call synchronises.
 * SL3D_E_INVALID_ARG for bad views or a max_residual that is NaN or <= 0 (+infinity: no pixel is rejected); SL3D_E_STATE without
 * SL3D_FLAG_KEEP_STAGES or before sl3d_set_calibration.  A refused call changes nothing.
 * On a SL3D_FLAG_ANCHOR_PERIODS context (xs, ys) of step 1 are the anchored coordinates (see the flag); everything else is as above.
 * On a SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL context: the exactly determined one-axis solve instead (see the flags) -- no
 * residual plane; a finite max_residual is SL3D_E_UNSUPPORTED and changes nothing; counts = (triangulated, 0). */
int sl3d_triangulate_subpixel(sl3d_ctx *ctx, int first_view, int n_views, double max_residual, uint32_t *counts);
/* The residual plane of a view, out[row * stride_elems + col]: NaN on every pixel the last sl3d_triangulate_subpixel over the view did
 * not triangulate (and on a view none has run over).  SL3D_E_STATE before the context's first sl3d_triangulate_subpixel.
 * On a SL3D_FLAG_SUBPIXEL context sl3d_run writes the plane too (it exists from sl3d_create on): SL3D_E_STATE before the first sl3d_run
 * (with KEEP_STAGES: before the first sl3d_run or sl3d_triangulate_subpixel), the text names the missing call. */
int sl3d_get_residuals(sl3d_ctx *ctx, int view, float *out, size_t stride_elems);
/* (xs, ys) of step 1 for every window pixel, xy[(row * stride_elems + col) * 2 + {0, 1}], bit for bit those expressions; NaN where
 * either per-axis valid byte is not 1 (the pixels stage 5 does not form them for).  Computed from the stage-4 planes as they are: no
 * sl3d_compute_c_p_map is needed, a rejection does not show.  SL3D_E_STATE without SL3D_FLAG_KEEP_STAGES.  On a
 * SL3D_FLAG_ANCHOR_PERIODS context: the anchored coordinates, bit for bit the flag's definition (same NaN pattern).  On a one-axis
 * context (SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL): the coordinate of the coded axis, NaN in the other component.
 * sl3d_get_residuals on such a context: SL3D_E_UNSUPPORTED, there are none. */
int sl3d_get_correspondences_subpixel(sl3d_ctx *ctx, int view, double *xy, size_t stride_elems);

/* ---- the fused hot path ------------------------------------------------------------------- */
/* Stages 3(v) 3(h) 4(v) 4(h) 5 7 in main()'s order (m_tech_project_console.cpp:372-395) plus the
 * float cast of 8/save_point_cloud.cpp:100-102, for views [first_view, first_view+n_views), as ONE
 * kernel launch that reads every frame byte once and writes xyz (f32) + valid (u8). Asynchronous.
 * On a SL3D_FLAG_SUBPIXEL context: the sub-pixel scan and its residual plane instead (see the flag) -- still one launch per call
 * without KEEP_STAGES, the parity launch + sl3d_triangulate_subpixel's with it.  On a SL3D_FLAG_REPAIR_PERIODS context: the scan with
 * the period jumps of both axes repaired (see the flag), one launch per call without KEEP_STAGES as well.  On a SL3D_FLAG_DIRECT_GRAY
 * context: the Gray frames against the fringe mean, no inverse frame read (see the flag), one launch per call without KEEP_STAGES. */
int sl3d_run(sl3d_ctx *ctx, int first_view, int n_views);
/* The same pass with the compaction of 8/save_point_cloud.cpp:33-37,85-104 INSIDE the kernel: instead of the dense xyz plane every
 * view's valid points are written once, compacted in the reference's row-major scan order, plus the valid map:
 * ~47 + 12*valid_fraction + 1 bytes per pixel instead of 60 for the dense pass + 25 for a separate compaction.  Timed mode only
 * (no SL3D_FLAG_KEEP_STAGES), and the integer scan only: SL3D_E_UNSUPPORTED on a SL3D_FLAG_SUBPIXEL or SL3D_FLAG_REPAIR_PERIODS context, nothing
 * changed (sl3d_run + sl3d_compact_views give its clouds).  Asynchronous.
 *   SEGMENTED clouds.  Every wave of the kernel compacts the 256 consecutive scan pixels it owns into its own fixed slot
 *   (points [256*s, 256*s + count_s) of the view's region) and stores count_s.  The counts become offsets by a small scan kernel
 *   right behind a launch of more than 4 views; a launch of up to 4 views -- the reference's one scan per call -- leaves the scan
 *   to its consumer (the gap-closing kernel adds up the counts in front of its segments on entry; sl3d_get_cloud_segments and
 *   sl3d_register_clouds, which want the offsets as an array, run the scan kernel when they are called).
 *   No tile ever waits for another one, scan order is preserved inside and across segments, so a view's cloud is the
 *   concatenation of its segments -- and the consumers that exist anyway close the gaps for free: sl3d_download_clouds (host
 *   copy), sl3d_register_clouds (turntable registration), the pack before a group's RCCL send, or any device consumer through
 *   sl3d_get_cloud_segments.
 * sl3d_get_cloud_counts synchronises and returns, for views [first_view, first_view+n_views), the number of points of each
 * cloud; with device_xyz != NULL also a CONTIGUOUS device copy: view first_view+k's cloud is counts[k] points (3 floats each) at
 * *device_xyz + 3*k*(*view_stride_points), valid until the next sl3d_run_clouds / sl3d_compact_views on this context (produced
 * on demand by one gap-closing launch; pass NULL if only the counts are wanted). */
int sl3d_run_clouds(sl3d_ctx *ctx, int first_view, int n_views);
int sl3d_get_cloud_counts(sl3d_ctx *ctx, int first_view, int n_views, const float **device_xyz, size_t *view_stride_points, int64_t *counts);

/* The segmented clouds themselves, for consumers that stay on the device:
 * segment s of view first_view+k holds counts[k*view_stride_segments + s] points at xyz + 3*(k*view_stride_points +
 * s*segment_points); its first point is point number offsets[k*view_stride_segments + s] of the view's cloud. */
typedef struct sl3d_cloud_segments {
    const float *xyz;
    const uint32_t *counts;
    const uint64_t *offsets;
    int32_t n_segments;            /* per view */
    int32_t segment_points;        /* point slots per segment (256) */
    size_t view_stride_points;
    size_t view_stride_segments;   /* = n_segments */
} sl3d_cloud_segments;
int sl3d_get_cloud_segments(sl3d_ctx *ctx, int first_view, int n_views, sl3d_cloud_segments *out, int64_t *counts);

/* The reference's consumer is the host (8/save_point_cloud.cpp:85-104 fills a host pcl::PointCloud): the clouds of views
 * [first_view, first_view+n_views) of the last sl3d_run_clouds, back to back in host memory (at most `capacity` points in all;
 * xyz may be NULL: counts only).  Pinned memory (sl3d_host_alloc): the gap-closing kernel writes the host buffer directly;
 * otherwise a contiguous device copy is downloaded.  Synchronises. */
int sl3d_download_clouds(sl3d_ctx *ctx, int first_view, int n_views, float *xyz, int64_t capacity, int64_t *counts);

/* sl3d_register_views on the clouds of the last sl3d_run_clouds (no dense planes, no separate compaction): the rotation of
 * 9/register_point_clouds.cpp:83-128 is applied while the segments are concatenated. */
int sl3d_register_clouds(sl3d_ctx *ctx, int first_view, int n_views, float tx, float ty, float tz, float rot_step, float *xyz, int64_t capacity,
                         int64_t *total);
/* Name of the fused-kernel instantiation sl3d_run (clouds = 0) / sl3d_run_clouds (clouds = 1) launches for a batch of n_views views
 * with this context's configuration and calibration, spelled as rocprofv3 --kernel-trace prints it: benchmarks name the kernel
 * their roofline figure is about without restating the library's dispatch rules.  On a SL3D_FLAG_SUBPIXEL context without KEEP_STAGES
 * this, and sl3d_last_fused_kernel_name after the first sl3d_run, is "sl3d::k_subpixel_fused<false>" -- "sl3d::k_subpixel_fused<true>" with
 * SL3D_FLAG_ANCHOR_PERIODS -- (clouds = 1: SL3D_E_UNSUPPORTED), and sl3d_camera_table_bytes_per_pixel is 0: that kernel reads no table.  On a SL3D_FLAG_REPAIR_PERIODS context without KEEP_STAGES the same
 * holds with "sl3d::k_repair_fused<false>", or "sl3d::k_repair_fused<true>" if the context has SL3D_FLAG_SUBPIXEL too. */
int sl3d_fused_kernel_name(sl3d_ctx *ctx, int n_views, int clouds, char *buf, size_t capacity);
/* The instantiation the LAST fused launch of this context ran (sl3d_run, sl3d_run_clouds, sl3d_run_timed, sl3d_process_views): the
 * choice is recorded when the launch is made -- it depends on what was known about the views' masks at that moment (a small
 * launch over sparsely selected views takes another kernel; while the count of a selection is still on its way from the device, the
 * last count of that view that did arrive decides), so a later prediction could name a different one.  The choice never changes a
 * bit of the results. */
int sl3d_last_fused_kernel_name(sl3d_ctx *ctx, char *buf, size_t capacity);
/* How many fused launches of this context went to the context's stream and how many to its launch lanes (SL3D_FLAG_SERIAL_LAUNCHES):
 * what a benchmark or a test states beside a per-launch time of a series.  Either pointer may be NULL.  Touches nothing on the device. */
int sl3d_launch_counts(sl3d_ctx *ctx, int64_t *on_stream, int64_t *on_lanes);
/* Bytes per camera pixel a fused launch of n_views views reads from the camera-side table of sl3d_set_calibration (T1 per window pixel,
 * 7/triangulation.cpp:252-307), once per LAUNCH whatever the number of views: 0 = no table (no camera distortion, parity mode),
 * 8 = the radial factor as a double, 16 = the normalised point (tangential terms).  Benchmarks state the bytes a launch moves beside
 * the algorithmic ones with it.  < 0: error. */
int sl3d_camera_table_bytes_per_pixel(sl3d_ctx *ctx, int n_views);
/* sl3d_run bracketed by HIP events on the context's stream; returns the kernel time of this launch */
int sl3d_run_timed(sl3d_ctx *ctx, int first_view, int n_views, float *kernel_ms);
int sl3d_synchronize(sl3d_ctx *ctx);
/* HIP-event stopwatch on the context's stream (the stream the kernels are launched on): start
 * records an event, stop records a second one, waits for it and returns the elapsed device time
 * between the two -- used to time a whole region of back-to-back launches without host syncs. */
int sl3d_timer_start(sl3d_ctx *ctx);
int sl3d_timer_stop(sl3d_ctx *ctx, float *elapsed_ms);

/* ---- outputs (all synchronise the stream first; planes are window-sized, row-major) --------- */
/* valid_map_vertical / _horizontal / valid_map  (int[W][H] in the reference), as 0/1 bytes */
int sl3d_get_valid_map(sl3d_ctx *ctx, int view, int which, uint8_t *out, size_t stride);
/* wrapped_phi_{vertical,horizontal}: after stage 3 the atan2 phase, after stage 4 shifted by
 * +Pi in place on unwrapped pixels, as the reference does (4/phase_unwrap.cpp:290,308) */
int sl3d_get_wrapped_phase(sl3d_ctx *ctx, int view, int axis, float *out, size_t stride_elems);
int sl3d_get_unwrapped_phase(sl3d_ctx *ctx, int view, int axis, float *out, size_t stride_elems);
/* code_{vertical,horizontal}: Gray-decoded period index, -1 where invalid (4/phase_unwrap.cpp:143) */
int sl3d_get_code(sl3d_ctx *ctx, int view, int axis, int32_t *out, size_t stride_elems);
/* the 8-bit debug images of stage 3 (3/wrapped_phase.cpp:178-179,274) and stage 4
 * (4/phase_unwrap.cpp:334-335): the reference's known-answer images are these */
int sl3d_get_debug_image(sl3d_ctx *ctx, int view, int stage, int axis, uint8_t *out, size_t stride);
/* c_p_map: long[W*H][2] indexed [row*W+col] (common_variables.h:15), zeros where invalid */
int sl3d_get_c_p_map(sl3d_ctx *ctx, int view, int64_t *out);
/* intersection_points as row-major double [H][W][3] (the reference stores [col][row][3]) */
int sl3d_get_intersection_points(sl3d_ctx *ctx, int view, double *out);
/* dense f32 points [H][W][3] (NaN where invalid) + merged valid map [H][W]; either may be NULL */
int sl3d_get_points(sl3d_ctx *ctx, int view, float *xyz, uint8_t *valid);
/* One of the reference's image-shaped globals in the reference's OWN layout and types (common_variables.h:12-21,56-62: every one
 * is indexed [col][row]): transposed and converted on the device, then ONE contiguous copy into the caller's array.
 *   which: SL3D_G_VALID_V / _H / SL3D_G_VALID -> int [W][H]; SL3D_G_WRAPPED_V / _H, SL3D_G_UNWRAPPED_V / _H -> float [W][H];
 *          SL3D_G_CODE_V / _H -> int [W][H]; SL3D_G_INTERSECTION_POINTS -> double [W][H][3]
 *   out: element (col, row) of this context's window is written at out[col * out_height + out_row0 + row]: a whole-frame
 *        context passes (height, 0); a row stripe of a taller array passes the array's height and its own first row, and
 *        writes only its rows of every column.  Needs SL3D_FLAG_KEEP_STAGES.  Synchronises. */
enum sl3d_global {
    SL3D_G_VALID_V = 0, SL3D_G_VALID_H = 1, SL3D_G_VALID = 2, SL3D_G_WRAPPED_V = 3, SL3D_G_WRAPPED_H = 4,
    SL3D_G_UNWRAPPED_V = 5, SL3D_G_UNWRAPPED_H = 6, SL3D_G_CODE_V = 7, SL3D_G_CODE_H = 8, SL3D_G_INTERSECTION_POINTS = 9,
    /* double [W][H][3] like SL3D_G_INTERSECTION_POINTS, but the dense f32 result of sl3d_run widened to double (NaN where invalid):
     * what a context WITHOUT SL3D_FLAG_KEEP_STAGES has of intersection_points -- the very values 8/save_point_cloud.cpp:94-96
     * casts them to, i.e. all that the reference's only reader of that global ever sees (like SL3D_G_VALID, no KEEP_STAGES needed) */
    SL3D_G_POINTS_F64 = 10
};
int sl3d_get_global_colrow(sl3d_ctx *ctx, int view, int which, void *out, int out_height, int out_row0);

/* the compacted cloud of 8/save_point_cloud.cpp:85-104: valid points in row-major scan order;
 * writes at most `capacity` points, always returns the total count in *count */
int sl3d_get_cloud(sl3d_ctx *ctx, int view, float *xyz, int64_t capacity, int64_t *count);

/* save_point_cloud() colours every point with the pixel of a camera image (cvLoadImage("Point_cloud/texture.bmp"), split
 * into blue/green/red, 8/save_point_cloud.cpp:46-52,70-72): sl3d_set_texture uploads that image for a view (window-sized,
 * B,G,R interleaved as cvLoadImage returns it, `stride` bytes per row); sl3d_get_cloud_rgb returns the compacted cloud and
 * r,g,b per point, gathered on the device in the same scan order. */
int sl3d_set_texture(sl3d_ctx *ctx, int view, const uint8_t *bgr, size_t stride);
int sl3d_get_cloud_rgb(sl3d_ctx *ctx, int view, float *xyz, uint8_t *rgb, int64_t capacity, int64_t *count);

/* the same compaction left on the device (valid until the next sl3d_compact / sl3d_get_cloud on this context):
 * *device_xyz points at count*3 floats in HBM; the count comes back to the host */
int sl3d_compact(sl3d_ctx *ctx, int view, const float **device_xyz, int64_t *count);

/* the compaction of views [first_view, first_view+n_views) in one go (three launches, one read-back of the counts):
 * view first_view+k's cloud is counts[k] points at *device_xyz + 3*k*(*view_stride_points) floats, valid until the next
 * sl3d_compact_views on this context */
int sl3d_compact_views(sl3d_ctx *ctx, int first_view, int n_views, const float **device_xyz, size_t *view_stride_points, int64_t *counts);
/* the same with a host copy: the clouds back to back in xyz (at most `capacity` points in all; xyz may be NULL) */
int sl3d_get_clouds(sl3d_ctx *ctx, int first_view, int n_views, float *xyz, int64_t capacity, int64_t *counts);

/* ---- the mesh of a view: ordered faces over the compacted cloud (0.8.0) ------------------------------------------
 * The dense result of a view is an organized grid, one point per camera pixel; the mesh connects neighbouring valid pixels
 * unless an edge longer than max_edge (mm, > 0, +inf allowed) lies between them.  The reference has no such stage (its user
 * meshed the PLY of stage 8 by hand); the definition is this library's own and exact:
 *   vertices  the compacted cloud of sl3d_get_cloud: the valid pixels in row-major scan order, id = position in that cloud
 *   len2(p,q) (dx*dx + dy*dy) + dz*dz of the float coordinates widened to double; an edge is short iff len2 <= max_edge^2
 *             (in double; NaN is not short).  A NaN the arithmetic produces only ever enters these comparisons: its sign and payload
 *             are not part of the definition; the vertices are copies and keep the bits of whatever lies under a valid pixel.
 *   cells     r in [0, height-1), c in [0, width-1): corners a = (r,c), b = (r,c+1), d = (r+1,c), e = (r+1,c+1).
 *             4 valid corners: diagonal a-e iff len2(a,e) <= len2(b,d), candidates (a,d,e) then (a,e,b); else b-d, candidates
 *             (a,d,b) then (b,d,e).  3 valid corners: e missing (a,d,b); a missing (b,d,e); b missing (a,d,e); d missing (a,e,b).
 *   faces     the candidates whose three edges are short, cell by cell in row-major order, a cell's faces in the order above;
 *             three int32 vertex ids each, at most 2*(width-1)*(height-1) per view.  One orientation throughout.
 * Deterministic: the result does not depend on the batch a view is meshed in or on the run.
 * Works wherever sl3d_compact_views works (every context with a dense result: timed, parity, windows); ids are relative to the
 * view's own cloud; points, valid and whatever sl3d_compact* / sl3d_run_clouds handed out are not modified.
 * Not covered: groups (sl3d_group_*: the cells across a stripe seam need the neighbour's row), a mesh straight from the segments of
 * sl3d_run_clouds, registration of meshes, the drop-in shim (the reference has nothing to mirror).  Vertex normals: below (0.9.0). */
typedef struct sl3d_mesh {            /* device-resident, valid until the next sl3d_mesh_views / sl3d_get_meshes on this context */
    const float *xyz;                 /* view first_view+k: n_vertices[k] points  at xyz   + 3*k*view_stride_points */
    const int32_t *faces;             /* view first_view+k: n_faces[k] id triples at faces + 3*k*view_stride_faces  */
    size_t view_stride_points, view_stride_faces;
} sl3d_mesh;
/* meshes views [first_view, first_view+n_views) on the device (six launches, one read-back of the counts); device_mesh may be NULL.
 * A NaN or non-positive max_edge, a bad view range or NULL counts: SL3D_E_INVALID_ARG, and nothing on the device changes. */
int sl3d_mesh_views(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, sl3d_mesh *device_mesh, int64_t *n_vertices, int64_t *n_faces);
/* the same with a host copy: the clouds back to back in xyz (at most vertex_capacity points in all), then the faces back to back
 * in faces (at most face_capacity triples in all); xyz / faces may be NULL; the per-view counts are always returned */
int sl3d_get_meshes(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, float *xyz, int64_t vertex_capacity, int32_t *faces,
                    int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces);

/* ---- vertex normals of a view's mesh (0.9.0) ------------------------------------------------------------------------
 * One normal per vertex of the mesh sl3d_mesh_views(first_view, n_views, max_edge) defines, computed on the device from the dense
 * result alone (a vertex's faces lie in the four cells around its pixel: a gather, no atomics, no adjacency lists).  Exact:
 *   face vector  face (i,j,k) in the order the face list gives its ids, points p,q,s widened to double: u = q-p, v = s-p,
 *                fn = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x), every product and difference one IEEE double
 *                operation, no contraction: the area-weighted face normal; every vertex of the face accumulates the same value
 *   vertex sum   acc = (+0,+0,+0), then acc += fn for every face that contains the vertex, in the order of the view's face list: for
 *                the vertex at pixel (r,c) the cells (r-1,c-1), (r-1,c), (r,c-1), (r,c), within a cell the cell's face order (<= 8 faces)
 *   normal       ss = (acc.x*acc.x + acc.y*acc.y) + acc.z*acc.z; if 0 < ss < +inf: n = (float)(acc / sqrt(ss)) per component (sqrt and
 *                division correctly rounded in double, the cast to nearest even); otherwise n = (+0,+0,+0): a vertex in no face,
 *                degenerate faces, an overflow, a NaN or infinity under a valid pixel.  Where the arithmetic PRODUCES a NaN (none
 *                reaches a normal: NaN sums give +0), its sign and payload are not part of the definition.
 *   orientation  follows the faces: for points (x,y,z) = (col, row, f(col,row)) the normal is (f_x, f_y, -1)/|..|.  Nothing is flipped
 *                towards the camera: that choice is the caller's.
 *   output       one float triple per vertex in vertex-id order (the order of sl3d_get_cloud); deterministic as the faces are.
 * Works wherever sl3d_mesh_views works (timed and parity contexts, windows: cells end at the window).  The normals live in a buffer of
 * their own (allocated on first use): points, valid, the clouds of sl3d_compact* / sl3d_run_clouds and the device mesh of the last
 * sl3d_mesh_views are not modified and stay valid.  A NaN or non-positive max_edge, a bad view range or NULL n_vertices:
 * SL3D_E_INVALID_ARG, and nothing on the device changes.  Not covered: as for the mesh. */
/* normals of the meshes sl3d_mesh_views(first_view, n_views, max_edge) defines; view first_view+k: n_vertices[k] float triples at
 * *device_normals + 3*k*(*view_stride_points), valid until the next sl3d_mesh_normals / sl3d_get_mesh_normals on this context
 * (three launches, one read-back of the counts; device_normals / view_stride_points may be NULL) */
int sl3d_mesh_normals(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, const float **device_normals,
                      size_t *view_stride_points, int64_t *n_vertices);
/* the same with a host copy, back to back, at most vertex_capacity triples in all; normals may be NULL (counts only) */
int sl3d_get_mesh_normals(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, float *normals, int64_t vertex_capacity,
                          int64_t *n_vertices);

/* ---- connected components of a view's mesh, and the mesh without its small components (0.10.0) --------------------------------
 * The mesh of a real scan is one object plus hundreds of fragments; this labels them on the device and drops the small ones.  The
 * mesh is the one sl3d_mesh_views(first_view, n_views, max_edge) defines: vertices = the valid pixels in scan order, faces as there.
 *   component     two vertices are connected iff they share a face; components are the transitive closure.  A vertex that is in no
 *                 face is a component of its own, of size 1.
 *   label         the smallest vertex id of the vertex's component: one int32 per vertex in vertex-id order.  A component's root is
 *                 the vertex whose label is its own id.
 *   n_components  the number of roots, singletons included.
 *   size          the number of vertices of the component.
 *   filtered mesh for min_vertices >= 1, a sub-mesh of the original: the vertices whose component has size >= min_vertices, in scan
 *                 order, renumbered 0..n'; the original faces whose vertices are kept (a face's three vertices share a component: any
 *                 and all coincide), in the original order, with the new ids; vertex_ids[i] = the original id of new vertex i,
 *                 ascending.  min_vertices = 1 gives the mesh itself.
 * The filtered mesh is NOT the mesh of the filtered valid map: take a cell with four valid corners in which len2(a,e) <= len2(b,d) <=
 * max_edge^2 and d-e and b-e are long -- it has no face; with e dropped from the valid map the three-corner rule would invent the face
 * (a,d,b).  The face list is filtered, never derived again.
 * Gathers through vertex_ids are exact: every face of a kept vertex is kept, so the normals of the filtered mesh are
 * normals[vertex_ids] of sl3d_mesh_normals and its colours rgb[vertex_ids] of sl3d_get_cloud_rgb -- no filtered form of either exists
 * or is needed.
 * Labels are integers fixed by the definition: the result is the same bit for bit whatever the batch, the launch shape or the run.
 * Works wherever sl3d_mesh_views works (timed and parity contexts, windows: cells end at the window).  Everything lives in buffers of
 * its own (allocated on first use): points, valid, the clouds of sl3d_compact* / sl3d_run_clouds, the device mesh of the last
 * sl3d_mesh_views and the normals of the last sl3d_mesh_normals are not modified and stay valid.  A NaN or non-positive max_edge,
 * min_vertices < 1, a bad view range or NULL count pointers: SL3D_E_INVALID_ARG, and nothing on the device changes.  A fixed sequence
 * of launches, no launch depends on the data; should a label walk ever exceed its iteration bound (a logic error) the call returns
 * SL3D_E_INTERNAL with a text.  Not covered: as for the mesh (groups, segments, the shim). */
/* labels of the meshes of views [first_view, first_view+n_views): view first_view+k has n_vertices[k] int32 labels at *device_labels +
 * k*(*view_stride_points) and n_components[k] components; valid until the next sl3d_mesh_components / sl3d_get_mesh_components on this
 * context (five launches, one read-back of the counts; device_labels / view_stride_points may be NULL) */
int sl3d_mesh_components(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, const int32_t **device_labels,
                         size_t *view_stride_points, int64_t *n_vertices, int64_t *n_components);
/* the same with a host copy, back to back, at most vertex_capacity labels in all; labels may be NULL (counts only) */
int sl3d_get_mesh_components(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int32_t *labels, int64_t vertex_capacity,
                             int64_t *n_vertices, int64_t *n_components);
typedef struct sl3d_mesh_filtered {   /* device-resident, valid until the next sl3d_mesh_views_filtered / sl3d_get_meshes_filtered */
    const float *xyz;                 /* view first_view+k: n_vertices[k] points       at xyz        + 3*k*view_stride_points */
    const int32_t *faces;             /* view first_view+k: n_faces[k] new-id triples  at faces      + 3*k*view_stride_faces  */
    const int32_t *vertex_ids;        /* view first_view+k: n_vertices[k] original ids at vertex_ids + k*view_stride_points   */
    size_t view_stride_points, view_stride_faces;
} sl3d_mesh_filtered;
/* the filtered meshes of views [first_view, first_view+n_views) on the device (seven launches, one read-back of the counts);
 * device_mesh may be NULL */
int sl3d_mesh_views_filtered(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int64_t min_vertices,
                             sl3d_mesh_filtered *device_mesh, int64_t *n_vertices, int64_t *n_faces);
/* the same with a host copy under the capacity contract of sl3d_get_meshes: points in xyz and original ids in vertex_ids (at most
 * vertex_capacity of each in all), faces in faces (at most face_capacity triples in all); any of the three may be NULL */
int sl3d_get_meshes_filtered(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int64_t min_vertices, float *xyz,
                             int32_t *vertex_ids, int64_t vertex_capacity, int32_t *faces, int64_t face_capacity, int64_t *n_vertices,
                             int64_t *n_faces);

/* ---- smoothed vertex positions of a view's mesh, and the normals of the smoothed mesh (0.11.0) -----------------------------------
 * The phase noise of a scan is of the order of its sample spacing, and the normals of sl3d_mesh_normals are the normals of that noise;
 * this smooths the vertices on the device by Taubin's lambda|mu steps over the 1-ring.  Let M = (vertices, faces) be the mesh
 * sl3d_mesh_views(first_view, n_views, max_edge) defines.  The faces and the vertex ids do not change; the connectivity is taken once,
 * from the original positions.  Exact:
 *   neighbours  two vertices are neighbours iff some face contains both: 0..8 of them, among the 8 pixels around the vertex's own.
 *   boundary    an edge is a boundary edge iff exactly one face contains it (no edge lies in more than two faces); a boundary vertex is
 *               an endpoint of a boundary edge.
 *   one step    with factor f (a double: the float argument widened) reads positions p as float32 and writes p' as float32.  A vertex
 *               with k >= 1 neighbours that is not fixed, per component: s = the neighbours' coordinates widened to double, added one
 *               after the other in ascending vertex id, starting from +0; m = s / (double)k; p' = (float)((double)p + f * (m - (double)p)).
 *               Every +, -, *, / is one IEEE double operation, nothing contracted; the cast rounds to nearest even.  Ascending vertex id
 *               is the pixels' scan order: (r-1,c-1), (r-1,c), (r-1,c+1), (r,c-1), (r,c+1), (r+1,c-1), (r+1,c), (r+1,c+1).  A vertex with
 *               k = 0, or a fixed one, keeps p' = p bitwise.  All vertices of a step read the positions of the step before (Jacobi).  No
 *               special case for a NaN or infinity under a valid pixel: the arithmetic above is all there is.  The sign and payload of a
 *               NaN the arithmetic PRODUCES (inf - inf after a step left the float range, ...) are not part of the definition; a NaN that
 *               is copied (p' = p) keeps its bits.
 *   iterations  >= 1; each is one step with lambda, then one step with mu if mu != 0 (Taubin's lambda|mu; mu == 0: plain Laplacian
 *               smoothing).
 *   flags       SL3D_SMOOTH_FIX_BOUNDARY: boundary vertices are fixed (scans are open surfaces, and the umbrella operator shrinks their
 *               rims).  SL3D_SMOOTH_NORMALS: also the normals -- the definition of sl3d_mesh_normals applied to the faces of M with the
 *               smoothed positions (the connectivity is NOT derived again from positions that have moved).
 *   output      one float triple per vertex in vertex-id order; the same bit for bit whatever the launch shape, the batch or the run.
 * No filtered form exists or is needed: gathers through vertex_ids of sl3d_mesh_views_filtered are exact for the smoothed positions and
 * their normals alike -- a kept vertex keeps all its faces, hence all its neighbours and its boundary edges.
 * Works wherever sl3d_mesh_views works (timed and parity contexts, windows: cells end at the window).  Everything lives in buffers of
 * its own (allocated on first use): points, valid, the clouds of sl3d_compact* / sl3d_run_clouds, the device mesh of the last
 * sl3d_mesh_views, the normals of the last sl3d_mesh_normals and the labels and filtered mesh of sl3d_mesh_components /
 * sl3d_mesh_views_filtered are not modified and stay valid.  SL3D_E_INVALID_ARG, and nothing on the device changes, for: a NaN or
 * non-positive max_edge, iterations outside [1, 1024], lambda not finite or outside (0, 1], mu not finite or outside [-1, 0], an unknown
 * flag bit, a bad view range, a NULL n_vertices.  The launch sequence is fixed by the arguments alone (cells, scan, rings, one launch per
 * step, vertices out, normals on request); nothing is read back but the counts.  Not covered: as for the mesh (groups, segments, the
 * shim). */
#define SL3D_SMOOTH_FIX_BOUNDARY 1u
#define SL3D_SMOOTH_NORMALS 2u
typedef struct sl3d_mesh_smoothed {   /* device-resident, valid until the next sl3d_mesh_smooth / sl3d_get_mesh_smoothed */
    const float *xyz;                 /* view first_view+k: n_vertices[k] triples at xyz + 3*k*view_stride_points */
    const float *normals;             /* same layout; NULL without SL3D_SMOOTH_NORMALS */
    size_t view_stride_points;
} sl3d_mesh_smoothed;
/* the smoothed vertices (and normals) of the meshes of views [first_view, first_view+n_views) on the device; device_mesh may be NULL */
int sl3d_mesh_smooth(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu, unsigned flags,
                     sl3d_mesh_smoothed *device_mesh, int64_t *n_vertices);
/* the same with a host copy under the capacity contract of sl3d_get_meshes: back to back, at most vertex_capacity triples in all in
 * xyz and in normals; xyz may be NULL; normals is looked at only with SL3D_SMOOTH_NORMALS (and may be NULL then) */
int sl3d_get_mesh_smoothed(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu,
                           unsigned flags, float *xyz, float *normals, int64_t vertex_capacity, int64_t *n_vertices);

/* ---- level-of-detail mesh of a view: one vertex per step x step pixel block (0.12.0) ----------------------------------------------
 * The meshes above work at full pixel resolution: a 1080p view gives about 2 M vertices and 4 M faces.  The organized grid makes a
 * lighter mesh cheap and exact: group the pixels into blocks, keep one vertex per block, mesh the coarse grid with the cell rules of
 * sl3d_mesh_views.  Inputs: a view with a dense result, step in [1, 16], max_edge and min_vertices as for sl3d_mesh_views_filtered,
 * lod_edge (mm, > 0, +inf allowed), flags.  Exact:
 *   candidates      the pixels whose vertex is in the filtered mesh sl3d_mesh_views_filtered(first_view, n_views, max_edge, min_vertices)
 *                   defines.  For min_vertices == 1 these are all valid pixels, whatever max_edge is (it must still be a valid argument).
 *   blocks          the coarse grid has H' = ceil(H / step) rows and W' = ceil(W / step) columns; block (R, C) covers rows
 *                   [R*step, min(R*step + step, H)) and columns [C*step, min(C*step + step, W)) of the WINDOW (blocks are anchored at the
 *                   window's row 0 / column 0, not at the camera frame's).
 *   representative  among a block's candidates (r, c) the one with the smallest integer
 *                   d = (2(r - R*step) + 1 - step)^2 + (2(c - C*step) + 1 - step)^2 -- the distance to the centre of the FULL block, for
 *                   blocks clipped by the window too; among equals the first in row-major scan order.  A block without a candidate
 *                   gives an invalid coarse pixel.  At an even step the four centre pixels tie and the upper left one wins: a bias of
 *                   half a pixel towards the window's origin, fixed and the same for every block.
 *   position        without SL3D_LOD_MEAN the representative's float triple, copied bitwise.  With SL3D_LOD_MEAN the members of a block
 *                   are the representative, always, and every other candidate q of the block with
 *                   len2(q, rep) <= (double)lod_edge * (double)lod_edge (len2 of sl3d_mesh_views; a NaN len2 is not a member); k = their
 *                   number.  k == 1: the representative's bits.  Otherwise, per component: s = +0, then s += (double)q over the members in
 *                   row-major scan order of the block; m = s / (double)k; the position is (float)m.  Every operation is one IEEE double
 *                   operation, nothing contracted; the cast rounds to nearest even.  A mean that never averages across a depth step
 *                   wider than lod_edge.  (As for the smoothing: sign and payload of a NaN the arithmetic PRODUCES are not defined.)
 *   vertices        the valid coarse pixels in row-major order of the coarse grid; the id of a vertex is its position in that order.
 *   vertex_ids      vertex_ids[i] = the id of vertex i's representative in the view's compacted cloud, in the order of sl3d_get_cloud --
 *                   the ORIGINAL id also for min_vertices > 1, exactly as for the filtered mesh.  Distinct, but not ascending: every id
 *                   of a coarse row lies above those of the coarse row before it, while within a coarse row the representatives of
 *                   neighbouring blocks may lie in different pixel rows.  Colours, normals and smoothed positions of the fine mesh
 *                   follow by gather: rgb[vertex_ids], smoothed[vertex_ids].
 *   faces           the definition of sl3d_mesh_views applied to the coarse grid -- the positions and the coarse valid map above -- with
 *                   lod_edge for max_edge: at most 2(W'-1)(H'-1) faces per view.  The diagonal choice and the edge tests read the
 *                   positions THIS call outputs.
 *   normals         (SL3D_LOD_NORMALS) the definition of sl3d_mesh_normals applied to that coarse mesh.
 *   identity        step == 1: vertices, faces and normals are those of sl3d_mesh_views(.., lod_edge) and sl3d_mesh_normals, bit for
 *                   bit (every block has one pixel, d = 0, k = 1); with min_vertices == 1 as well vertex_ids is 0 .. n-1.
 * The result is the same bit for bit whatever the batch, the launch shape or the run.  The launch sequence is fixed by the arguments
 * alone (min_vertices == 1: the cell pass and its scan for the ids -- no component kernel; min_vertices > 1: the components' launches and
 * the keep bytes of the filter, without its emit; then the block pass, the compaction and the mesh launches over the coarse grid, the
 * ids, normals on request); nothing is read back but the counts.  The outputs live in buffers of their own, allocated on first use for
 * the step asked and grown only when a later call needs more: points, valid, the clouds, the device mesh of sl3d_mesh_views, the normals,
 * labels, filtered mesh and smoothed mesh earlier calls handed out are not modified and stay valid.  SL3D_E_INVALID_ARG, and nothing on
 * the device changes, for: step outside [1, 16], a NaN or non-positive max_edge or lod_edge, min_vertices < 1, an unknown flag bit, a bad
 * view range, NULL count pointers.  Not covered: groups, segments, the shim; components or smoothing of the coarse mesh itself. */
#define SL3D_LOD_MEAN 1u
#define SL3D_LOD_NORMALS 2u
typedef struct sl3d_mesh_lod {        /* device-resident, valid until the next sl3d_mesh_views_lod / sl3d_get_meshes_lod */
    const float *xyz;                 /* view first_view+k: n_vertices[k] triples at xyz + 3*k*view_stride_points */
    const int32_t *faces;             /* n_faces[k] id triples at faces + 3*k*view_stride_faces */
    const int32_t *vertex_ids;        /* n_vertices[k] original ids at vertex_ids + k*view_stride_points */
    const float *normals;             /* layout of xyz; NULL without SL3D_LOD_NORMALS */
    size_t view_stride_points, view_stride_faces;
    int32_t grid_width, grid_height;  /* W', H' */
} sl3d_mesh_lod;
/* the level-of-detail meshes of views [first_view, first_view+n_views) on the device; device_mesh may be NULL */
int sl3d_mesh_views_lod(sl3d_ctx *ctx, int first_view, int n_views, int step, float max_edge, int64_t min_vertices, float lod_edge,
                        unsigned flags, sl3d_mesh_lod *device_mesh, int64_t *n_vertices, int64_t *n_faces);
/* the same with a host copy under the capacity contract of sl3d_get_meshes: back to back, at most vertex_capacity entries in all in
 * each of xyz, vertex_ids and normals, at most face_capacity triples in faces; any output pointer may be NULL (normals is looked at only
 * with SL3D_LOD_NORMALS); the counts are always returned */
int sl3d_get_meshes_lod(sl3d_ctx *ctx, int first_view, int n_views, int step, float max_edge, int64_t min_vertices, float lod_edge,
                        unsigned flags, float *xyz, int32_t *vertex_ids, float *normals, int64_t vertex_capacity, int32_t *faces,
                        int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces);

/* ---- small holes of a view's mesh filled from their rims (0.13.0) -------------------------------------------------------------------
 * A structured-light scan has dropouts -- specular pixels, pixels the modulation test rejects, the pixels of the fragments
 * sl3d_mesh_views_filtered drops -- and the meshes above leave them open.  The organized grid makes closing the small ones cheap and
 * exact.  Inputs: a view with a dense result (window W x H), max_edge and min_vertices as for sl3d_mesh_views_filtered, max_hole
 * (pixels, >= 0), fill_edge (mm, > 0, +inf allowed), flags.  Exact:
 *   candidates      as for the level-of-detail mesh: the valid pixels, or for min_vertices > 1 the pixels whose vertex
 *                   sl3d_mesh_views_filtered(first_view, n_views, max_edge, min_vertices) keeps.
 *   hole            a 4-connected component of non-candidate pixels of the window that contains no pixel of row 0, row H-1, column 0 or
 *                   column W-1 and has at most max_hole pixels.  Two holes that touch only at a corner are two components, each judged
 *                   by its own size.  n_holes counts the qualifying components.
 *   rim             of a hole pixel (r, c): L, R, U, D, the nearest candidates to its left, right, above and below.  They exist: a
 *                   walk along a line stays inside the component until it meets a candidate, and the component touches no border.
 *                   dl = c - c_L, dr = c_R - c, du = r - r_U, dd = r_D - r, all >= 1.
 *   usable          the row interpolant is usable iff len2(L, R) <= t * t with t = (double)fill_edge * (double)(dl + dr) (len2 of
 *                   sl3d_mesh_views; a NaN len2 is not usable); the column interpolant likewise with U, D and du + dd.  The rule: the
 *                   mean sample spacing along the span is at most fill_edge -- it keeps the fill from bridging a depth step or an
 *                   outlier on the rim.
 *   position        per component k, in double, every operation one IEEE operation in this order, nothing contracted:
 *                     h = ((double)dr * L_k + (double)dl * R_k) / (double)(dl + dr)
 *                     v = ((double)dd * U_k + (double)du * D_k) / (double)(du + dd)
 *                   both usable: (float)(((double)(du + dd) * h + (double)(dl + dr) * v) / (double)((dl + dr) + (du + dd)));
 *                   one usable: (float)h or (float)v; none: the pixel stays empty -- its hole counts in n_holes, the pixel not in
 *                   n_filled.  The casts round to nearest even.  (Sign and payload of a NaN the arithmetic PRODUCES are not defined.)
 *                   The rim consists of candidates only: a filled pixel never serves as the rim of another.
 *   filled grid     points: candidates keep their bits, filled pixels carry the position above.  valid: candidates and filled pixels,
 *                   and no other pixel -- for min_vertices > 1 that leaves out the valid pixels of dropped fragments, which a hole may
 *                   swallow and overwrite.
 *   vertices        the valid pixels of the filled grid in scan order; the id of a vertex is its position in that order.
 *   vertex_ids      for a candidate its id in the view's compacted cloud, in the order of sl3d_get_cloud -- the ORIGINAL id also for
 *                   min_vertices > 1, as for the filtered mesh; for a filled vertex -1.  Ascending apart from the -1s.
 *   faces           the definition of sl3d_mesh_views applied to the filled grid with max_edge.
 *   normals         (SL3D_FILL_NORMALS) the definition of sl3d_mesh_normals applied to that mesh.
 *   identity        max_hole == 0 and min_vertices == 1: vertices, faces and normals are those of sl3d_mesh_views / sl3d_mesh_normals bit
 *                   for bit, vertex_ids is 0 .. n-1.  For min_vertices > 1 and max_hole == 0 the result is the mesh of the CANDIDATE MAP:
 *                   as for the level-of-detail mesh at step 1 this is not the filtered mesh -- two kept vertices that the filter
 *                   separated only by dropping a fragment between them may share a face here if their edge is short.
 * The result is the same bit for bit whatever the batch, the launch shape or the run.  The launch sequence is fixed by the arguments
 * alone (candidates and ids as for the level-of-detail mesh; four launches that label the holes by a bounded lock-free union-find over
 * the non-candidate pixels and fill them, and the scan of their counts; the compaction and the mesh launches over the filled grid, the
 * ids, normals on request);
 * nothing is read back but the counts and the failure words.  The outputs live in buffers of their own, allocated on first use: points,
 * valid, the clouds, the device mesh of sl3d_mesh_views, the normals, labels, filtered, smoothed and level-of-detail meshes earlier calls
 * handed out are not modified and stay valid.  SL3D_E_INVALID_ARG, and nothing on the device changes, for: a NaN or non-positive max_edge
 * or fill_edge, max_hole < 0, min_vertices < 1, an unknown flag bit, a bad view range, NULL count pointers.  Not covered: groups,
 * segments, the shim; components, smoothing or level of detail of the filled mesh; colours of filled vertices. */
#define SL3D_FILL_NORMALS 1u
typedef struct sl3d_mesh_holes {      /* device-resident, valid until the next sl3d_mesh_fill_holes / sl3d_get_meshes_holes_filled */
    const float *xyz;                 /* view first_view+k: n_vertices[k] triples at xyz + 3*k*view_stride_points */
    const int32_t *faces;             /* n_faces[k] id triples at faces + 3*k*view_stride_faces */
    const int32_t *vertex_ids;        /* n_vertices[k] original ids (-1: filled) at vertex_ids + k*view_stride_points */
    const float *normals;             /* layout of xyz; NULL without SL3D_FILL_NORMALS */
    size_t view_stride_points, view_stride_faces;
} sl3d_mesh_holes;
/* the hole-filled meshes of views [first_view, first_view+n_views) on the device; device_mesh may be NULL.  n_holes[k]: the qualifying
 * holes of view first_view+k, n_filled[k]: the pixels filled */
int sl3d_mesh_fill_holes(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int64_t min_vertices, int64_t max_hole,
                         float fill_edge, unsigned flags, sl3d_mesh_holes *device_mesh, int64_t *n_vertices, int64_t *n_faces,
                         int64_t *n_holes, int64_t *n_filled);
/* the same with a host copy under the capacity contract of sl3d_get_meshes_lod: back to back, at most vertex_capacity entries in all in
 * each of xyz, vertex_ids and normals, at most face_capacity triples in faces; any output pointer may be NULL (normals is looked at only
 * with SL3D_FILL_NORMALS); the counts are always returned */
int sl3d_get_meshes_holes_filled(sl3d_ctx *ctx, int first_view, int n_views, float max_edge, int64_t min_vertices, int64_t max_hole,
                                 float fill_edge, unsigned flags, float *xyz, int32_t *vertex_ids, float *normals,
                                 int64_t vertex_capacity, int32_t *faces, int64_t face_capacity, int64_t *n_vertices, int64_t *n_faces,
                                 int64_t *n_holes, int64_t *n_filled);

/* register_point_clouds(unsigned, float tx, float ty, float tz, float rot_step)  9/register_point_clouds.cpp:23:
 * the compacted clouds of views [first_view, first_view+n_views) are rotated about the Y axis through (tx,ty,tz)
 * by 0, rot_step, 2*rot_step ... degrees and concatenated in view order; writes at most `capacity` points to xyz
 * (may be NULL) and always returns the total count. */
int sl3d_register_views(sl3d_ctx *ctx, int first_view, int n_views, float tx, float ty, float tz, float rot_step,
                        float *xyz, int64_t capacity, int64_t *total);

/* ---- host-buffer pipeline -------------------------------------------------------------------- */
/* The reference hands every stage host images (IplImage loaded from disk, 3/wrapped_phase.cpp:44, 4/phase_unwrap.cpp:78,84)
 * and reads host arrays back.  For callers that stay on that side of the boundary, sl3d_process_views runs a batch of
 * host-resident views through the context's view slots as a three-stage pipeline on three HIP streams (upload of view k+1,
 * fused kernel of view k, download of view k-1 overlap), so the sustained rate is that of the slowest stage (the PCIe
 * upload), not the sum.  planes: n_views * planes_per_view pointers, view-major, plane order of sl3d_device_buffers;
 * xyz: n_views dense [height][width][3] float images, NaN where invalid (may be NULL); valid: n_views [height][width]
 * byte images (may be NULL).  Masks and calibration must be set (sl3d_set_mask for every slot < max_views).
 * sl3d_host_alloc returns pinned memory: with it the copies are asynchronous DMA (pageable memory works, serialised).
 * A SL3D_FLAG_DIRECT_GRAY context uploads the F + N fringe and Gray planes of each coded axis alone: the pointers of the inverse planes
 * may be NULL. */
void *sl3d_host_alloc(size_t bytes);
void sl3d_host_free(void *p);
int sl3d_process_views(sl3d_ctx *ctx, int n_views, const uint8_t *const *planes, size_t stride, float *xyz, uint8_t *valid);

/* ---- capture-side undistortion --------------------------------------------------------------- */
/* cvUndistort2(src, dst, intrinsic_matrix, distortion_coeffs) as the acquisition stage applies it to every captured frame
 * before it is saved for stage 3/4 (2/project_pattern.cpp:220,232,287,...): OpenCV 2.4.0's algorithm on the device --
 * stripe-wise inverse map accumulated along each row in double, positions rounded to 1/32 pixel, INTER_LINEAR in 2^15
 * fixed point, BORDER_CONSTANT 0.  8-bit images of 1 or 3 interleaved channels, any size; src and dst must not overlap.
 * The arithmetic lives in OpenCV (not in the reference tree) and no raw capture is available: parity unpinned. */
int sl3d_undistort(sl3d_ctx *ctx, const uint8_t *src, size_t src_stride, int width, int height, int channels, const double K[9],
                   const double dist[5], uint8_t *dst, size_t dst_stride);

/* sl3d_set_frames for RAW captures: the frames go through cvUndistort2 with the camera calibration of sl3d_set_calibration
 * on their way into the frame stack (one launch for all planes of the axis, the map is built once per calibration), i.e.
 * the step 2/project_pattern.cpp:220,232,287 performs before stage 3/4 read the images.  Whole frames only. */
int sl3d_set_frames_raw(sl3d_ctx *ctx, int view, int axis, const uint8_t *const *planes, int n_planes, size_t stride);

/* ---- projector patterns (1/pattern_generator.cpp) ------------------------------------------- */
/* allocate_memory() 1/pattern_generator.cpp:224-229: number of codes = ceil(extent / fringe_width) and number of
 * Gray / binary bit planes = ceil(logf(codes) / logf(2)) (float arithmetic, as the reference writes it). Host only. */
int sl3d_pattern_counts(int proj_extent, int fringe_width, int *n_codes, int *n_planes);

#define SL3D_PATTERN_FRINGE 0        /* fringe_pattern_generate_3/_4/_5   :291-383  (index = phase step 0..F-1) */
#define SL3D_PATTERN_GRAY 1          /* generate_gray_coded_patterns      :56-197   (index = bit plane, MSB first) */
#define SL3D_PATTERN_INVERSE_GRAY 2  /* generate_inverse_gray_coded_patterns :490-507 */
#define SL3D_PATTERN_BINARY 3        /* binary_pattern_generate           :386-412 */

/* One projector pattern of generate_pattern() (1/pattern_generator.cpp:513), proj_width x proj_height 8-bit, generated
 * on the device from the context's configuration (n_fringe, fringe widths, n_gray_v / n_gray_h bit planes).
 * axis: SL3D_AXIS_VERTICAL = the pattern varies with the column.  index == n_gray (the extra image the reference
 * saves, :433-465, and never fills) is all zeros.  host_dst (may be NULL) receives the image, `stride` bytes per row;
 * device_ptr / device_pitch (may be NULL) return the HBM copy, valid until the next call on this context. */
int sl3d_generate_pattern(sl3d_ctx *ctx, int kind, int axis, int index, uint8_t *host_dst, size_t stride,
                          const uint8_t **device_ptr, size_t *device_pitch);

/* one cloud of register_point_clouds() (9/register_point_clouds.cpp:83-128) given in host memory, as the reference reads
 * it from a PLY file: p -> R_y(theta)*(p - t) + t in the reference's arithmetic; theta in degrees (Pi = 22/7) */
int sl3d_transform_cloud(sl3d_ctx *ctx, const float *xyz_in, int64_t n, float theta_deg, float tx, float ty, float tz, float *xyz_out);

/* ---- device-resident access ---------------------------------------------------------------- */
/* Frames may be produced in place (frames buffer) and points / valid consumed in place.  The mask buffer is exposed for
 * inspection only: set masks through sl3d_set_mask, which also normalises the bytes to 0/1 and evaluates the quads within
 * 3 pixels of the frame border (a second plane the kernels read for those quads). */
int sl3d_get_device_buffers(sl3d_ctx *ctx, sl3d_device_buffers *out);
/* Copy `bytes` from a device address this library handed out (sl3d_get_cloud_counts, sl3d_compact, sl3d_compact_views,
 * sl3d_mesh_views, sl3d_get_device_buffers) to host memory, ordered after the context's work; synchronises. */
int sl3d_download(sl3d_ctx *ctx, void *host_dst, const void *device_src, size_t bytes);
/* the same for a pitched region (`height` rows of `width_bytes`), ENQUEUED on the context's stream: asynchronous for pinned host
 * memory (the caller waits with sl3d_synchronize), so many regions can be queued behind one wait */
int sl3d_download_2d(sl3d_ctx *ctx, void *host_dst, size_t dst_pitch, const void *device_src, size_t src_pitch, size_t width_bytes, size_t height);

/* ---- several GPUs behind one caller: row-stripe groups -------------------------------------------------------------
 * The reference is ONE process that scans one view after the other (m_tech_project_console.cpp:366-395); a group lets that
 * single caller use the GPUs of a node without becoming a distributed program.  The window of `cfg` is cut into n_stripes
 * contiguous row stripes (stripe i gets rows [row0_i, row0_i + rows_i): height/n_stripes rows each, the first
 * height % n_stripes stripes one more); stripe i is an ordinary context on HIP device devices[i] with its own stream.
 * Every stage is a per-pixel map whose only neighbourhood input is the selection mask, so the stripes need NO exchange
 * while they compute (each keeps 2 halo rows of the INPUT mask).  The only exchange is the assembly of the results on the
 * root (stripe 0's device): sl3d_group_gather = ONE RCCL group of point-to-point sends over xGMI (ncclSend / ncclRecv,
 * a gather) that land in place in the root's dense [view][row] buffers -- rank order = row order, so the row-major scan
 * order of 8/save_point_cloud.cpp:85 is preserved; stripes that live on the root's own GPU are device-to-device copies.
 * Devices may repeat (several stripes on one GPU: tests, or more stripes than GPUs).  cfg->device and cfg->stream are
 * ignored.  All group calls are asynchronous unless stated; compute runs on the stripes' streams, communication on one
 * communication stream per GPU, handed over by events, so sl3d_group_run of the next views overlaps the gather of the
 * previous ones. */
typedef struct sl3d_group sl3d_group;

int sl3d_group_create(const sl3d_config *cfg, const int *devices, int n_stripes, sl3d_group **out);
void sl3d_group_destroy(sl3d_group *g);
/* text of the last error on this group; sl3d_last_error(NULL) after a failed sl3d_group_create */
const char *sl3d_group_last_error(const sl3d_group *g);
int sl3d_group_size(const sl3d_group *g);
/* stripe i: its rows inside the window, its device and its context (owned by the group; any single-context call that
 * does not change the configuration may be used on it, e.g. sl3d_synth_view, sl3d_get_points, sl3d_get_device_buffers) */
int sl3d_group_stripe(sl3d_group *g, int i, int *row0, int *rows, int *device, sl3d_ctx **ctx);
/* "rccl" if stripes on other GPUs travel by RCCL send/recv, "copy" if every transfer is a (peer) device copy */
const char *sl3d_group_transport(const sl3d_group *g);

/* the single-context inputs, applied to every stripe (each uploads only its own byte range of every plane, on its own GPU;
 * planes are WINDOW-sized: `width` x `height` of cfg) */
int sl3d_group_set_calibration(sl3d_group *g, const double Kc[9], const double dc[5], const double rc[3], const double tc[3],
                               const double Kp[9], const double dp[5], const double rp[3], const double tp[3]);
int sl3d_group_set_mask(sl3d_group *g, int view, const uint8_t *full_frame_mask, size_t stride);
int sl3d_group_set_frames(sl3d_group *g, int view, int axis, const uint8_t *const *planes, int n_planes, size_t stride);

/* sl3d_run on every stripe (one launch per GPU stream) */
int sl3d_group_run(sl3d_group *g, int first_view, int n_views);
/* assemble xyz + valid of views [first_view, first_view+n_views) on the root GPU: waits (on the device) for the stripes'
 * kernels of those views, then one grouped exchange on the communication streams */
int sl3d_group_gather(sl3d_group *g, int first_view, int n_views);
/* the assembled dense results of a view (window-sized [height][width][3] f32, NaN where invalid; [height][width] valid);
 * waits for the gather of that view; either pointer may be NULL */
int sl3d_group_get_points(sl3d_group *g, int view, float *xyz, uint8_t *valid);
/* The assembly for the reference's real consumer, the HOST (its results are host globals / a host cloud: common_variables.h:12-21,
 * 56-62, 8/save_point_cloud.cpp:85-104): views [first_view, first_view+n_views) as n_views dense [height][width][3] float images
 * (NaN where invalid) and [height][width] valid bytes; either pointer may be NULL.  Every stripe copies its rows straight into
 * the caller's images on its own stream and over its own GPU's PCIe link -- no gather to a root, no xGMI hop.  Use pinned
 * memory (sl3d_host_alloc) for concurrent DMA.  Waits for the stripes' kernels and for the copies. */
int sl3d_group_download_points(sl3d_group *g, int first_view, int n_views, float *xyz, uint8_t *valid);
/* sl3d_process_views for a group: host-resident views through every stripe's three-stream pipeline (upload of its rows,
 * kernel, download into the caller's dense images); the stripes work concurrently.  planes: n_views * planes_per_view
 * pointers to window-sized planes, view-major. */
int sl3d_group_process_views(sl3d_group *g, int n_views, const uint8_t *const *planes, size_t stride, float *xyz, uint8_t *valid);
/* the assembled buffers in the root GPU's memory, for consumers that stay on the device (layout of sl3d_device_buffers'
 * points / valid with the window's height; frames / mask members are not filled) */
int sl3d_group_get_device_buffers(sl3d_group *g, sl3d_device_buffers *out);

/* the compacted variant: sl3d_run_clouds on every stripe, then the counts come back to the host and every stripe sends
 * exactly its valid points; the root concatenates them in stripe order = the reference's scan order.
 * counts[k] = points of view first_view+k (all stripes).  sl3d_group_get_cloud waits for the transfer. */
int sl3d_group_run_clouds(sl3d_group *g, int first_view, int n_views);
int sl3d_group_gather_clouds(sl3d_group *g, int first_view, int n_views, int64_t *counts);
int sl3d_group_get_cloud(sl3d_group *g, int view, float *xyz, int64_t capacity, int64_t *count);

/* waits for every stripe's stream and every communication stream */
int sl3d_group_synchronize(sl3d_group *g);

#ifdef __cplusplus
}
#endif
#endif /* SL3D_H */
