// sl3d_internal.h -- structures shared by the C-ABI host code (sl3d_capi_*.cpp) and the HIP kernels (sl3d_fused_*.hip, sl3d_kernels.hip,
// sl3d_clouds.hip, sl3d_modulation.hip, sl3d_mesh.hip, sl3d_mesh_normals.hip, sl3d_mesh_components.hip, sl3d_mesh_smooth.hip, sl3d_mesh_lod.hip, sl3d_mesh_holes.hip, sl3d_period.hip, sl3d_subpixel.hip, sl3d_subpixel_fused.hip, sl3d_repair_fused.hip, sl3d_one_axis.hip, sl3d_direct_gray.hip, sl3d_exposure.hip, sl3d_outlier.hip, sl3d_voxel.hip, sl3d_align.hip, sl3d_align_plane.hip, sl3d_tsdf.hip -- the four before the last five share sl3d_quad.h, what a quad-per-lane kernel is made of).  Not part of
// the public ABI.  What the consumers of a dense result share on the HOST side is here (CompactScratch, compact_blocks, view_planes,
// mesh_launch, mesh_face_stride, CcTotals); the block idioms of their kernels are in sl3d_block.h, a mesh lane's loads in sl3d_mesh_lane.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>   // dim3
#include <hip/hip_vector_types.h>  // float2

#include "sl3d_fused_choice.h"  // SL3D_MAX_GRAY, SL3D_SMALL_LAUNCH_VIEWS, SL3D_BLOCK, SL3D_SMALL_BLOCK, FusedKey

#define SL3D_MASK_HALO 2        // rows / columns of selection mask kept around the window
#define SL3D_MASK_LPAD 16       // bytes in front of window column 0 in every mask row
#define SL3D_ATAN_T1 511        // t1 = I0 - I2        in [-255, 255]
#define SL3D_ATAN_T2 1021       // t2 = 2*I1 - I0 - I2 in [-510, 510]
#define SL3D_SEG_POINTS 256     // pixels (point slots) per segment of the segmented clouds = one wave of the fused kernel

struct AlignCam;   // sl3d_align.h
struct AlignPass;
struct TsdfVolume;  // sl3d_tsdf.h
struct TsdfTurn;
struct TsdfPlanes;

namespace sl3d {

// Intrinsics of one device (camera or projector) as stage 7 uses them (T1).
struct Intr {
    double K[9];
    double ifx, ify, cx, cy;      // cvUndistortPoints normalises with the reciprocal focal lengths
    double k1, k2, p1, p2, k3;
    int has_dist;                 // any distortion coefficient non-zero (else the 5 iterations are an exact no-op)
    int affine;                   // last row of K is (0,0,1): the homogeneous divide is an exact no-op
    int has_tan;                  // p1 or p2 non-zero
    int plain;                    // affine and K[1] == K[3] == 0 (no skew)
    int identity;                 // plain and no distortion: undistort + re-project returns the pixel itself
};

// One node of a radial undistortion table: s(r0^2) = (factor of the last of the 5 fixed-point iterations of cvUndistortPoints) - 1 for a
// purely radial model, as a quadratic around node i of a uniform grid over r0^2 (w = distance to the node in node spacings,
// |w| <= 1/2):  s = c0 + (c1 + c2*w)*w.  The quadratic interpolates s at the node and at both cell boundaries, so neighbouring
// cells agree where they meet; with SL3D_RAD_NODES nodes its remainder is ~1e-10 of the normalised coordinate.
struct __attribute__((aligned(16))) RadEntry {
    double c0;
    float c1, c2;
};
#define SL3D_RAD_NODES 256
#define SL3D_RAD_COPIES 8                      // copies of a table the kernels read (one per XCD)
#define SL3D_RAD_STRIDE (SL3D_RAD_NODES + 16)  // entries between two copies: 4 KB + 256 B, so that the copies start on different channels

// Per-scan constants of stage 7 (T0): A = K*[R|t] for camera and projector.
struct DevCal {
    double Ac[12], Ap[12];
    Intr cam, proj;
    // Camera-frame form of the same least-squares problem (fast path of the fused kernel; valid when the camera matrix
    // is upper triangular and affine, K = [fx s cx; 0 fy cy; 0 0 1]).  With Y = Rc*X + tc the two camera rows of P become
    // fx*(1,0,-xn) + s*(0,1,-yn) and fy*(0,1,-yn) with a zero right-hand side ((xn,yn) = undistorted normalised coordinates --
    // cvUndistortPoints normalises with fx, fy, cx, cy only, the skew enters when K re-projects), so their part of
    // P^T P is a handful of flops instead of 26; the rigid change of variables leaves the minimiser unchanged.
    double Apc[12];       // Ap * [Rc tc; 0 1]^-1 : projector projection matrix acting on camera-frame points
    double Rct[9], tcn[3];  // X = Rct*Y + tcn  (Rct = Rc^T, tcn = -Rc^T tc)
    double fx2, fy2;      // Kc[0]^2, Kc[1]^2 + Kc[4]^2
    double fxs;           // Kc[0]*Kc[1]: the skew term (0 for the usual K); the camera-frame form holds for any upper-triangular affine K
};

// Scene + camera model of the synthetic-capture generator (k_synth).
struct SynthParams {
    double Rc[9], tc[3], Rp[9], tp[3];  // world -> camera / projector
    double Kp[9];
    double z0, a, b;                    // plane Z = z0 + a*X + b*Y
    float gain, offset;
    int noise;                          // uniform integer noise in [-noise, noise]
    unsigned long long seed;
    int view_id;                        // enters the noise hash
};

// Where k_mask_prepare reads a selection mask from: the staging plane behind sl3d_set_mask's copy, or the caller's device memory.
struct MaskSrc {
    uintptr_t origin;      // address of plane row 0, byte 0 (= window row -2, window column -16); only bytes inside the region below are read
    size_t stride;         // bytes between rows
    size_t view_stride;    // bytes between the masks of consecutive views of one call (0: every view gets the same mask)
    int bx0, bx1, r0, r1;  // plane bytes [bx0, bx1) x plane rows [r0, r1) hold source pixels: window + 2-pixel halo, clipped to the frame
};

// A MASKIN launch (k_fused with CMODE bit 4: the valid bits come from the raw selection -- H0 / S3b / S3d inside the fused kernel):
// where the selection of view first_view + k lies (MaskSrc::origin of that view), the region of the plane that holds source bytes,
// what may be read at all, and where every wave leaves {seq << 8 | quads with a valid pixel}.
struct MaskIn {
    uintptr_t origin[SL3D_SMALL_LAUNCH_VIEWS];
    size_t stride;
    int bx0, bx1, r0, r1;  // as in MaskSrc
    int lo, hi;            // plane bytes [lo, hi) of a row may be READ (the staging plane: the whole row; a caller's mask: the frame's columns)
    unsigned *part;        // host memory mapped into the device: [view][part_stride] words, one per wave that owns pixels
    unsigned part_stride;
    unsigned seq;
};

// Everything a kernel needs to address one context's buffers.
struct KParams {
    int W, H;                  // window
    int fullW, fullH;          // camera frame
    int col0, row0;            // window origin in the frame
    int PW, PH;
    int F, Nv, Nh;
    int fwv, fwh;
    int ncodes_v, ncodes_h;
    int ablate;                // measurement builds only (-DSL3D_MEASURE, env SL3D_ABLATE): bit2 skips the camera undistortion; 0 otherwise
    int pitch;                 // bytes per row of every u8 plane (multiple of 16)
    int planes_per_view;
    size_t plane_stride;       // pitch * H
    size_t view_stride;        // planes_per_view * plane_stride
    int mpitch;                // mask row pitch (pitch + 32)
    size_t mask_view_stride;   // mpitch * (H + 2*SL3D_MASK_HALO)
    const uint8_t *frames;
    const uint8_t *mask;       // 0/1 bytes, halo included
    const uint8_t *band;       // [view][row][pitch]: final valid bytes of the quads within 3 px of the frame border (set_mask)
    const float2 *proj_disp;   // [PH][PW] undistorted-minus-raw projector point (set_calibration; NULL unless the projector is distorted)
    const RadEntry *proj_rad;  // rig 3: SL3D_RAD_NODES nodes of a purely radial projector model over r0^2 in [0, (NODES - 1) / proj_rad_scale]
    float proj_rad_scale;      // nodes per unit of r0^2
    const double *cam_tab;     // T1 of the camera per window pixel (set_calibration, timed mode): kind 1 = [H][pitch] factor of the last
                               // undistortion iteration (radial model), kind 2 = [H][pitch][2] normalised point (tangential terms)
    int cam_tab_kind;          // 0 = no table (no distortion: nothing to iterate)
    int use_cam_table;         // set per launch: 0, or cam_tab_kind
    // dense results
    float *points;             // [view][row][pitch][3] f32
    uint8_t *valid;            // [view][row][pitch]    merged valid map
    size_t px_view_stride;     // pitch * H   (elements per view of every per-pixel plane)
    // ordered clouds written by the fused kernel itself (sl3d_run_clouds; NULL until first used)
    float *clouds;             // [view][px_view_stride][3]: per view 4*n_tiles segments of SL3D_SEG_POINTS point slots
    unsigned long long *cloud_totals;  // [view] number of valid points -- HOST memory mapped into the device: k_seg_scan stores the
                                       // count where sl3d_get_cloud_counts reads it after the stream has drained (no copy)
    int n_tiles;               // 1024-pixel tiles per view = blocks of the fused kernel along x that own pixels
    int prefer_gated;          // set per launch (host only): small launch over sparsely selected views -> the large-launch kernel
    // a segment's first seg_counts[view][seg] slots are its valid points in scan order
    unsigned *seg_counts;              // [view][n_segs]
    unsigned long long *seg_offsets;   // [view][n_segs] exclusive scan of the counts (k_seg_scan)
    int n_segs;                        // 4 * n_tiles
    unsigned long long *dbg;   // measurement builds (-DSL3D_TRACE): [block][wave][8] clock stamps of the dense kernel's phases; NULL otherwise
    // stage-boundary planes (NULL unless SL3D_FLAG_KEEP_STAGES)
    float *wrapped[2];
    float *unwrapped[2];
    int32_t *code[2];
    uint8_t *valid_axis[2];
    uint8_t *dbg3[2];
    uint8_t *dbg4[2];
    int64_t *cpmap;            // [view][row][pitch][2]
    double *ipoints;           // [view][row][pitch][3]
    // (appended in round 6: the fields above keep their kernel-argument offsets)
    MaskIn mi;                 // MASKIN launches only (read through the kernel-argument segment, sl3d_fused.h: maskin_args)
};
static_assert(SL3D_SMALL_LAUNCH_VIEWS == 4, "MaskIn::origin holds one entry per view of a small launch");

// launchers (sl3d_fused_launch.hip, sl3d_kernels.hip, sl3d_clouds.hip); `stream` is a hipStream_t
// cmode: 0 = dense xyz + valid planes, 2 = segmented clouds
// prefer_gated: the views of a small launch are sparsely selected (sl3d_capi_inputs.cpp: sparse_views)
// mi != nullptr: a MASKIN launch (the views' valid bits from their raw selection; only where fused_choice has a MASKIN kernel)
// ran: the instantiation that went out (left alone if none did)
int launch_fused(const KParams &P, const DevCal *d_cal, int rig, int first_view, int n_views, bool keep, int cmode, void *stream, bool prefer_gated,
                 const MaskIn *mi, FusedKey &ran);
// the k_fused instantiation such a launch runs (sl3d_fused_choice.h: fused_key; nmax == 0: none)
FusedKey fused_choice(const KParams &P, int rig, int n_views, bool keep, int cmode, bool prefer_gated, bool maskin);
// the launchers of one family of k_fused instantiations (fused_family), one per key: family FAMILY is instantiated by the
// sl3d_fused_*.hip unit that compiles it, and launch_fused looks its keys up.  A family no unit instantiates is a null weak reference
// (its launches fail with hipErrorInvalidValue; tests/test_fused_choice.py: the library's instantiations are the rule's keys).
typedef void (*FusedLauncher)(unsigned grid_x, unsigned grid_y, unsigned block, void *stream, const KParams &P, const DevCal *C, int first_view, int n_views,
                              int vpt);
struct FusedEntry {
    FusedKey key;
    FusedLauncher launch;
};
struct FusedTable {
    const FusedEntry *entry;
    int n;
};
template <int FAMILY>
__attribute__((weak)) FusedTable fused_table();
// words per view in MaskIn::part (one per wave of the small-launch grid) / how many of them belong to waves that own pixels
unsigned fused_maskin_part_stride(const KParams &P);
unsigned fused_maskin_part_words(const KParams &P);
// segmented clouds: offsets / totals of views [first_view, first_view + n_views) from the counts the fused kernel stored
int launch_seg_scan(const KParams &P, int first_view, int n_views, void *stream);
// segments -> contiguous (k_seg_close): view first_view + k's points go to dst + 3 * k * dst_view_stride_points (dst: device memory or
// mapped host memory).  scan: the views' counts have NOT been scanned -- the kernel scans on entry instead of reading P.seg_offsets, writes
// at most capacity_points points of each view and leaves the views' totals in P.cloud_totals.  R4 (not together with scan):
// register_point_clouds on the way -- every point rotated about Y by R4 = {r00, r02, r20, r22} around (tx, ty, tz)
struct SegClose {
    float *dst;
    size_t dst_view_stride_points;
    bool scan;
    unsigned long long capacity_points;
    const float *R4;
    float tx, ty, tz;
};
int launch_seg_close(const KParams &P, int first_view, int n_views, const SegClose &c, void *stream);
int fused_tiles(const KParams &P);  // number of 1024-pixel tiles per view (KParams::n_tiles)
// k_mask_prepare over views [first_view, first_view + n_views): view k reads S.origin + k * S.view_stride; block b of view v stores
// {seq, quads with a valid pixel} at partials[v * mask_prepare_blocks(P) + b] (host memory mapped into the device)
int launch_mask_prepare(const KParams &P, int first_view, int n_views, const MaskSrc &S, unsigned long long *partials, unsigned seq, void *stream);
// the fringe-modulation test (sl3d_modulation.hip, sl3d_modulation.h): views [first_view, first_view + n_views) -> slot k of the mask staging
// plane `staging` (mask_view_stride bytes apart) gets view first_view + k's selection, 0/1 bytes over its frame region (has_mask: ANDed
// with the mask bytes == 1 already staged there); whole frames, F == 3 only
int launch_modulation_select(const KParams &P, int first_view, int n_views, uint8_t *staging, bool has_mask, double thr, void *stream);
// gamma of one axis of one view -> out[row * pitch + col] (pitch * H floats, 16-byte aligned)
int launch_modulation_gamma(const KParams &P, int view, int axis, float *out, void *stream);
int mask_prepare_blocks(const KParams &P);
int launch_to_colrow(const KParams &P, int view, int which, void *dst, void *stream);  // a global in the reference's [col][row] layout
int launch_mask_from_colrow(const KParams &P, const int *sel, int gx0, int gy0, int ncols, int nrows, uint8_t *raw, void *stream);
int launch_proj_table(const DevCal *d_cal, int PW, int PH, float2 *out, void *stream);
// SL3D_RAD_COPIES copies (SL3D_RAD_STRIDE entries apart) of the SL3D_RAD_NODES nodes of the radial factor of the camera (which = 0) or
// the projector (1) over r0^2 in [0, r2max]
int launch_radial_table(const DevCal *d_cal, int which, double r2max, RadEntry *out, void *stream);
int launch_cam_table(const KParams &P, const DevCal *d_cal, int kind, double *out, void *stream);
int launch_wrap(const KParams &P, int view, int axis, void *stream);
int launch_unwrap(const KParams &P, int view, int axis, void *stream);
int launch_corr(const KParams &P, int view, void *stream);
// the period repair of one axis of one view (sl3d_period.hip, sl3d_period.h): jump [px_view_stride] bytes and, for an axis of 8 or more
// Gray planes (else NULL), wide [px_view_stride] ints -- scratch the two launches hand j over in; counts: the two words the launch ADDS
// the repaired and the unrepairable pixels to
struct PeriodPlanes {
    int8_t *jump;
    int *wide;
    unsigned *counts;
};
int launch_period_repair(const KParams &P, int view, int axis, int radius, const PeriodPlanes &b, void *stream);
int launch_tri(const KParams &P, const DevCal &C, int view, void *stream);
// the sub-pixel triangulation of views [first_view, first_view + n_views) in one launch (sl3d_subpixel.hip, sl3d_subpixel.h): residual
// [max_views][px_view_stride]; partials: NULL, or [n_views][subpixel_blocks(P)] words of scratch -- then a second launch sums them into
// counts [n_views][2], the triangulated and the rejected pixels of view first_view + k.  launch_subpixel_coords: (xs, ys) of one view ->
// xy [px_view_stride][2].  anchor (SL3D_FLAG_ANCHOR_PERIODS, sl3d_anchor.h): the coordinates of both from the wrapped-phase and code planes
unsigned subpixel_blocks(const KParams &P);
int launch_subpixel(const KParams &P, const DevCal &C, int first_view, int n_views, double max_residual, float *residual, unsigned *partials,
                    unsigned *counts, bool anchor, void *stream);
int launch_subpixel_coords(const KParams &P, int view, double *xy, bool anchor, void *stream);
// the sub-pixel scan of a timed context (sl3d_subpixel_fused.hip, SL3D_FLAG_SUBPIXEL): frames and prepared valid bytes of views [first_view,
// first_view + n_views) -> their points, valid and residual planes, what launch_wrap / launch_unwrap of both axes, launch_corr and
// launch_subpixel(+inf, anchor) leave there, in one launch.  SL3D_SUBPIXEL_FUSED_NAME / _ANCHOR_NAME: the two instantiations as rocprofv3
// spells them
#define SL3D_SUBPIXEL_FUSED_NAME "sl3d::k_subpixel_fused<false>"
#define SL3D_SUBPIXEL_FUSED_ANCHOR_NAME "sl3d::k_subpixel_fused<true>"
int launch_subpixel_fused(const KParams &P, const DevCal *d_cal, int first_view, int n_views, float *residual, bool anchor, void *stream);
// the one-axis scan (SL3D_FLAG_ONLY_VERTICAL / _HORIZONTAL, sl3d_one_axis.h; axis: the coded one).  Staged: launch_corr_one (sl3d_kernels.hip)
// is stage 5 of that axis alone, launch_subpixel_one / launch_subpixel_coords_one (sl3d_subpixel.hip) the one-axis forms of launch_subpixel
// (no residual, nothing rejected: counts [n_views][2] = triangulated, 0) and launch_subpixel_coords.  Timed: launch_one_axis
// (sl3d_one_axis.hip) leaves in the views' points and valid planes what launch_wrap / launch_unwrap of that axis, launch_corr_one and
// launch_subpixel_one leave there, in one launch.  SL3D_ONE_AXIS_NAME: its four instantiations as rocprofv3 spells them
int launch_corr_one(const KParams &P, int view, int axis, void *stream);
int launch_subpixel_one(const KParams &P, const DevCal &C, int axis, int first_view, int n_views, unsigned *partials, unsigned *counts, bool anchor,
                        void *stream);
int launch_subpixel_coords_one(const KParams &P, int axis, int view, double *xy, bool anchor, void *stream);
#define SL3D_ONE_AXIS_NAME(axis, anchor) \
    ((axis) == 0 ? ((anchor) ? "sl3d::k_one_axis<0, true>" : "sl3d::k_one_axis<0, false>") : ((anchor) ? "sl3d::k_one_axis<1, true>" : "sl3d::k_one_axis<1, false>"))
int launch_one_axis(const KParams &P, const DevCal *d_cal, int axis, int first_view, int n_views, bool anchor, void *stream);
// the scans of a SL3D_FLAG_DIRECT_GRAY context (sl3d_direct_gray.h / .hip): stage 4's Gray bit against the fringe mean, no inverse plane read.
// Staged: launch_unwrap_direct is launch_unwrap with that bit.  Timed: launch_direct_gray leaves in the views' points and valid planes (axes
// == 2: and in `residual`) what launch_wrap / launch_unwrap_direct, launch_corr / launch_corr_one and launch_subpixel(+inf) / launch_subpixel_one
// leave there, in one launch; axes: 0 / 1 the one coded axis, 2 both.  SL3D_DIRECT_GRAY_NAME: its six instantiations as rocprofv3 spells them
int launch_unwrap_direct(const KParams &P, int view, int axis, void *stream);
#define SL3D_DIRECT_GRAY_NAME(axes, anchor)                                                                  \
    ((axes) == 0   ? ((anchor) ? "sl3d::k_direct_gray<0, true>" : "sl3d::k_direct_gray<0, false>")          \
     : (axes) == 1 ? ((anchor) ? "sl3d::k_direct_gray<1, true>" : "sl3d::k_direct_gray<1, false>")          \
                   : ((anchor) ? "sl3d::k_direct_gray<2, true>" : "sl3d::k_direct_gray<2, false>"))
int launch_direct_gray(const KParams &P, const DevCal *d_cal, int axes, int first_view, int n_views, float *residual, bool anchor, void *stream);
// the fringe-modulation test of a one-axis context: gamma of the coded axis alone, no plane of the other axis read
int launch_modulation_select_one(const KParams &P, int first_view, int n_views, uint8_t *staging, bool has_mask, double thr, int axis, void *stream);
// the exposure fusion (sl3d_exposure.hip, sl3d_exposure.h; the rule: include/sl3d_fuse.h, sl3d_fuse_exposures).  The planes in use: of coded axis
// i (n_axes of them) the count[i] planes from plane base[i] of planes_per_view on, its F fringe planes first.  Exposure e is view first_view
// + e; map: the map plane of dst_view ([row][pitch] bytes); counts: n_exposures + 1 words the launch ADDS to (the caller has cleared them)
#define SL3D_EXPOSURE_COUNTS 9  // SL3D_MAX_EXPOSURES + 1
struct ExposurePlan {
    int n_axes;
    int base[2], count[2];
};
int launch_fuse_exposures(const KParams &P, const ExposurePlan &X, int first_view, int n_exposures, int dst_view, int saturation, uint8_t *map,
                          unsigned *counts, void *stream);
// the radius outlier filter (sl3d_outlier.hip, sl3d_outlier.h; the rule: include/sl3d_filter.h, sl3d_filter_outliers).  support: the support
// planes [max_views][px_view_stride] bytes, view v's at v * px_view_stride.  launch_outlier_support writes the planes of the launch's views
// (radius 1 .. SL3D_OUTLIER_MAX_RADIUS) and changes nothing else; launch_outlier_apply, behind it, rejects the samples whose support is
// below min_neighbours (0: none, the launch only counts) in P.valid, P.points and, where the context has it, P.ipoints; counts: [n_views][2]
// words the launch ADDS the views' samples and rejected samples to (the caller has cleared them)
int launch_outlier_support(const KParams &P, int first_view, int n_views, int radius, float max_dist, uint8_t *support, void *stream);
int launch_outlier_apply(const KParams &P, int first_view, int n_views, int min_neighbours, const uint8_t *support, unsigned *counts, void *stream);
// the period-repaired scan of a timed context (sl3d_repair_fused.hip, SL3D_FLAG_REPAIR_PERIODS): what launch_wrap / launch_unwrap of both
// axes, launch_period_repair(radius SL3D_REPAIR_FUSED_RADIUS) of every axis that has Gray planes, launch_corr and launch_tri leave in
// the views' points and valid planes, in one launch; residual != NULL: the sub-pixel ending instead (launch_subpixel(+inf)) and the
// residual plane with it.  SL3D_REPAIR_FUSED_NAME / _SUB_NAME: the two instantiations as rocprofv3 spells them
#define SL3D_REPAIR_FUSED_RADIUS 4
#define SL3D_REPAIR_FUSED_NAME "sl3d::k_repair_fused<false>"
#define SL3D_REPAIR_FUSED_SUB_NAME "sl3d::k_repair_fused<true>"
int launch_repair_fused(const KParams &P, const DevCal *d_cal, int first_view, int n_views, float *residual, void *stream);
// counts per block (or chunk) of a launch's views, their exclusive scan (k_compact_scan) and the views' totals: the scratch of every
// consumer of a dense result.  Compaction (O1 / N2): cnt / off hold one slot per view OF A LAUNCH (slot k: view first_view + k), a slot =
// the valid pixels of the view's 1024-pixel blocks; tot: [max_views], view v's at tot[v].  Mesh: cnt / off [max_views][2][mesh_chunks]
// (valid pixels, faces per chunk), tot [max_views][2].  Normals: cnt / off [max_views][mesh_chunks] valid pixels per chunk, tot [max_views]
struct CompactScratch {
    unsigned *cnt;
    unsigned long long *off, *tot;
};
inline size_t compact_blocks(const KParams &P) { return (P.px_view_stride + 1023) / 1024; }  // 1024-pixel blocks of a view: counts per slot
// the valid / points planes of view first_view of the dense result (the views behind it follow px_view_stride elements apart)
struct ViewPlanes {
    const uint8_t *valid;
    const float *points;
};
inline ViewPlanes view_planes(const KParams &P, int first_view)
{
    return {P.valid + (size_t)first_view * P.px_view_stride, P.points + 3 * (size_t)first_view * P.px_view_stride};
}
int launch_compact_views(const KParams &P, int first_view, int n_views, const CompactScratch &s, float *clouds, const uint8_t *texture,
                         uint8_t *rgb_out, void *stream);
int launch_compact_scan(const unsigned *counts, unsigned long long *offsets, int n, int n_arrays, unsigned long long *totals, void *stream);
// the voxel grid over an unorganised cloud (sl3d_voxel.hip, sl3d_voxel.h; the rule: include/sl3d_voxel.h, sl3d_voxel_grid).  The table is a
// structure of arrays of `capacity` slots (voxel_table_capacity); sums: 3 x capacity, the three coordinates one after the other, NULL in
// first mode.  slot_of: a word per point, padded to whole 1024-point blocks.  words: VOXEL_WORDS 64-bit words of the call.  All of it is
// initialised on the stream by launch_voxel_grid itself (keys and first to all ones, the rest to zero)
struct VoxelTable {
    unsigned long long *key;
    unsigned *first, *count;
    long long *sums;
    unsigned long long capacity;
};
enum { VOXEL_WORD_DROPPED, VOXEL_WORD_OCCUPIED, VOXEL_WORD_KEPT, VOXEL_WORD_ERROR, VOXEL_WORDS };
struct VoxelOut {
    float *xyz;
    int *first;
    unsigned *count;
};
// cloud: n (> 0, < 2^31) points on the device.  Memsets, k_voxel_insert, k_voxel_count, k_compact_scan, k_voxel_scatter: out holds the
// cells kept, in order of first appearance; words[VOXEL_WORD_KEPT] their number (the scan's total), words[VOXEL_WORD_ERROR] is non-zero
// if a probe ran through the whole table (it cannot at this load factor)
int launch_voxel_grid(const float *cloud, long long n, float leaf, long long min_points, bool centroid, const VoxelTable &T, unsigned *slot_of,
                      const CompactScratch &s, unsigned long long *words, const VoxelOut &out, void *stream);
// one correspondence pass of the turntable refinement (sl3d_align.hip, sl3d_align.h; the rule: include/sl3d_align.h, sl3d_align_sums): pair j
// is (source view first_view + j + 1, target view first_view + j), window 0 .. ALIGN_MAX_WINDOW; record: [n_pairs][ALIGN_WORDS] 64-bit words,
// cleared on the stream by the launcher itself in front of k_align_pass
int launch_align_pass(const KParams &P, int first_view, int n_pairs, int window, const ::AlignCam &cam, const ::AlignPass &a, unsigned long long *record,
                      void *stream);
// the point-to-plane form (sl3d_align_plane.hip, sl3d_align_plane.h; the rule: include/sl3d_align_plane.h).  k_align_normals over views
// [first_view, first_view + n_views): normals is the plane of first_view, the views' planes 3 * px_view_stride floats apart and laid out
// like points.  k_align_plane_pass: pairs as launch_align_pass, a.Q the scale of the lengths (align_plane_Q), normals the plane of the first target view, record: [n_pairs]
// [ALIGN_PLANE_WORDS] words cleared on the stream by the launcher itself
int launch_align_normals(const KParams &P, int first_view, int n_views, float normal_edge, float *normals, void *stream);
int launch_align_plane_pass(const KParams &P, int first_view, int n_pairs, int window, const ::AlignCam &cam, const ::AlignPass &a,
                            const float *normals, unsigned long long *record, void *stream);
// the TSDF volume (sl3d_tsdf.hip, sl3d_tsdf.h; the rule: include/sl3d_tsdf.h).  launch_tsdf_integrate: views [first_view, first_view +
// n_views) into the planes sum / weight of vol; turns: [n_views] rotations on the device; depth: n_views * px_view_stride doubles, the
// views' depth planes (k_tsdf_depth fills them first); words: TSDF_WORDS 64-bit words, the two of an
// integration cleared on the stream by the launcher itself.  launch_tsdf_count: k_tsdf_count and k_compact_scan over s.cnt / s.off (a
// slot per 1024 voxels), the two words of an extraction cleared likewise; launch_tsdf_scatter: the crossings into arrays of at least
// words[TSDF_WORD_CROSSINGS] rows
int launch_tsdf_integrate(const KParams &P, int first_view, int n_views, const ::AlignCam &cam, const ::TsdfVolume &vol, double tx, double tz,
                          const ::TsdfTurn *turns, double *depth, int32_t *sum, uint32_t *weight, unsigned long long *words, void *stream);
int launch_tsdf_count(const ::TsdfPlanes &planes, const ::TsdfVolume &vol, const CompactScratch &s, unsigned long long *words, void *stream);
int launch_tsdf_scatter(const ::TsdfPlanes &planes, const ::TsdfVolume &vol, const CompactScratch &s, float *xyz, float *normals, int32_t *edge,
                        void *stream);
// the mesh stage (sl3d_mesh.hip, sl3d_mesh.h): the faces of views [first_view, first_view + n_views) over their dense result.  A row has
// mesh_row_chunks(P) chunks (1024 pixels of one row), a view mesh_chunks(P) = H times as many; s: the mesh form of CompactScratch,
// faces: [max_views][face_stride][3] vertex ids into the view's compacted cloud (launch_compact_views)
int mesh_row_chunks(const KParams &P);
int mesh_chunks(const KParams &P);
inline size_t mesh_face_stride(const KParams &P)  // the faces a view can have (an allocation of at least 1)
{
    const size_t n = 2 * (size_t)(P.W - 1) * (size_t)(P.H - 1);
    return n ? n : 1;
}
// what every launch_mesh_* starts from: chunks per row / per view, the grid of a kernel over every chunk of the launch's views, the input
// planes and the pixel offset of its first view; sliced(s, k): a chunk scratch of k count arrays per view from that view on
struct MeshLaunch {
    int nck, n_chunks, first_view, n_views;
    dim3 grid;
    ViewPlanes in;
    size_t v0;
    CompactScratch sliced(const CompactScratch &s, int k) const
    {
        return {s.cnt + (size_t)first_view * k * n_chunks, s.off + (size_t)first_view * k * n_chunks, s.tot + (size_t)k * first_view};
    }
};
inline MeshLaunch mesh_launch(const KParams &P, int first_view, int n_views)
{
    const int nck = mesh_row_chunks(P);
    return {nck, P.H * nck, first_view, n_views, dim3(nck, P.H, n_views), view_planes(P, first_view), (size_t)first_view * P.px_view_stride};
}
int launch_mesh_views(const KParams &P, int first_view, int n_views, float max_edge, const CompactScratch &s, int *faces, size_t face_stride,
                      void *stream);
// vertex normals of those meshes (sl3d_mesh_normals.hip): s: the normals form of CompactScratch, normals: [max_views][normal_stride][3],
// view v's in the order of its compacted cloud
int launch_mesh_normals(const KParams &P, int first_view, int n_views, float max_edge, const CompactScratch &s, float *normals,
                        size_t normal_stride, void *stream);
// The cell pass of the components and the smoothing calls (k_mesh_cells, sl3d_mesh.hip) and the scan behind it: mesh_cell of every cell
// once, left in cells ([max_views][px_view_stride], a byte per cell: cc_cell_code); c: the launch's slice of a [max_views][mesh_chunks]
// scratch -- valid pixels per chunk, their scan, the views' totals.  labels != NULL: the union-find variant -- label of a pixel = its
// own index, size = 0, stat (the launch's first view's) zeroed
int launch_mesh_cells(const KParams &P, const MeshLaunch &L, float max_edge, uint8_t *cells, int *labels, int *sizes, unsigned long long *stat,
                      const CompactScratch &c, void *stream);
// The totals of a components / filter call: ONE device array of 5 words per view of the context, read back whole once per call.  `at`:
// the array or its host copy, mv: the context's max_views
struct CcTotals {
    unsigned long long *at;
    size_t mv;
    unsigned long long *vertices(int v) const { return at + v; }                   // [mv] vertices (the cell pass's scan)
    unsigned long long *kept(int v) const { return at + mv + 2 * (size_t)v; }      // [mv][2] kept vertices, kept faces (the filter's scan)
    unsigned long long *stat(int v) const { return at + 3 * mv + 2 * (size_t)v; }  // [mv][2] components, failure word
    size_t words() const { return 5 * mv; }
};
// connected components of those meshes and the meshes without their small components (sl3d_mesh_components.hip, sl3d_mesh_components.h).
// Every plane is [max_views][px_view_stride]: cells = a byte per cell (cc_cell_code), labels = the union-find over pixel indices (after the
// launch: every valid pixel's root), vid = vertex id of a pixel, sizes = vertices of the component at its root's pixel.  s: cnt / off
// [max_views][mesh_chunks] valid pixels per chunk and their scan, tot = CcTotals::vertices; stat: CcTotals::stat;
// labels_out: [max_views][px_view_stride] labels in vertex-id order, or NULL: the caller only wants the state the filter starts from
struct CcBuffers {
    uint8_t *cells;
    int *labels, *vid, *sizes;
    CompactScratch s;
    unsigned long long *stat;
    int *labels_out;
};
// the filtered mesh: keep = 0/1 byte per pixel; s: cnt / off [max_views][2][mesh_chunks] (kept vertices, kept faces per chunk), tot =
// CcTotals::kept; xyz [max_views][px_view_stride][3], ids [max_views][px_view_stride], faces [max_views][face_stride][3]
struct CcFiltered {
    uint8_t *keep;
    CompactScratch s;
    float *xyz;
    int *ids, *faces;
    size_t face_stride;
};
int launch_mesh_components(const KParams &P, int first_view, int n_views, float max_edge, const CcBuffers &b, void *stream);
// behind launch_mesh_components over the same views: vertices of components of >= min_vertices vertices, and the faces among them
int launch_mesh_filter(const KParams &P, int first_view, int n_views, int min_vertices, const CcBuffers &b, const CcFiltered &f, void *stream);
// its first launch alone: f.keep (and the counts in f.s.cnt) of those views, nothing scanned, nothing emitted
int launch_mesh_keep(const KParams &P, int first_view, int n_views, int min_vertices, const CcBuffers &b, const CcFiltered &f, void *stream);
// smoothing of those meshes (sl3d_mesh_smooth.hip, sl3d_mesh_smooth.h).  cells / rings: [max_views][px_view_stride] a byte per cell
// (cc_cell_code) / per pixel (smooth_ring); plane[2]: [max_views][px_view_stride][3] the ping-pong planes of the steps -- step s writes
// plane[s & 1], and plane[smooth_steps & 1], the one the last step did not write, takes the compacted vertices (view v's at 3 * v *
// px_view_stride); s: cnt / off [max_views][mesh_chunks] valid pixels per chunk and their scan, tot [max_views]; normals:
// [max_views][px_view_stride][3] in vertex-id order, or NULL: no normals asked for
struct SmoothBuffers {
    uint8_t *cells, *rings;
    float *plane[2];
    CompactScratch s;
    float *normals;
};
inline int smooth_steps(int iterations, float mu) { return iterations * (mu != 0.0f ? 2 : 1); }  // a step with mu == 0 is left out
int launch_mesh_smooth(const KParams &P, int first_view, int n_views, float max_edge, int iterations, float lambda, float mu, bool fix_boundary,
                       const SmoothBuffers &b, void *stream);
// the level-of-detail mesh (sl3d_mesh_lod.hip, sl3d_mesh_lod.h): one vertex per step x step block of a view's pixels.  The coarse grid is
// a dense result of its own -- valid / points planes of W' x H' pixels, rows a multiple of 16 apart -- so a KParams that carries it feeds
// launch_compact_views, launch_mesh_views and launch_mesh_normals as they stand
inline KParams lod_params(const KParams &P, int step, uint8_t *valid, float *points)
{
    KParams C = P;
    C.W = (P.W + step - 1) / step, C.H = (P.H + step - 1) / step;
    C.pitch = (C.W + 15) & ~15;
    C.px_view_stride = (size_t)C.pitch * (size_t)C.H;
    C.valid = valid, C.points = points;
    return C;
}
// where the candidates of the fine views come from: cand [max_views][px_view_stride] 0/1 bytes; their ids in the view's compacted cloud
// either from offsets -- the candidates are the valid pixels: the launch's slice of the scan launch_mesh_cells left, [view][mesh_chunks]
// -- or, offsets == NULL, from vid [max_views][px_view_stride] (CcBuffers::vid)
struct LodSource {
    const uint8_t *cand;
    const unsigned long long *offsets;
    const int *vid;
};
// everything over the coarse grid Pc = lod_params(...): ids = the id plane beside Pc.valid / Pc.points; blk / chk / nrm: the scratch of
// launch_compact_views / launch_mesh_views / launch_mesh_normals at Pc's sizes; xyz, normals [max_views][Pc.px_view_stride][3],
// vertex_ids [max_views][Pc.px_view_stride], faces [max_views][face_stride][3]
struct LodBuffers {
    int *ids;
    CompactScratch blk, chk, nrm;
    float *xyz, *normals;
    int *vertex_ids, *faces;
    size_t face_stride;
};
int launch_mesh_lod(const KParams &P, const KParams &Pc, int first_view, int n_views, int step, float lod_edge, bool mean, const LodSource &src,
                    const LodBuffers &b, bool normals, void *stream);
// the ids of a grid's valid pixels in vertex order (k_lod_ids, sl3d_mesh_lod.hip): ids = the id plane beside Pc.valid, chk = the scratch
// launch_mesh_views left over Pc, vertex_ids [max_views][Pc.px_view_stride]
int launch_mesh_ids(const KParams &Pc, int first_view, int n_views, const CompactScratch &chk, const int *ids, int *vertex_ids, void *stream);
// the hole filling (sl3d_mesh_holes.hip, sl3d_mesh_holes.h): the small interior holes of a view's candidate map filled from their rims.
// The filled grid F -- P with valid / points planes of its own -- is a dense result, so it feeds launch_compact_views, launch_mesh_views
// and launch_mesh_normals as they stand.  labels / sizes [max_views][px_view_stride]: the union-find over the non-candidate pixels and
// the pixels of a component at its root; ids: the id plane beside F.valid / F.points; hol: cnt / off [max_views][2][mesh_chunks] (holes,
// filled pixels per chunk), tot [max_views][2]; failed [max_views]: a word set when an iteration bound ran out; blk / chk / nrm, xyz,
// normals, vertex_ids, faces: as LodBuffers', at P's sizes
struct HoleBuffers {
    int *labels, *sizes, *ids;
    unsigned long long *failed;
    CompactScratch hol, blk, chk, nrm;
    float *xyz, *normals;
    int *vertex_ids, *faces;
    size_t face_stride;
};
int launch_mesh_holes(const KParams &P, const KParams &F, int first_view, int n_views, float max_edge, int max_hole, float fill_edge, const LodSource &src,
                      const HoleBuffers &b, bool normals, void *stream);
int launch_register(const float *in, float *out, long n, const float R4[4], float tx, float ty, float tz, void *stream);
int launch_synth(const KParams &P, const DevCal &C, const SynthParams &S, int view, void *stream);
int launch_undistort(const uint8_t *src, size_t sstride, uint8_t *dst, size_t dstride, int width, int height, int cn, const double K[9],
                     const double dist[5], short *m1, unsigned short *m2, bool build_map, void *stream);
int launch_undistort_planes(const uint8_t *src, size_t spitch, size_t splane, uint8_t *dst, size_t dpitch, size_t dplane, int width, int height,
                            int n_planes, const double K[9], const double dist[5], short *m1, unsigned short *m2, bool build_map, void *stream);
int launch_pattern(uint8_t *dst, size_t pitch, int PW, int PH, int axis, const uint8_t *profile, void *stream);
int launch_atan_selfcheck(const float *tab_phi, const float *tab_shift, unsigned *mismatches, void *stream);

}  // namespace sl3d
