// sl3d_fused_launch.hip -- launch_fused: grid shape, views per lane and the k_fused instantiation (sl3d_fused_choice.h: the rule).
// The instantiations themselves live in the sl3d_fused_*.hip translation units (a few families each); this unit only looks them up,
// and does not see the kernel.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <utility>

#include "sl3d_internal.h"

namespace sl3d {

// number of 1024-pixel tiles (= blocks along x that own pixels) of one view
int fused_tiles(const KParams &P)
{
    const long quads = (long)(P.pitch >> 2) * P.H;
    return (int)((quads + SL3D_BLOCK - 1) / SL3D_BLOCK);
}

// views per lane: as many as possible up to SL3D_VPT_MAX (amortises the set-up of a block and the camera table entries) while
// the grid still has >= ~16 blocks per CU to balance the tail (8 until the end of round 4: with the repaired pipeline 3 / 4 views of
// 1080p run 1 % / 0.4 % faster at one view per lane than at two, 8 views the same at two as at four -- profiles/r04_vpt_final.txt).
// (Rounds 1-2: at most 8 views per lane.  With the stores streaming past the L2 the optimum moved: 16 views per launch 354.5 us at 4 against 359.6 at 8 and 359.3 at 2, 372.7 at 16; 32 views 700 against 708,
// profiles/r03_vpt_sweep4.txt; configs[2], 3 views of 12 Mpx: 1 / 2 / 3 views per lane 0.670 / 0.681 / 0.685,
// profiles/c2_r04_views_vpt_sweep.txt.)
#define SL3D_VPT_MAX 4
#define SL3D_BLOCK_SLOTS 1024 /* blocks of the fused kernel resident at once: 256 CUs x SL3D_OCC */
static int views_per_lane(unsigned bx, int n_views, int cam_table_kind, bool small)
{
    int vpt = 1;
    // (a two-double camera table -- tangential terms -- costs a block 16 B/px: those rigs keep 8 views per lane, measured -0.6 % at 4)
    const int cap = cam_table_kind == 2 ? 8 : SL3D_VPT_MAX;
    // (large launches -- early requests, the block's LDS tables filled under them -- want their 4 views per lane as soon as one round
    // of blocks is left: 5 / 6 / 8 / 12 views of 1080p +1.3...1.7 % at 4 views per lane against 2, profiles/r04_vpt_final.txt)
    const long min_blocks = small ? 4096 : SL3D_BLOCK_SLOTS;
    while (vpt < cap && vpt < n_views && (long)bx * ((n_views + 2 * vpt - 1) / (2 * vpt)) >= min_blocks) vpt *= 2;
#ifdef SL3D_MEASURE
    if (getenv("SL3D_VPT") && atoi(getenv("SL3D_VPT")) >= 1) vpt = atoi(getenv("SL3D_VPT"));
#endif
    return vpt;
}

// what the rule looks at (sl3d_fused_choice.h)
static FusedShape fused_shape(const KParams &P, int rig, int n_views, bool keep, int cmode, bool prefer_gated, bool maskin)
{
    return {keep, P.F, P.Nv, P.Nh, n_views, rig, cmode, prefer_gated, maskin, P.proj_disp != nullptr, P.proj_rad != nullptr,
            P.cam_tab != nullptr && P.cam_tab_kind == 2};
}

FusedKey fused_choice(const KParams &P, int rig, int n_views, bool keep, int cmode, bool prefer_gated, bool maskin)
{
#ifdef SL3D_MEASURE
    // (every launch takes the large-launch instantiation, as if it had more views)
    if (getenv("SL3D_NO_SMALL") && n_views <= SL3D_SMALL_LAUNCH_VIEWS) n_views = SL3D_SMALL_LAUNCH_VIEWS + 1;
#endif
    return fused_key(fused_shape(P, rig, n_views, keep, cmode, prefer_gated, maskin));
}

// the launcher of key k: from its family's table (a family no unit instantiates is a null weak reference: sl3d_internal.h)
template <int... F>
static FusedLauncher fused_launcher(const FusedKey &k, std::integer_sequence<int, F...>)
{
    static FusedTable (*const tables[])() = {&fused_table<F>...};
    if (k.nmax == 0 || !tables[fused_family_id(k)]) return nullptr;
    const FusedTable t = tables[fused_family_id(k)]();
    for (int i = 0; i < t.n; i++)
        if (t.entry[i].key == k) return t.entry[i].launch;
    return nullptr;
}

unsigned fused_maskin_part_stride(const KParams &P)
{
    const long quads = (long)(P.pitch >> 2) * P.H;
    return 4u * (((unsigned)((quads + SL3D_SMALL_BLOCK - 1) / SL3D_SMALL_BLOCK) + 7u) & ~7u);
}
unsigned fused_maskin_part_words(const KParams &P) { return (unsigned)(((long)(P.pitch >> 2) * P.H + 63) / 64); }

int launch_fused(const KParams &P_, const DevCal *d_cal, int rig, int first_view, int n_views, bool keep, int cmode, void *stream, bool prefer_gated,
                 const MaskIn *mi, FusedKey &ran)
{
    KParams P = P_;
    P.prefer_gated = prefer_gated ? 1 : 0;
    const FusedKey k = fused_choice(P, rig, n_views, keep, cmode, prefer_gated, mi != nullptr);
    const FusedLauncher launch = fused_launcher(k, std::make_integer_sequence<int, FUSED_FAMILIES>());
    if (!launch) return (int)hipErrorInvalidValue;  // (a MASKIN launch the shape has no kernel for, or a key no unit compiled)
    if (mi) P.mi = *mi;
    const long quads = (long)(P.pitch >> 2) * P.H;
    const unsigned bx = ((unsigned)((quads + SL3D_BLOCK - 1) / SL3D_BLOCK) + 7u) & ~7u;  // a multiple of 8: consecutive tiles go round the 8 XCDs
    // (`small` is the SIZE of the launch, not the kernel it takes: a launch of up to 4 sparsely selected views runs the large-launch
    // kernel (prefer_gated) but keeps the views-per-lane rule of small launches -- the A/B that chose that kernel for sparse
    // selections, profiles/r04_sparse_mask.txt, was measured with it; following the kernel instead is 5-12 % slower at 19 % / 5 %
    // coverage with 4 views per launch, 1-4 % faster at 50 %: profiles/r05_sparse_small_launch_vpt_ab.txt)
    // (a MASKIN launch: one view per item -- nothing of a next view is in flight beside the selection bytes)
    const bool small = fused_small_launch(fused_shape(P, rig, n_views, keep, cmode, prefer_gated, mi != nullptr));
    const int vpt = mi ? 1 : views_per_lane(bx, n_views, P.cam_tab != nullptr ? P.cam_tab_kind : 0, small);
    const unsigned block = (unsigned)fused_traits(k).block;
    const unsigned gx = ((unsigned)((quads + block - 1) / block) + 7u) & ~7u;
    // the timed kernels read the camera-side T1 from the per-calibration table whatever the batch is: with 8 views per lane it
    // costs nothing (1 B/px/view), with 1..4 it saves the iteration (+2..13 %), and a view's result does not depend on the
    // batch it was launched in
    P.use_cam_table = P.cam_tab != nullptr ? P.cam_tab_kind : 0;
#ifdef SL3D_MEASURE
    if (getenv("SL3D_CAMTAB") && atoi(getenv("SL3D_CAMTAB")) == 0) P.use_cam_table = 0;
#endif
    (void)hipGetLastError();  // an earlier sticky error of another library is not this launch's
    launch(gx, (unsigned)((n_views + vpt - 1) / vpt), block, stream, P, d_cal, first_view, n_views, vpt);
    const int rc = (int)hipGetLastError();
    if (rc == hipSuccess) ran = k;
    return rc;
}

}  // namespace sl3d
