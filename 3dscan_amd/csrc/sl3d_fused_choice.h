// sl3d_fused_choice.h -- WHICH k_fused instantiation a launch runs: the rule as one constexpr function of the launch's shape, free of
// HIP so that the same code runs in a CPU test (tests/native/fused_choice_check.cpp, tests/test_fused_choice.py).  Everything else is
// derived from it: the instantiations the sl3d_fused_*.hip units compile (fused_family), the launcher launch_fused looks up, and the
// names sl3d_fused_kernel_name / sl3d_last_fused_kernel_name print.
//
// Instantiations: the timed 3-step kernel exists for every N = 6..12 with both axes equal (EXACT), as padded straight-line code for
// every NMAX = 6..12 (any other pair of axes up to NMAX planes -- issue_gray; the 4-/5-step fringes have this form only) and with
// the unroll bound 16 beyond; the parity mode uses the bounds 8 / 12 / 16 with per-plane tests.  Dense 3-step launches
// of at most SL3D_SMALL_LAUNCH_VIEWS views take the instantiation without the LDS reciprocal table (re-measured with the streaming
// stores: 8 views 185.6-187.5 us through it against 183.8-184.7, 16 views +-0: stays at 4).
#pragma once
#include <stdio.h>

#define SL3D_MAX_GRAY 16
#define SL3D_SMALL_LAUNCH_VIEWS 4  // launches of at most this many views take the small-launch instantiation (sl3d_fused.h)
#define SL3D_BLOCK 256 /* threads per block of the fused kernel: a block is a 1024-pixel tile of the scan, 4 waves = 4 segments of 256 pixels */
#define SL3D_SMALL_BLOCK SL3D_BLOCK /* the small-launch instantiation keeps 256-thread blocks too (round 4: 128 / 64 threads +-0.5 %) */

namespace sl3d {

// the template arguments of k_fused (sl3d_fused.h: what each one means), as values.  nmax == 0: no kernel.
struct FusedKey {
    bool keep = false;
    int nmax = 0;
    bool fgen = false, exact = false;
    int rig = 0, cmode = 0;  // cmode: 0 / 2 (dense / segmented clouds) + 4 (MASKIN)
    bool rcpt = false, early = false;
};
constexpr bool operator==(const FusedKey &a, const FusedKey &b)
{
    return a.keep == b.keep && a.nmax == b.nmax && a.fgen == b.fgen && a.exact == b.exact && a.rig == b.rig && a.cmode == b.cmode && a.rcpt == b.rcpt &&
           a.early == b.early;
}

// what a key implies: every switch k_fused derives from its template arguments, stated once -- the kernel and its helpers read it
// (sl3d_fused.h: FusedKernel), launch_fused takes the block size from it, and the CPU check asserts `legal` for every compiled key
struct FusedTraits {
    bool seg;     // CMODE bit 2: segmented clouds instead of dense planes
    bool maskin;  // CMODE bit 4: the launch evaluates the views' raw selection itself
    bool pipe;    // the timed kernels of the camera-frame rigs: the planes of view v + 1 are requested in the middle of view v, the
                  // block's LDS tables are filled under the item's first requests, the results of view v leave behind the decode of v + 1
    bool early;   // the first view's planes of an item are requested before its mask is known
    bool split;   // ... and stage 3 runs ahead of the wait for the Gray planes
    bool unroll;  // the small-launch instantiation: both pixel pairs of phases A and B in one basic block
    int block;    // threads per block
    int planes;   // how an axis with N Gray planes maps onto the NMAX unrolled ones (sl3d_fused.h: issue_gray)
    bool legal;   // a combination k_fused compiles
};
constexpr FusedTraits fused_traits(const FusedKey &k)
{
    FusedTraits t = {};
    t.seg = (k.cmode & 2) != 0;
    t.maskin = (k.cmode & 4) != 0;
    t.pipe = !k.keep && k.rig != 0;
    t.early = k.early;
    t.split = k.early;
    t.unroll = !k.rcpt;
    t.block = k.rcpt ? SL3D_BLOCK : SL3D_SMALL_BLOCK;
    // exact; padded (the timed kernels up to 12 planes; 3: the pad count through v_readfirstlane, the gated MASKIN kernels); tests
    t.planes = k.exact ? 1 : (!k.keep && k.nmax <= 12) ? ((t.maskin && k.rcpt) ? 3 : 2) : 0;
    t.legal = (k.cmode & ~6) == 0 &&  // 0 = dense planes, 2 = segmented clouds (1 was round 2's look-back compaction), + 4 = MASKIN
              // MASKIN: the pipelined small-launch instantiations, and the gated large-launch ones (views known to be sparsely selected)
              (!t.maskin || (t.pipe && (k.rcpt ? !k.early : k.early))) &&
              !(k.keep && k.cmode != 0) &&  // the parity mode writes dense planes
              !(k.keep && k.rig != 0) &&    // the parity mode evaluates everything with the reference's operation order
              // early requests: the pipelined kernels only; the small-launch instantiation: early requests iff pipelined
              (k.early ? t.pipe : (k.rcpt || !t.pipe));
    return t;
}

// what the rule looks at: the launch, and the calibration facts the rig classes need
struct FusedShape {
    bool keep;             // the parity mode
    int F, nv, nh;         // fringe steps, Gray planes per axis
    int n_views;
    int rig;               // the context's rig class (sl3d_fused.h: RIG); the timed kernels fold it at compile time
    int cmode;             // 0 = dense xyz + valid planes, 2 = segmented clouds
    bool prefer_gated;     // the views are sparsely selected (sl3d_capi_inputs.cpp: sparse_views)
    bool maskin;           // the launch evaluates the views' raw selection itself (sl3d_fused.h: maskin_request)
    bool proj_disp;        // the projector-side table exists (rig class 2)
    bool proj_rad;         // the projector's radial table exists (rig class 3)
    bool cam_tab2;         // the camera table is of the two-double kind (tangential terms)
};

// the rig class of the kernel (0 = the un-pipelined general kernel): more than 12 Gray planes on an axis take the general kernel
// whatever the calibration is -- it evaluates any rig, and it is the only one whose per-plane-test form does not spill; so does an axis
// without Gray planes (no plane to pad the straight-line kernels with)
constexpr int fused_rig(const FusedShape &s)
{
    if (s.keep || s.nv > 12 || s.nh > 12 || s.nv == 0 || s.nh == 0) return 0;
    return s.rig == 1 ? 1 : (s.rig == 2 && s.proj_disp) ? 2 : (s.rig == 3 && s.proj_rad && s.F == 3) ? 3 : 0;
}

// the SIZE of the launch: a handful of views of the reference's own fringes (one scan per call).  Such a launch takes the small-launch
// instantiation unless its views are sparsely selected (fused_key), and the views-per-lane rule of small launches either way (launch_fused)
constexpr bool fused_small_launch(const FusedShape &s) { return !s.keep && s.F == 3 && s.n_views <= SL3D_SMALL_LAUNCH_VIEWS; }

// THE rule.  prefer_gated: the views of the launch are sparsely selected -- a small launch then takes the large-launch instantiation,
// whose plane requests wait for the valid bits instead of going out first (one view of 1080p with 19 % of the frame selected, as in the
// reference's real captures: 15.8 us against 22.2; a full frame: 26.9 against 24.6 -- profiles/r04_sparse_mask.txt).
// A MASKIN launch exists for 3-step fringes, a pipelined rig class and a small launch: the small-launch form with early requests, or
// (views known to be sparsely selected) the gated large-launch form.  It compiles the one-double camera table only: its mask words
// live in the registers of the two-double kind.
constexpr FusedKey fused_key(const FusedShape &s)
{
    FusedKey k;
    const bool fgen = s.F != 3;
    const int rig = fused_rig(s);
    if (s.maskin && (s.keep || fgen || s.n_views > SL3D_SMALL_LAUNCH_VIEWS || rig == 0 || s.cam_tab2)) return k;
    const int m = s.nv > s.nh ? s.nv : s.nh;
    k.keep = s.keep;
    k.fgen = fgen;
    k.rig = rig;
    k.cmode = s.keep ? 0 : (s.cmode & 2) | (s.maskin ? 4 : 0);  // (the parity mode writes dense planes)
    k.exact = !s.keep && !fgen && s.nv == s.nh && s.nv >= 6 && s.nv <= 12;
    if (k.exact) k.nmax = s.nv;
    else if (!s.keep && m <= 12 && s.nv > 0 && s.nh > 0) k.nmax = m < 6 ? 6 : m;  // padded (4-/5-step fringes: always)
    else if (!s.keep) k.nmax = SL3D_MAX_GRAY;  // more than 12 planes, or an axis with NONE (sl3d_config allows 0): the per-plane tests
    else k.nmax = m <= 8 ? 8 : (m <= 12 ? 12 : SL3D_MAX_GRAY);
    const bool small = fused_small_launch(s) && !s.prefer_gated;
    k.rcpt = !small;
    // (early requests: the pipelined kernels only -- rig class 0 is the un-pipelined general kernel)
    k.early = small ? rig != 0 : rig != 0 && !fgen && !s.prefer_gated;
    return k;
}

// the key as rocprofv3 spells the kernel; returns snprintf's value
inline int fused_key_name(const FusedKey &k, char *buf, size_t cap)
{
    auto b = [](bool v) { return v ? "true" : "false"; };
    return snprintf(buf, cap, "sl3d::k_fused<%s, %d, %s, %s, %d, %d, %s, %s>", b(k.keep), k.nmax, b(k.fgen), b(k.exact), k.rig, k.cmode, b(k.rcpt), b(k.early));
}

// ---- families: the keys of one (keep, fgen, rig, cmode), compiled together by one sl3d_fused_*.hip unit -----------------------------
constexpr int FUSED_FAMILIES = 64, FUSED_FAMILY_MAX = 48;
constexpr int fused_family_id(bool keep, bool fgen, int rig, int cmode) { return (keep ? 32 : 0) | (fgen ? 16 : 0) | rig << 2 | cmode >> 1; }
constexpr int fused_family_id(const FusedKey &k) { return fused_family_id(k.keep, k.fgen, k.rig, k.cmode); }

struct FusedFamily {
    int n = 0;
    FusedKey key[FUSED_FAMILY_MAX] = {};
};
// a domain of shapes that is complete for every family: the key depends on the planes per axis, on the launch being small or not, on
// gating, and on the calibration facts only through the rig class (which the most permissive facts below all reach)
struct FusedDomain {
    int max_gray = SL3D_MAX_GRAY;
    int views[2] = {1, SL3D_SMALL_LAUNCH_VIEWS + 1};
};
constexpr FusedFamily fused_family(int id, FusedDomain d = {})
{
    FusedFamily f;
    bool seen[(SL3D_MAX_GRAY + 1) * 8] = {};  // (by nmax, exact, rcpt, early: what tells the keys of one family apart)
    const bool keep = (id & 32) != 0, fgen = (id & 16) != 0;
    const int rig = id >> 2 & 3, cmode = (id & 3) << 1;
    for (int nv = 0; nv <= d.max_gray; nv++)
        for (int nh = 0; nh <= d.max_gray; nh++)
            for (int n_views : d.views)
                for (int gated = 0; gated < 2; gated++) {
                    const FusedKey k = fused_key({keep, fgen ? 4 : 3, nv, nh, n_views, rig, cmode & 2, gated != 0, (cmode & 4) != 0, true, true, false});
                    const int slot = k.nmax * 8 + k.exact * 4 + k.rcpt * 2 + k.early;
                    if (k.nmax == 0 || fused_family_id(k) != id || seen[slot]) continue;
                    seen[slot] = true;
                    f.key[f.n++] = k;
                }
    return f;
}

}  // namespace sl3d
