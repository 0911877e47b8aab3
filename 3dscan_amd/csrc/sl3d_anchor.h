// sl3d_anchor.h -- the anchored projector coordinate of SL3D_FLAG_ANCHOR_PERIODS: the fringe period nearest the centre of the
// pixel's Gray cell instead of the Gray code itself, and the fringe period measured with pi instead of 22/7.
//
// Shared by k_subpixel / k_subpixel_coords (sl3d_subpixel.hip), k_subpixel_fused (sl3d_subpixel_fused.hip), sl3d_create /
// sl3d_group_create (the refusals) and the CPU check the test suite runs (tests/native/anchor_check.cpp): plain C++, no HIP types.
//
// The reference's generator and decoder write Pi = 22/7 inside and around a real cos / atan2: the Gray cell is fw projector pixels wide,
// the projected fringe has the period fw * pi / (22/7).  Stage 4's  w + code * 2Pi  therefore mixes two period lengths: the continuous
// coordinate is off by p * (22/7 - pi) / (22/7), and the wrap of the phase drifts away from the Gray edge, a period jump behind every
// edge.  Per axis of a pixel, with  w  the float stage 4 leaves in the wrapped-phase plane (shift_pi(phi)) and  code  stage 4's int, all
// in IEEE double without contraction, in this order:
//   a  = (double)w + c_F                               c_3 = 0, c_4 = 0.75 * (pi - 22/7): what the four shifts of Pi/2 leave in the phase
//   m  = rint((((double)code + 0.5) * P2 - a) * INV)   the fringe period nearest the cell's centre; round half to even
//   xs = (double)fw * ((a + TWOPI * m) / P2)
// applied to an axis only where stage 4's loop runs (anchor_applies) and only if the axis has Gray planes; elsewhere the coordinate stays
// correspond_arg(unwrapped) (sl3d_device.h).  Validity, c_p_map and every stage plane are not touched.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SL3D_ANCHOR_FN __host__ __device__ __forceinline__
#else
#define SL3D_ANCHOR_FN static inline
#endif

#include <math.h>

#define SL3D_ANCHOR_P2 ((2.0 * 22.0) / 7.0)          /* the project's TWO_PI_REF: (2.0*Pi) of the reference */
#define SL3D_ANCHOR_TWOPI (2.0 * 3.141592653589793)
#define SL3D_ANCHOR_INV 0.15915494309189535          /* 1 / TWOPI, as this literal */

// c_F: the phase the generator's offset and its shifts leave beside the 3-step form (5 steps decode nothing)
SL3D_ANCHOR_FN double anchor_phase_offset(int n_fringe) { return n_fringe == 4 ? 0.75 * (3.141592653589793 - 22.0 / 7.0) : 0.0; }

// the fringe period nearest the centre of Gray cell `code`
SL3D_ANCHOR_FN double anchor_period(double a, int code) { return rint((((double)code + 0.5) * SL3D_ANCHOR_P2 - a) * SL3D_ANCHOR_INV); }

// the anchored continuous projector coordinate of one axis of a pixel
SL3D_ANCHOR_FN double anchor_coordinate(float w, int code, int fw, int n_fringe)
{
    const double a = (double)w + anchor_phase_offset(n_fringe);
    const double m = anchor_period(a, code);
    return (double)fw * ((a + SL3D_ANCHOR_TWOPI * m) / SL3D_ANCHOR_P2);
}

// does the formula apply to this axis of a pixel?  pos / full: the pixel's frame column and the frame's width (vertical axis), its frame
// row and the frame's height (horizontal axis): stage 4's loop, 4/phase_unwrap.cpp:285 / :304
SL3D_ANCHOR_FN bool anchor_applies(int n_gray, int pos, int full) { return n_gray > 0 && pos >= 1 && pos <= full - 2; }

// The refusal of a flag combination by sl3d_create / sl3d_group_create, before a device is touched: NULL, or the text that goes with
// SL3D_E_UNSUPPORTED.  (The repair turns `code` from "Gray cell" into "fringe index": the pixel then sits at the edge of that cell, where
// anchoring to its centre is a coin flip.)
SL3D_ANCHOR_FN const char *anchor_refusal(bool anchor, bool subpixel, bool repair)
{
    if (!anchor) return 0;
    if (!subpixel)
        return "SL3D_FLAG_ANCHOR_PERIODS needs SL3D_FLAG_SUBPIXEL: the integer scan has no use for the anchored coordinate (add SL3D_FLAG_SUBPIXEL, "
               "or drop the flag)";
    if (repair)
        return "SL3D_FLAG_ANCHOR_PERIODS | SL3D_FLAG_REPAIR_PERIODS is not supported: the repair turns code from the Gray cell into a fringe index, "
               "which leaves nothing to anchor to (choose one of the two flags)";
    return 0;
}
