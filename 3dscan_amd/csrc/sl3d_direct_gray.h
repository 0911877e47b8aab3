// sl3d_direct_gray.h -- the Gray decode of SL3D_FLAG_DIRECT_GRAY: a Gray frame thresholded against the MEAN of the pixel's fringe
// frames instead of against its inverse frame, so that the inverse frames need not be projected, captured or uploaded at all.
//
// Shared by k_unwrap_direct (sl3d_direct_gray.hip, the staged route), k_direct_gray (the same unit, the timed route), sl3d_create /
// sl3d_group_create (the refusals), the upload paths (which planes of a view a context reads) and the CPU check the test suite runs
// (tests/native/direct_gray_check.cpp): plain C++, integers only, no HIP types.
//
// The reference's fringe steps are Pi/2 apart (1/pattern_generator.cpp:302,342), so fringe frames 0 and 2 are half a period apart and
// I0 + I2 is twice the pixel's mean intensity, for 3 and for 4 steps: the level halfway between a lit and a dark Gray stripe.  Bit i of an
// axis of a pixel, with gray_i the byte of Gray plane i and I0, I2 fringe bytes 0 and 2 of the SAME axis of the same view:
//   G_i = (2 * (int)gray_i - ((int)I0 + (int)I2) >= 0)          ties -> 1, as pos - inv >= 0 in 4/phase_unwrap.cpp:183
// Everything behind the bit -- the XOR chain, code, shift_pi, unwrap_value, stage 5, the anchored coordinate, the solves -- is unchanged.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SL3D_DIRECT_GRAY_FN __host__ __device__ __forceinline__
#else
#define SL3D_DIRECT_GRAY_FN static inline
#endif

#define SL3D_DIRECT_GRAY_BIT 4096u

// G_i.  gray, i0, i2: bytes, 0..255
SL3D_DIRECT_GRAY_FN int direct_gray_bit(int gray, int i0, int i2) { return 2 * gray - (i0 + i2) >= 0 ? 1 : 0; }

// stage 4's code of one axis of a pixel from its Gray bytes (most significant plane first): 4/phase_unwrap.cpp:187-193 over the bits above
SL3D_DIRECT_GRAY_FN int direct_gray_code(const unsigned char *gray, int n_gray, int i0, int i2)
{
    int b = 0, code = 0;
    for (int i = 0; i < n_gray; i++) {
        b ^= direct_gray_bit(gray[i], i0, i2);
        code = code * 2 + b;
    }
    return code;
}

// The same bit and the same chain for the four pixels of one dword of a u8 plane at once (k_direct_gray: a lane owns such a quad), two
// pixels per 32-bit word in 16-bit fields: word `odd` = 0 holds pixels 0 (low field) and 2 (high field), word 1 pixels 1 and 3.
//   direct_gray_sum2   per field I0 + I2 (<= 510) of the fringe dwords i0, i2
//   direct_gray_bit2   per field G of the Gray dword: the field's (2 * gray + 0x8000) - (I0 + I2) never borrows (0x8000 > 510), and its bit
//                      15 is set iff 2 * gray - (I0 + I2) >= 0 -- direct_gray_bit, ties included
//   direct_gray_step2  the chain per field: b ^= G; code = code * 2 + b.  A code of up to 16 planes fills its field exactly
//   direct_gray_field  pixel k's field of the pair of words
// (tests/native/direct_gray_check.cpp runs them against direct_gray_bit / direct_gray_code over every (gray, I0 + I2).)
SL3D_DIRECT_GRAY_FN unsigned direct_gray_sum2(unsigned i0, unsigned i2, int odd)
{
    return ((i0 >> (8 * odd)) & 0x00ff00ffu) + ((i2 >> (8 * odd)) & 0x00ff00ffu);
}
SL3D_DIRECT_GRAY_FN unsigned direct_gray_bit2(unsigned gray, unsigned sum2, int odd)
{
    return ((((((gray >> (8 * odd)) & 0x00ff00ffu) << 1) | 0x80008000u) - sum2) >> 15) & 0x00010001u;
}
SL3D_DIRECT_GRAY_FN void direct_gray_step2(unsigned gray, unsigned sum2, int odd, unsigned &b2, unsigned &code2)
{
    b2 ^= direct_gray_bit2(gray, sum2, odd);
    code2 = (code2 << 1) + b2;
}
SL3D_DIRECT_GRAY_FN int direct_gray_field(unsigned even2, unsigned odd2, int k) { return (int)((((k & 1) ? odd2 : even2) >> (16 * (k >> 1))) & 0xffffu); }

// the planes of a coded axis such a context reads (frame_plane_runs, sl3d_ctx.h: what the upload paths copy): the F fringe planes and the N
// Gray planes behind them, never the N inverse planes
SL3D_DIRECT_GRAY_FN int direct_gray_planes(int n_fringe, int n_gray) { return n_fringe + n_gray; }

// The refusal of a flag combination by sl3d_create / sl3d_group_create, before a device is touched: NULL, or the text that goes with
// SL3D_E_UNSUPPORTED
SL3D_DIRECT_GRAY_FN const char *direct_gray_refusal(bool direct, bool subpixel, bool repair)
{
    if (!direct) return 0;
    if (!subpixel)
        return "SL3D_FLAG_DIRECT_GRAY needs SL3D_FLAG_SUBPIXEL: the integer scan's kernel reads the inverse Gray frames (add SL3D_FLAG_SUBPIXEL, or drop "
               "the flag)";
    if (repair)
        return "SL3D_FLAG_DIRECT_GRAY | SL3D_FLAG_REPAIR_PERIODS is not supported: the fused period repair has no direct form (drop one of the two "
               "flags; sl3d_repair_periods works on a SL3D_FLAG_KEEP_STAGES context)";
    return 0;
}
