// sl3d_exposure.h -- the rule of the exposure fusion (sl3d_fuse_exposures, include/sl3d_fuse.h: per pixel the exposure with the fewest clipped
// planes, among those the best modulated, among those the first): the score of one axis of one exposure and the packed key whose argmax
// over the exposures IS that lexicographic choice.
//
// Shared by k_fuse_exposures (sl3d_exposure.hip) and by the CPU check the test suite runs over every (I0, I1, I2) triple
// (tests/native/exposure_check.cpp): plain C, no HIP types, integers only.
//
//   S = t1*t1 + t2*t2, with t1 and t2 the integers stage 3 hands to atan2 for the axis:
//     F == 3:  t1 = I0 - I2,  t2 = 2*I1 - I0 - I2         |t1| <= 255, |t2| <= 510:  S <= 325125 < 2^19
//     F == 4:  t1 = I3 - I1,  t2 = I0 - I2                |t1|, |t2| <= 255:         S <= 130050
//   K = ((127 - n) << 22) | (q << 3) | (7 - e)            n <= 72 clipped planes, q = min of S over the coded axes, e <= 7:
//                                                         the three fields do not overlap (q < 2^19) and K < 2^29
// A larger K is: fewer clipped planes; then a larger q; then a smaller e.
#pragma once

#ifdef __HIPCC__
#define SL3D_EXP_FN __host__ __device__ __forceinline__
#else
#define SL3D_EXP_FN static inline
#endif

#define SL3D_EXP_MAX_SCORE 325125

// the score of one axis from its fringe bytes (i3 is read for F == 4 only)
SL3D_EXP_FN unsigned exp_score(int F, int i0, int i1, int i2, int i3)
{
    const int t1 = F == 4 ? i3 - i1 : i0 - i2;
    const int t2 = F == 4 ? i0 - i2 : 2 * i1 - i0 - i2;
    return (unsigned)(t1 * t1 + t2 * t2);
}

// the key of exposure e with n clipped planes and score q
SL3D_EXP_FN unsigned exp_key(unsigned n, unsigned q, unsigned e) { return ((127u - n) << 22) | (q << 3) | (7u - e); }

// what a key holds
SL3D_EXP_FN unsigned exp_key_exposure(unsigned key) { return 7u - (key & 7u); }
SL3D_EXP_FN unsigned exp_key_clipped(unsigned key) { return 127u - (key >> 22); }

// ---- the clip count on packed bytes ---------------------------------------------------------------------------------------------------
// A dword holds the bytes of one plane at 4 consecutive pixels.  exp_clipped4(w, T) has bit 0 of byte k set iff byte k of w is >=
// saturation (1 .. 256; 256: never), so the clip counts of 4 pixels add up as ONE dword add per plane (<= 72 planes: no carry between
// bytes).  With x = xh*128 + xl per byte, and s = sh*128 + sl the saturation:  (x | 0x80) - sl  has bit 7 set iff xl >= sl (every byte is
// >= 0x80 - 0x7f > 0: no borrow crosses a byte), and  x >= s  iff  sh == 0 ? (xh | xl >= sl) : (xh & xl >= sl).
struct ExpClipTest {
    unsigned sl;    // (saturation & 127) in every byte
    unsigned a, b;  // sh == 0: ~0, ~0;  sh == 1: 0, 0
    unsigned m;     // 0x80808080, or 0 for saturation == 256
};

SL3D_EXP_FN struct ExpClipTest exp_clip_test(int saturation)
{
    struct ExpClipTest t;
    t.sl = (unsigned)(saturation & 127) * 0x01010101u;
    t.a = t.b = saturation < 128 ? ~0u : 0u;
    t.m = saturation <= 255 ? 0x80808080u : 0u;
    return t;
}

SL3D_EXP_FN unsigned exp_clipped4(unsigned w, const struct ExpClipTest t)
{
    const unsigned ge = (w | 0x80808080u) - t.sl;
    return ((((w & t.a) | ge) & (w | t.b)) & t.m) >> 7;
}

// 0xff in every byte of c (bytes 0 .. 7) that equals e
SL3D_EXP_FN unsigned exp_bytes_equal(unsigned c, unsigned e)
{
    const unsigned x = c ^ (e * 0x01010101u);                              // 0 where equal, 1 .. 7 elsewhere
    return ((((x + 0x7f7f7f7fu) & 0x80808080u) ^ 0x80808080u) >> 7) * 0xffu;
}
