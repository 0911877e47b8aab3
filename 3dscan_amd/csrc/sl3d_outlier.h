// sl3d_outlier.h -- the rule of the radius outlier filter (sl3d_filter_outliers, include/sl3d_filter.h: a sample of the dense result is
// rejected when fewer than min_neighbours samples of its (2 * radius + 1)^2 window lie within max_dist of it): the in-range test, the
// support of one pixel over pitched planes, the rejection predicate.
//
// Shared by k_outlier_support / k_outlier_apply (sl3d_outlier.hip) and by the CPU check the test suite runs over crafted planes
// (tests/native/outlier_check.cpp): plain C, no HIP types.  The distance is the mesh stage's (sl3d_mesh.h), not a second spelling:
//
//   len2(p, q) = (dx*dx + dy*dy) + dz*dz with dx = (double)p.x - (double)q.x ..., IEEE double, no contraction      (mesh_len2)
//   thr2       = (double)max_dist * (double)max_dist                                                               (mesh_thr2)
//   in range   iff len2 <= thr2; a NaN len2 is not                                                                 (mesh_short)
//   sample     a window pixel whose valid byte is 1 -- the byte decides, not the point: a sample with a NaN coordinate has support 0
//   support(p) = the number of samples q != p with |dr| <= radius, |dc| <= radius, inside the window of W x H pixels, in range of p;
//                at most (2 * radius + 1)^2 - 1 <= 80
//   rejected   iff min_neighbours > 0 and support < min_neighbours
// len2(p, q) == len2(q, p) bit for bit (a difference and its negative have the same square), so the relation is symmetric.
#pragma once
#include <stdint.h>

#include "sl3d_mesh.h"

#define SL3D_OUTLIER_MAX_RADIUS 4    // SL3D_FILTER_MAX_RADIUS of include/sl3d_filter.h
#define SL3D_OUTLIER_NO_SAMPLE 0xFFu  // the support byte of a window pixel that is not a sample

// is sample q within range of sample p?  (false for a NaN length: a NaN or an infinite coordinate on either side)
SL3D_MESH_FN int outlier_in_range(const float *p, const float *q, double thr2) { return mesh_short(mesh_len2(p, q), thr2); }

// the largest min_neighbours a radius takes: the pixels of the neighbourhood
SL3D_MESH_FN int outlier_max_support(int radius) { return (2 * radius + 1) * (2 * radius + 1) - 1; }

// is a sample with this support rejected?
SL3D_MESH_FN int outlier_rejected(unsigned support, int min_neighbours) { return min_neighbours > 0 && support < (unsigned)min_neighbours; }

// The support byte of window pixel (r, c) of one view: valid [H][pitch] bytes, points [H][pitch][3] floats, the window W x H.  No byte
// and no float outside the window is read: the padding columns [W, pitch) are not pixels.
SL3D_MESH_FN unsigned outlier_support(const uint8_t *valid, const float *points, int W, int H, int pitch, int r, int c, int radius, double thr2)
{
    if (valid[(size_t)r * pitch + c] != 1) return SL3D_OUTLIER_NO_SAMPLE;
    const float *p = points + 3 * ((size_t)r * pitch + c);
    unsigned n = 0;
    for (int dr = -radius; dr <= radius; dr++)
        for (int dc = -radius; dc <= radius; dc++) {
            const int rr = r + dr, cc = c + dc;
            if ((dr == 0 && dc == 0) || rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
            const size_t i = (size_t)rr * pitch + cc;
            if (valid[i] == 1) n += (unsigned)outlier_in_range(p, points + 3 * i, thr2);
        }
    return n;
}
