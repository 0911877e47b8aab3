// sl3d_mesh_holes.h -- the arithmetic of the hole-filling stage (sl3d_mesh_fill_holes; the definition: include/sl3d.h): which pixels of a
// view form a small interior hole, and where a filled pixel lies.  Shared by the kernels of sl3d_mesh_holes.hip and by the CPU check the
// test suite runs over whole frames (tests/native/mesh_holes_check.cpp): plain C, no HIP types.
//
//   hole        a 4-connected component of non-candidate pixels of the window without a pixel of row 0 / H-1 or column 0 / W-1 and with
//               at most max_hole pixels
//   rim         of a hole pixel (r, c): the nearest candidates L, R of its row and U, D of its column, dl / dr / du / dd pixels away
//   usable      the row interpolant iff mesh_len2(L, R) <= t * t, t = (double)fill_edge * (double)(dl + dr) (a NaN len2 is not); the column
//               interpolant likewise with U, D and du + dd
//   position    h = (dr*L + dl*R) / (dl + dr), v = (dd*U + du*D) / (du + dd); both usable: ((du+dd)*h + (dl+dr)*v) / ((dl+dr) + (du+dd));
//               every operation one IEEE double operation in this order, nothing contracted, one cast to float at the end
//
// The labelling is the union-find of sl3d_mesh_components.h (labels only decrease, every write an atomic minimum, every loop bounded)
// over the NON-candidate pixels, with two additions that keep it off the background sheet:
//   - a pixel starts as the child of the first pixel of its row run inside its chunk (MESH_CHUNK columns of one row in the kernels), so
//     the unions inside a run are never made;
//   - a virtual root HOLE_OUTSIDE = -1, below every pixel index: a run gets it at once if it cannot belong to a hole (hole_run_outside),
//     and joining anything to it is one atomic minimum.  hole_find never indexes the label plane with it.
// Labels of candidate pixels are HOLE_NONE and are never visited.
#pragma once
#include <stdint.h>

#include "sl3d_mesh_components.h"

#define SL3D_HOLE_FN SL3D_CC_FN

#define HOLE_OUTSIDE (-1)
#define HOLE_NONE 0x7fffffff

// can the row run [s, e) of row r (columns of the window, inside one chunk) belong to no hole, by itself?
SL3D_HOLE_FN int hole_run_outside(int r, int s, int e, int W, int H, int max_hole) { return r == 0 || r == H - 1 || s == 0 || e == W || e - s > max_hole; }

// the root of x: a pixel index, or HOLE_OUTSIDE.  Path halving as cc_find
SL3D_HOLE_FN int hole_find(CC_LABEL_T *L, int x, int bound, int *failed)
{
    if (x == HOLE_OUTSIDE) return x;
    int p = CC_LOAD(L + x);
    while (p != x) {
        if (p == HOLE_OUTSIDE) return p;
        if (bound-- <= 0) {
            *failed = 1;
            return x;
        }
        const int g = CC_LOAD(L + p);
        if (g != p) CC_FETCH_MIN(L + x, g);
        x = p, p = g;
    }
    return x;
}

// cc_union over hole_find: the larger root is hung under the smaller; HOLE_OUTSIDE is the smallest of all and is never written to
SL3D_HOLE_FN void hole_union(CC_LABEL_T *L, int a, int b, int bound, int *failed)
{
    for (int tries = bound;;) {
        a = hole_find(L, a, bound, failed);
        b = hole_find(L, b, bound, failed);
        if (*failed || a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = CC_FETCH_MIN(L + a, b);
        if (old == a) return;
        if (tries-- <= 0) {
            *failed = 1;
            return;
        }
        a = old;
    }
}

// The unions of the non-candidate pixel p = r * pitch + c.  seam: c is the first column of a chunk (and not column 0); left / below /
// below_left: the pixels (r, c-1), (r+1, c), (r+1, c-1) exist in the window and are no candidates.  The run of p joins the run in front
// of the chunk seam, and the run below -- once per pair of runs of one chunk: where both pixels to the left continue the same two runs,
// the pixel to the left has made the union already
SL3D_HOLE_FN void hole_pixel_unions(CC_LABEL_T *L, int p, int pitch, int seam, int left, int below, int below_left, int bound, int *failed)
{
    if (seam && left) hole_union(L, p, p - 1, bound, failed);
    if (below && !(left && below_left && !seam)) hole_union(L, p, p + pitch, bound, failed);
}

// does the component of root `root` (hole_find's result, stored by the flatten pass) qualify as a hole?  size: pixels of the component
SL3D_HOLE_FN int hole_qualifies(int root, int size, int max_hole) { return root != HOLE_OUTSIDE && size <= max_hole; }

// The walks to the rim.  at: the pixel's candidate byte, stride: +-1 or +-pitch, n: the pixels the walk may visit -- min(the pixels the
// window has in that direction, the bound of a walk); a qualifying pixel finds a candidate among them.  The bytes are read in batches of
// HOLE_WALK_BATCH whose loads do not wait for one another: bit j of a batch = the pixel min(d0 + j, n) away is a candidate.  The clamp
// keeps every load inside the window and needs no branch; a clamped duplicate of pixel n sits above n's own bit, so the lowest set bit
// is always a real distance
#define HOLE_WALK_BATCH 8
SL3D_HOLE_FN unsigned hole_walk_batch(const uint8_t *at, long stride, int d0, int n)
{
    unsigned hit = 0u;
    SL3D_MESH_UNROLL
    for (int j = 0; j < HOLE_WALK_BATCH; j++) {
        const int d = d0 + j < n ? d0 + j : n;
        hit |= (unsigned)(at[(long)d * stride] & 1u) << j;
    }
    return hit;
}

// the distance to the nearest candidate at least d0 away; none within n: *failed is set
SL3D_HOLE_FN int hole_walk_from(const uint8_t *at, long stride, int d0, int n, int *failed)
{
    for (; d0 <= n; d0 += HOLE_WALK_BATCH) {
        const unsigned hit = hole_walk_batch(at, stride, d0, n);
        if (hit) return d0 + __builtin_ctz(hit);
    }
    *failed = 1;
    return 0;
}

SL3D_HOLE_FN int hole_usable(const float *a, const float *b, int span, float fill_edge)
{
    const double t = (double)fill_edge * (double)span;
    return mesh_short(mesh_len2(a, b), t * t);  // false for NaN
}

// (wb * a + wa * b) / (wa + wb) per component: a is wa pixels away, b is wb
SL3D_HOLE_FN void hole_interpolant(const float *a, int wa, const float *b, int wb, double out[3])
{
    SL3D_MESH_UNROLL
    for (int k = 0; k < 3; k++) out[k] = ((double)wb * (double)a[k] + (double)wa * (double)b[k]) / (double)(wa + wb);
}

#define HOLE_ROW 1  // the row interpolant is usable
#define HOLE_COL 2  // the column interpolant is usable
// the position of a hole pixel from its rim; returns HOLE_ROW | HOLE_COL bits, 0: the pixel stays empty (out is left alone)
SL3D_HOLE_FN int hole_position(const float *Lp, int dl, const float *Rp, int dr, const float *Up, int du, const float *Dp, int dd, float fill_edge,
                               float out[3])
{
    const int use = (hole_usable(Lp, Rp, dl + dr, fill_edge) ? HOLE_ROW : 0) | (hole_usable(Up, Dp, du + dd, fill_edge) ? HOLE_COL : 0);
    double h[3], v[3];
    hole_interpolant(Lp, dl, Rp, dr, h);
    hole_interpolant(Up, du, Dp, dd, v);
    SL3D_MESH_UNROLL
    for (int k = 0; k < 3; k++) {
        if (use == (HOLE_ROW | HOLE_COL))
            out[k] = (float)(((double)(du + dd) * h[k] + (double)(dl + dr) * v[k]) / (double)((dl + dr) + (du + dd)));
        else if (use == HOLE_ROW)
            out[k] = (float)h[k];
        else if (use == HOLE_COL)
            out[k] = (float)v[k];
    }
    return use;
}

// The fill of the qualifying pixel (r, c): walks over the candidate bytes `cand` (a W x H window, rows pitch apart) -- the first batch of
// all four directions at once, further batches only where a span is longer --, loads the four rim points from pts ([..][3]),
// hole_position.  bound: the steps a walk may take.  Points under non-candidates are never read
SL3D_HOLE_FN int hole_fill_pixel(const uint8_t *cand, const float *pts, int r, int c, int W, int H, int pitch, int bound, float fill_edge, float out[3],
                                 int *failed)
{
    const long p = (long)r * pitch + c;
    const uint8_t *at = cand + p;
    const int nl = c < bound ? c : bound, nr = W - 1 - c < bound ? W - 1 - c : bound, nu = r < bound ? r : bound, nd = H - 1 - r < bound ? H - 1 - r : bound;
    if (nl < 1 || nr < 1 || nu < 1 || nd < 1) {  // (a pixel on the border, or a bound of 0: no hole pixel)
        *failed = 1;
        return 0;
    }
    const unsigned hl = hole_walk_batch(at, -1, 1, nl), hr = hole_walk_batch(at, 1, 1, nr);
    const unsigned hu = hole_walk_batch(at, -(long)pitch, 1, nu), hd = hole_walk_batch(at, pitch, 1, nd);
    const int dl = hl ? 1 + __builtin_ctz(hl) : hole_walk_from(at, -1, 1 + HOLE_WALK_BATCH, nl, failed);
    const int dr = hr ? 1 + __builtin_ctz(hr) : hole_walk_from(at, 1, 1 + HOLE_WALK_BATCH, nr, failed);
    const int du = hu ? 1 + __builtin_ctz(hu) : hole_walk_from(at, -(long)pitch, 1 + HOLE_WALK_BATCH, nu, failed);
    const int dd = hd ? 1 + __builtin_ctz(hd) : hole_walk_from(at, pitch, 1 + HOLE_WALK_BATCH, nd, failed);
    if (*failed) return 0;
    const float *l = pts + 3 * (p - dl), *q = pts + 3 * (p + dr), *u = pts + 3 * (p - (long)du * pitch), *d = pts + 3 * (p + (long)dd * pitch);
    const float l3[3] = {l[0], l[1], l[2]}, q3[3] = {q[0], q[1], q[2]}, u3[3] = {u[0], u[1], u[2]}, d3[3] = {d[0], d[1], d[2]};
    return hole_position(l3, dl, q3, dr, u3, du, d3, dd, fill_edge, out);
}
