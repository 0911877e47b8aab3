// sl3d_mesh_lod.h -- the arithmetic of the level-of-detail stage (sl3d_mesh_views_lod; the definition: include/sl3d.h): which pixel of a
// step x step block represents it, which of the block's candidates go into its mean, and the ordered sum.  Shared by k_lod_blocks
// (sl3d_mesh_lod.hip) and by the CPU check the test suite runs over whole frames (tests/native/mesh_lod_check.cpp): plain C, no HIP types.
//
//   block (R, C)     rows [R*step, min(R*step + step, H)), columns [C*step, min(C*step + step, W)) of the window
//   representative   the candidate (r, c) of the block with the smallest d = (2(r - R*step) + 1 - step)^2 + (2(c - C*step) + 1 - step)^2,
//                    the first in row-major scan order among equals: the minimum of the packed key d << 8 | scan index (d <= 450, index <= 255)
//   members          the representative, and every other candidate q with mesh_len2(q, rep) <= (double)lod_edge * (double)lod_edge
//   position         the representative's bits; with the mean and k > 1 members, per component: s = +0, s += (double)q over the members in
//                    scan order, (float)(s / (double)k) -- every operation one IEEE double operation, nothing contracted
//
// Both users work on a TILE: `rows` fine rows (one coarse row) times tw = lod_tile_cols(step, width) * step fine columns, a multiple of 4,
// starting at window column col0 = tile * tw.  cand: [rows][tw] bytes, bit 0 = candidate (0 beyond the window), bit 1 = member, set by the
// second pass; pts: [rows][tw][3] (those under a byte of 0 never reach a result); and for the ids of a view whose candidates are its
// valid pixels, qpre: [rows][tw / 4], per row the exclusive prefix of the candidates over the tile's quads, front: [rows] the candidates
// of the row between the start of the chunk (MESH_CHUNK columns of one row, sl3d_mesh.h) col0 lies in and col0.
#pragma once
#include <stdint.h>

#include "sl3d_mesh.h"

#define SL3D_LOD_FN SL3D_MESH_FN
#ifdef __HIPCC__
#define SL3D_LOD_UNROLL4 _Pragma("unroll 4")
#else
#define SL3D_LOD_UNROLL4
#endif

#define LOD_MAX_STEP 16
#define LOD_TILE_W 256         // fine columns of a kernel tile at most: LOD_MAX_STEP rows of them are 48 KB of points
#define LOD_NONE 0xffffffffu   // the key of a block without a candidate

// coarse pixels along an axis of n fine ones
SL3D_LOD_FN int lod_coarse(int n, int step) { return (n + step - 1) / step; }

// coarse columns of a tile of at most `width` fine columns: a multiple of 4 (at least 4), so that every tile starts on a quad
SL3D_LOD_FN int lod_tile_cols(int step, int width)
{
    const int n = (width / step) & ~3;
    return n < 4 ? 4 : n;
}

// the packed key of pixel (dr, dc) of a block, both in [0, step)
SL3D_LOD_FN unsigned lod_key(int dr, int dc, int step)
{
    const int a = 2 * dr + 1 - step, b = 2 * dc + 1 - step;
    return (unsigned)(a * a + b * b) << 8 | (unsigned)(dr * step + dc);
}

// the tie rule: the scan index in the low bits decides between equal distances
SL3D_LOD_FN unsigned lod_key_min(unsigned x, unsigned y) { return y < x ? y : x; }

SL3D_LOD_FN int lod_member(const float *q, const float *rep, double thr2) { return mesh_short(mesh_len2(q, rep), thr2); }  // false for NaN

// The three passes over a staged tile.  None of their loops branches on what it loads, so the loads of an iteration do not wait for
// the result of the one before; only the ordered sum is a dependent chain, as the definition demands.
//
// 1. the smallest key of row dr of the block whose first column is tile column c0 (LOD_NONE: no candidate in that row).  The minimum is
//    associative: a block's key is the minimum over its rows in any order
SL3D_LOD_FN unsigned lod_row_key(const uint8_t *cand, int tw, int c0, int dr, int step)
{
    unsigned key = LOD_NONE;
    SL3D_LOD_UNROLL4
    for (int dc = 0; dc < step; dc++) key = lod_key_min(key, (cand[dr * tw + c0 + dc] & 1u) ? lod_key(dr, dc, step) : LOD_NONE);
    return key;
}

// the key of the representative of that block, or LOD_NONE
SL3D_LOD_FN unsigned lod_block_rep(const uint8_t *cand, int tw, int c0, int rows, int step)
{
    unsigned key = LOD_NONE;
    for (int dr = 0; dr < rows; dr++) key = lod_key_min(key, lod_row_key(cand, tw, c0, dr, step));
    return key;
}

// 2. the member bit of pixel (dr, dc) of that block, `key` its representative's: to be ORed into the pixel's byte.  Independent per pixel
#define LOD_MEMBER 2u
SL3D_LOD_FN unsigned lod_member_bit(const uint8_t *cand, const float *pts, int tw, int c0, int dr, int dc, int step, unsigned key, double thr2)
{
    if (!(cand[dr * tw + c0 + dc] & 1u) || key == LOD_NONE) return 0u;
    const int at = (int)(key & 255u), rr = at / step, rc = at - rr * step;
    if (dr == rr && dc == rc) return LOD_MEMBER;
    const float *q = pts + 3 * (dr * tw + c0 + dc), *rep = pts + 3 * (rr * tw + c0 + rc);
    const float q3[3] = {q[0], q[1], q[2]}, rep3[3] = {rep[0], rep[1], rep[2]};
    return lod_member(q3, rep3, thr2) ? LOD_MEMBER : 0u;
}

// 3. the position of that block (key != LOD_NONE); with the mean, from the member bits of pass 2.  The sum starts at +0 and a sum that
//    starts at +0 never becomes -0, so adding +0 for a pixel that is no member leaves every bit of it alone: the members are added in
//    scan order, one IEEE addition each, and the loop needs no branch.  Points under a byte without the bit are loaded and dropped
SL3D_LOD_FN void lod_block_position(const uint8_t *cand, const float *pts, int tw, int c0, int rows, int step, unsigned key, int mean, float out[3])
{
    const int at = (int)(key & 255u), rr = at / step, rc = at - rr * step;
    const float *rep = pts + 3 * (rr * tw + c0 + rc);
    out[0] = rep[0], out[1] = rep[1], out[2] = rep[2];
    if (!mean) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int k = 0;
    for (int dr = 0; dr < rows; dr++) {
        SL3D_LOD_UNROLL4
        for (int dc = 0; dc < step; dc++) {
            const int m = (int)(cand[dr * tw + c0 + dc] >> 1 & 1u);
            const float *q = pts + 3 * (dr * tw + c0 + dc);
            const float q0 = q[0], q1 = q[1], q2 = q[2];
            s0 += m ? (double)q0 : 0.0, s1 += m ? (double)q1 : 0.0, s2 += m ? (double)q2 : 0.0;
            k += m;
        }
    }
    if (k > 1) out[0] = (float)(s0 / (double)k), out[1] = (float)(s1 / (double)k), out[2] = (float)(s2 / (double)k);
}

// The candidates of a row in front of tile column c inside c's chunk: the id of a valid pixel in its view's compacted cloud is its chunk's
// offset plus this.  cand_row / qpre_row: the row's bytes / quad prefixes in the tile, front: the row's `front` word.  A tile is narrower
// than a chunk and both start on a quad: at most one chunk starts inside a tile.
SL3D_LOD_FN unsigned lod_rank_in_chunk(const uint8_t *cand_row, const unsigned *qpre_row, unsigned front, int col0, int c)
{
    const int start = ((col0 + c) & ~(MESH_CHUNK - 1)) - col0;  // the chunk's first column, as a tile column
    unsigned n = qpre_row[c >> 2];
    for (int j = c & ~3; j < c; j++) n += cand_row[j] & 1u;
    return start > 0 ? n - qpre_row[start >> 2] : front + n;
}
