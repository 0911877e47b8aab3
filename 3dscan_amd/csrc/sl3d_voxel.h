// sl3d_voxel.h -- the arithmetic of the voxel grid (sl3d_voxel_grid, the rule: include/sl3d_voxel.h): the cell index of a coordinate and
// its range test, the key of a cell, the fixed-point offset of a point inside its cell, the centroid from the integer sums, the hash of a
// key and the capacity of the table.
//
// Shared by k_voxel_insert / k_voxel_count / k_voxel_scatter (sl3d_voxel.hip) and by the CPU check the test suite runs
// (tests/native/voxel_check.cpp): plain C, no HIP types, each piece spelled once.  Every operation is one IEEE double operation, no
// contraction (the library is built with -ffp-contract=off):
//
//   c        = floor((double)x / L), L = (double)leaf; in range iff -2^20 <= c < 2^20, tested on the double       (voxel_cell)
//   key      = ((cx + 2^20) << 42) | ((cy + 2^20) << 21) | (cz + 2^20): 63 bits, never VOXEL_EMPTY                (voxel_key)
//   q        = (int64)rint((((double)x - c * L) / L) * 2^24), ties to even; c * L is exact (21 x 24 bits)         (voxel_q)
//   centroid = (float)(c * L + (((double)S / (double)count) / 2^24) * L), S the int64 sum of q over the cell      (voxel_centroid)
//   hash     = the splitmix64 finaliser of the key                                                                (voxel_hash)
//   capacity = the smallest power of two >= max(1024, 2 * n); home slot = hash & (capacity - 1), linear probing   (voxel_table_capacity)
// x / L may round up to the next integer, so d = x - c * L lies in [-ulp, L] and q in [-1, 2^24]: a wave's 64 q's sum inside an int, a
// cloud's (fewer than 2^31 points) far inside an int64.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sl3d_mesh.h"  // SL3D_MESH_FN

#define VOXEL_EMPTY 0xFFFFFFFFFFFFFFFFull  // the key of an empty slot
#define VOXEL_NONE 0xFFFFFFFFu             // slot_of: the point is no run head; first: no point yet
#define VOXEL_INDEX_LIMIT 1048576.0        // 2^20
#define VOXEL_Q_ONE 16777216.0             // 2^24

// the floored cell index of a coordinate into *c; is it in range?  False for a NaN or an infinite x: the quotient is NaN or infinite then
SL3D_MESH_FN int voxel_cell(float x, double L, double *c)
{
    *c = floor((double)x / L);
    return *c >= -VOXEL_INDEX_LIMIT && *c < VOXEL_INDEX_LIMIT;
}

// the key of a cell whose three indices are in range
SL3D_MESH_FN uint64_t voxel_key(double cx, double cy, double cz)
{
    return (uint64_t)((int64_t)cx + 1048576) << 42 | (uint64_t)((int64_t)cy + 1048576) << 21 | (uint64_t)((int64_t)cz + 1048576);
}

// the fixed-point offset of coordinate x inside its cell c
SL3D_MESH_FN int64_t voxel_q(float x, double c, double L)
{
    const double base = c * L;
    const double d = (double)x - base;
    return (int64_t)rint((d / L) * VOXEL_Q_ONE);
}

// the centroid coordinate of a cell of index c, count points and sum S of their voxel_q
SL3D_MESH_FN float voxel_centroid(double c, double L, int64_t S, uint32_t count)
{
    const double base = c * L;
    return (float)(base + (((double)S / (double)count) / VOXEL_Q_ONE) * L);
}

SL3D_MESH_FN uint64_t voxel_hash(uint64_t k)
{
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

// slots of the table for a cloud of n points (0 <= n < 2^31): a load factor of at most 0.5
SL3D_MESH_FN uint64_t voxel_table_capacity(int64_t n)
{
    uint64_t cap = 1024;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    return cap;
}
