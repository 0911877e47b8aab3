/* sl3d_voxel.h -- a voxel grid over a cloud on the device (libsl3d 0.23.0 and later): two calls on a context of include/sl3d.h.
 * Plain C, like sl3d.h, which it includes; the functions are exported by the same library. */
#ifndef SL3D_VOXEL_H
#define SL3D_VOXEL_H

#include "sl3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VOXEL GRID over an unorganised cloud: one point per occupied cell of a regular grid of edge `leaf`, the centroid of the points that fall
 * into the cell -- what PCL's VoxelGrid does behind a registration.  Where the views of a turntable scan overlap, the concatenation
 * sl3d_register_views / sl3d_register_clouds leave samples the surface two, three or more times; the grid removes the duplicate density,
 * averages the layers and, with a minimum count per cell, drops the stray points that survive in one view only.  The cells are found with a
 * hash table in device memory (k_voxel_insert), the output is compacted in cloud order (k_voxel_count, k_compact_scan, k_voxel_scatter);
 * nothing leaves the device unless the caller asks for it.
 *
 * THE RULE.
 * The input is a cloud of n points p_0 .. p_{n-1}, float xyz, in cloud order.  L = (double)leaf.  All arithmetic is IEEE double, no
 * contraction.
 *
 * 1. The cell index of a coordinate is c = floor((double)x / L).  A point is a sample iff its three coordinates are finite and all three c
 *    lie in [-2^20, 2^20), tested on the floored double, before any conversion to an integer.  Every other point is dropped: it is
 *    counted and otherwise ignored.
 * 2. The key of a sample is ((cx + 2^20) << 42) | ((cy + 2^20) << 21) | (cz + 2^20), 63 bits; 0xFFFFFFFFFFFFFFFF means "empty slot".
 * 3. A cell is the set of samples with one key.  Its count is its size, its first is the smallest point index in it.
 * 4. The position of a cell.  With SL3D_VOXEL_FIRST: the bits of p_first, unchanged.  With SL3D_VOXEL_CENTROID: a cell of count == 1
 *    gives the bits of its one point; otherwise, per coordinate,
 *      base = (double)c * L                              (exact: 21 x 24 bits)
 *      d = (double)x - base
 *      q = (int64)rint((d / L) * 16777216.0)             (ties to even)
 *      S = the sum of q over the cell in int64           (exact, so the order of the sum does not matter)
 *      centroid = (float)(base + (((double)S / (double)count) / 16777216.0) * L)
 * 5. Cells with count < min_points are left out.
 * 6. The remaining cells come out in ascending order of first, that is, in order of first appearance in the cloud, as three parallel
 *    arrays: xyz float[m][3]; first int32[m], an index into the input cloud -- a caller gathers colours, normals or the source view
 *    through it --; count uint32[m].
 * 7. counts[0] = points in, counts[1] = points dropped, counts[2] = occupied cells, counts[3] = cells kept (m).
 *
 * The result is a pure function of the input cloud, leaf, min_points and flags: it does not depend on the run, the device, or how the
 * table happened to fill.  Every atomic of the kernels is an integer atomic; there are no float atomics.
 *
 * The table, for whoever crafts collisions: voxel_hash(key) is the splitmix64 finaliser k ^= k >> 30; k *= 0xbf58476d1ce4e5b9;
 * k ^= k >> 27; k *= 0x94d049bb133111eb; k ^= k >> 31.  The capacity is the smallest power of two >= max(1024, 2 * n); the home slot is
 * hash & (capacity - 1), with linear probing.  The context owns the table, grows it on demand and keeps it for the next call;
 * sl3d_destroy frees it.
 *
 * INPUT.  xyz_in == NULL takes the registered cloud the last sl3d_register_views / sl3d_register_clouds left on the device (n_in is
 * not used; SL3D_E_STATE if neither has run on this context).  Otherwise xyz_in is a host cloud of n_in points, uploaded to a scratch
 * buffer of the context; the caller's memory has been read when the call returns.  n = 0 is a valid call with an empty result.
 *
 * OUTPUT.  device_out (or NULL) receives the device addresses of the three arrays; they stay valid until the next grid call or
 * sl3d_destroy.  counts == NULL leaves the call asynchronous.  Otherwise the four counts are downloaded and the call returns with the
 * stream idle.  The call does not touch any view's planes, clouds or meshes, nor the registered cloud.
 *
 * Refusals are made before anything is allocated or enqueued, and a refused call changes nothing, the last result included.
 * SL3D_E_INVALID_ARG: leaf NaN, infinite or <= 0; min_points < 1; unknown flag bits; n_in < 0 or >= 2^31.
 *
 * There is no group entry point and no shim call. */
#define SL3D_VOXEL_FIRST    0u
#define SL3D_VOXEL_CENTROID 1u
typedef struct { const float *xyz; const int32_t *first; const uint32_t *count; } sl3d_voxels;   /* device pointers */

int sl3d_voxel_grid(sl3d_ctx *ctx, const float *xyz_in, int64_t n_in, float leaf, int64_t min_points, unsigned flags,
                    sl3d_voxels *device_out /* or NULL */, int64_t counts[4] /* or NULL: stays asynchronous */);

/* The result of the last sl3d_voxel_grid, by the size-then-fill protocol of the other getters: at most `capacity` rows are written to
 * each output that is not NULL, *n (not NULL) always receives the total m.
 * SL3D_E_INVALID_ARG: null n, capacity < 0; SL3D_E_STATE: no grid call has run on this context.  Synchronises. */
int sl3d_get_voxel_grid(sl3d_ctx *ctx, float *xyz, int32_t *first, uint32_t *count, int64_t capacity, int64_t *n);

#ifdef __cplusplus
}
#endif

#endif /* SL3D_VOXEL_H */
