// sl3d_capi_voxel.cpp -- the voxel grid over an unorganised cloud (the rule: include/sl3d_voxel.h; the kernels: sl3d_voxel.hip, their
// arithmetic: sl3d_voxel.h): sl3d_voxel_grid reduces the registered cloud of the context, or a host cloud, to one point per occupied
// cell and leaves xyz / first / count on the device; sl3d_get_voxel_grid hands them out.
#include "sl3d_capi_internal.h"
#include "../../include/sl3d_voxel.h"
#include "sl3d_voxel.h"

// the arrays of the context that grow with the cloud, in the order of sl3d_ctx::vox_cap
enum { VOX_IN, VOX_TABLE, VOX_SLOT, VOX_CNT, VOX_OFF, VOX_XYZ, VOX_FIRST, VOX_COUNT };

// Everything a grid over n points (> 0) with a table of `capacity` slots needs: what is there and large enough is kept.  The table is one
// allocation -- key, first, count, sums (launch_voxel_grid) -- sized for the centroid form from the start, so a context never holds two
static int ensure_voxel_buffers(sl3d_ctx *x, int64_t n, uint64_t capacity, bool upload)
{
    const size_t nb = (size_t)((n + 1023) / 1024);
    size_t *cap = x->vox_cap;
    int rc = SL3D_OK;
    if (upload) rc = grow_plane(x, &x->d_vox_in, &cap[VOX_IN], 3 * (size_t)n);
    if (!rc) rc = grow_plane(x, &x->d_vox_table, &cap[VOX_TABLE], (size_t)capacity * 40);
    if (!rc) rc = grow_plane(x, &x->d_vox_slot, &cap[VOX_SLOT], nb * 1024);
    if (!rc) rc = grow_plane(x, &x->vox_s.cnt, &cap[VOX_CNT], nb);
    if (!rc) rc = grow_plane(x, &x->vox_s.off, &cap[VOX_OFF], nb);
    if (!rc) rc = grow_plane(x, &x->d_vox_xyz, &cap[VOX_XYZ], 3 * (size_t)n);
    if (!rc) rc = grow_plane(x, &x->d_vox_first, &cap[VOX_FIRST], (size_t)n);
    if (!rc) rc = grow_plane(x, &x->d_vox_count, &cap[VOX_COUNT], (size_t)n);
    if (!rc) rc = ensure_plane(x, &x->d_vox_words, (size_t)VOXEL_WORDS);
    return rc;
}

// the call's words, once the stream has drained: a probe that ran through the table is the library's internal error
static int voxel_words(sl3d_ctx *x, unsigned long long w[VOXEL_WORDS])
{
    HIPCHK(x, hipMemcpyAsync(w, x->d_vox_words, VOXEL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    SYNC_FOR_CALLER(x);
    if (w[VOXEL_WORD_ERROR]) return fail(x, SL3D_E_INTERNAL, "voxel_grid: a probe ran through the whole table");
    return SL3D_OK;
}

// Memsets of the table and the words, k_voxel_insert, k_voxel_count, k_compact_scan, k_voxel_scatter on the context's stream behind the
// launch lanes (ON_DEVICE).  Every refusal comes before the first allocation.
extern "C" int sl3d_voxel_grid(sl3d_ctx *x, const float *xyz_in, int64_t n_in, float leaf, int64_t min_points, unsigned flags, sl3d_voxels *device_out,
                               int64_t counts[4])
try {
    if (!x) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: null context");
    if (!(leaf > 0.0f) || std::isinf(leaf)) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: leaf must be finite and > 0");
    if (min_points < 1) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: min_points must be >= 1");
    if (flags & ~SL3D_VOXEL_CENTROID) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: unknown flag bits");
    if (n_in < 0 || n_in >= (int64_t)1 << 31) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: n_in must be 0 .. 2^31 - 1");
    if (!xyz_in && x->reg_total < 0) return fail(x, SL3D_E_STATE, "voxel_grid: no sl3d_register_views / sl3d_register_clouds has left a cloud");
    const int64_t n = xyz_in ? n_in : x->reg_total;
    if (n >= (int64_t)1 << 31) return fail(x, SL3D_E_INVALID_ARG, "voxel_grid: the registered cloud has 2^31 points or more");
    const bool centroid = (flags & SL3D_VOXEL_CENTROID) != 0;
    ON_DEVICE(x);
    x->vox_n = -1;  // (from here on the last result is gone)
    if (n > 0) {
        const uint64_t capacity = voxel_table_capacity(n);
        int rc = ensure_voxel_buffers(x, n, capacity, xyz_in != nullptr);
        if (rc) return rc;
        if (xyz_in) {  // the caller's memory may be pageable: the upload is complete when the call returns
            HIPCHK(x, hipMemcpyAsync(x->d_vox_in, xyz_in, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, x->stream));
            HIPCHK(x, hipStreamSynchronize(x->stream));
        }
        uint8_t *t = x->d_vox_table;
        const VoxelTable T{(unsigned long long *)t, (unsigned *)(t + 8 * capacity), (unsigned *)(t + 12 * capacity),
                           centroid ? (long long *)(t + 16 * capacity) : nullptr, capacity};
        rc = launched(x, launch_voxel_grid(xyz_in ? x->d_vox_in : x->d_reg, n, leaf, min_points, centroid, T, x->d_vox_slot, x->vox_s, x->d_vox_words,
                                           VoxelOut{x->d_vox_xyz, x->d_vox_first, x->d_vox_count}, x->stream));
        if (rc) return rc;
    }
    x->vox_n = n;
    if (device_out) *device_out = sl3d_voxels{n ? x->d_vox_xyz : nullptr, n ? x->d_vox_first : nullptr, n ? x->d_vox_count : nullptr};
    if (!counts) return SL3D_OK;
    unsigned long long w[VOXEL_WORDS] = {0};
    if (n > 0) {
        const int rc = voxel_words(x, w);
        if (rc) return rc;
    } else
        SYNC_FOR_CALLER(x);
    counts[0] = n, counts[1] = (int64_t)w[VOXEL_WORD_DROPPED], counts[2] = (int64_t)w[VOXEL_WORD_OCCUPIED], counts[3] = (int64_t)w[VOXEL_WORD_KEPT];
    return SL3D_OK;
}
SL3D_CATCH(x)

// the result the last sl3d_voxel_grid left: size then fill
extern "C" int sl3d_get_voxel_grid(sl3d_ctx *x, float *xyz, int32_t *first, uint32_t *count, int64_t capacity, int64_t *n)
try {
    if (!x || !n || capacity < 0) return fail(x, SL3D_E_INVALID_ARG, "get_voxel_grid: null argument or capacity < 0");
    if (x->vox_n < 0) return fail(x, SL3D_E_STATE, "get_voxel_grid: no sl3d_voxel_grid has run on this context");
    ON_DEVICE(x);
    unsigned long long w[VOXEL_WORDS] = {0};
    if (x->vox_n > 0) {
        const int rc = voxel_words(x, w);
        if (rc) return rc;
    }
    const int64_t total = (int64_t)w[VOXEL_WORD_KEPT], m = total < capacity ? total : capacity;
    if (m > 0) {
        if (xyz) HIPCHK_DRAIN(x, hipMemcpyAsync(xyz, x->d_vox_xyz, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        if (first) HIPCHK_DRAIN(x, hipMemcpyAsync(first, x->d_vox_first, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
        if (count) HIPCHK_DRAIN(x, hipMemcpyAsync(count, x->d_vox_count, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    }
    SYNC_FOR_CALLER(x);
    *n = total;
    return SL3D_OK;
}
SL3D_CATCH(x)
