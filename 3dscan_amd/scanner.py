"""ctypes binding of the C ABI (include/sl3d.h) -- the Python face of the product library.

There is no fallback: if libsl3d.so is missing or no HIP device is present, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SL3D_LIB: another build of the SAME library (kernel A/B experiments, tools/ab.sh); never a fallback
LIB_PATH = os.environ.get("SL3D_LIB") or os.path.join(_HERE, "libsl3d.so")

SL3D_FLAG_KEEP_STAGES = 1
SL3D_FLAG_GROUP_FORCE_RCCL, SL3D_FLAG_GROUP_NO_RCCL, SL3D_FLAG_GROUP_DISTINCT_SIDES = 2, 4, 16
SL3D_FLAG_EAGER_MASK = 32
SL3D_FLAG_SERIAL_LAUNCHES = 64
SL3D_FLAG_SUBPIXEL = 128
SL3D_FLAG_REPAIR_PERIODS = 256
SL3D_FLAG_ANCHOR_PERIODS = 512
SL3D_FLAG_ONLY_VERTICAL, SL3D_FLAG_ONLY_HORIZONTAL = 1024, 2048
SL3D_FLAG_DIRECT_GRAY = 4096
AXIS_VERTICAL, AXIS_HORIZONTAL = 0, 1
PATTERN_FRINGE, PATTERN_GRAY, PATTERN_INVERSE_GRAY, PATTERN_BINARY = 0, 1, 2, 3
VALID_VERTICAL, VALID_HORIZONTAL, VALID_MERGED = 0, 1, 2
SL3D_SMOOTH_FIX_BOUNDARY, SL3D_SMOOTH_NORMALS = 1, 2
SL3D_LOD_MEAN, SL3D_LOD_NORMALS = 1, 2
SL3D_FILL_NORMALS = 1

class Sl3dError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "full_width", "full_height", "col0", "row0", "proj_width", "proj_height",
        "n_fringe", "n_gray_v", "n_gray_h", "fringe_width_v", "fringe_width_h", "n_codes_v", "n_codes_h",
        "max_views", "device")] + [("flags", C.c_uint32), ("stream", C.c_void_p)]


class DeviceBuffers(C.Structure):
    _fields_ = [
        ("frames", C.c_void_p), ("frame_pitch", C.c_size_t), ("plane_stride", C.c_size_t), ("view_stride", C.c_size_t),
        ("planes_per_view", C.c_int32),
        ("mask", C.c_void_p), ("mask_pitch", C.c_size_t), ("mask_view_stride", C.c_size_t),
        ("points", C.c_void_p), ("points_pitch", C.c_size_t), ("points_view_stride", C.c_size_t),
        ("valid", C.c_void_p), ("valid_pitch", C.c_size_t), ("valid_view_stride", C.c_size_t),
    ]


class CloudSegments(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("counts", C.c_void_p), ("offsets", C.c_void_p), ("n_segments", C.c_int32), ("segment_points", C.c_int32),
                ("view_stride_points", C.c_size_t), ("view_stride_segments", C.c_size_t)]


class Mesh(C.Structure):
    """sl3d_mesh: device addresses of the clouds and faces sl3d_mesh_views left in HBM"""
    _fields_ = [("xyz", C.c_void_p), ("faces", C.c_void_p), ("view_stride_points", C.c_size_t), ("view_stride_faces", C.c_size_t)]


class MeshFiltered(C.Structure):
    """sl3d_mesh_filtered: device addresses of the clouds, faces and original vertex ids sl3d_mesh_views_filtered left in HBM"""
    _fields_ = [("xyz", C.c_void_p), ("faces", C.c_void_p), ("vertex_ids", C.c_void_p), ("view_stride_points", C.c_size_t),
                ("view_stride_faces", C.c_size_t)]


class MeshSmoothed(C.Structure):
    """sl3d_mesh_smoothed: device addresses of the smoothed vertices and (with SL3D_SMOOTH_NORMALS, else None) their normals"""
    _fields_ = [("xyz", C.c_void_p), ("normals", C.c_void_p), ("view_stride_points", C.c_size_t)]


class MeshLod(C.Structure):
    """sl3d_mesh_lod: device addresses of the vertices, faces, original vertex ids and (with SL3D_LOD_NORMALS, else None) normals
    sl3d_mesh_views_lod left in HBM, and the size of the coarse grid"""
    _fields_ = [("xyz", C.c_void_p), ("faces", C.c_void_p), ("vertex_ids", C.c_void_p), ("normals", C.c_void_p),
                ("view_stride_points", C.c_size_t), ("view_stride_faces", C.c_size_t), ("grid_width", C.c_int32), ("grid_height", C.c_int32)]


class Voxels(C.Structure):
    """sl3d_voxels: device addresses of the xyz, first and count arrays sl3d_voxel_grid left in HBM"""
    _fields_ = [("xyz", C.c_void_p), ("first", C.c_void_p), ("count", C.c_void_p)]


class TsdfVolume(C.Structure):
    """sl3d_tsdf_volume: the origin, the voxel edge, the truncation distance and the dims (nx, ny, nz) of a TSDF volume"""
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("trunc", C.c_float), ("dims", C.c_int32 * 3)]


class TsdfSurface(C.Structure):
    """sl3d_tsdf_surface: device addresses of the xyz, normals and edge arrays sl3d_tsdf_extract left in HBM"""
    _fields_ = [("xyz", C.c_void_p), ("normals", C.c_void_p), ("edge", C.c_void_p)]


class Turntable(C.Structure):
    """sl3d_turntable: what sl3d_refine_turntable leaves"""
    _fields_ = [("tx", C.c_float), ("ty", C.c_float), ("tz", C.c_float), ("rot_step", C.c_float), ("est", C.c_double * 4), ("n", C.c_int64),
                ("sources", C.c_int64), ("rms_xz", C.c_double), ("rms_y", C.c_double), ("degenerate", C.c_int32), ("reserved", C.c_int32)]


class AlignIteration(C.Structure):
    """sl3d_align_iteration: one entry of sl3d_refine_turntable's log"""
    _fields_ = [("est", C.c_double * 4), ("n", C.c_int64), ("sources", C.c_int64), ("rms_xz", C.c_double), ("rms_y", C.c_double)]


class MeshHoles(C.Structure):
    """sl3d_mesh_holes: device addresses of the vertices, faces, original vertex ids (-1: filled) and (with SL3D_FILL_NORMALS, else
    None) normals sl3d_mesh_fill_holes left in HBM"""
    _fields_ = [("xyz", C.c_void_p), ("faces", C.c_void_p), ("vertex_ids", C.c_void_p), ("normals", C.c_void_p),
                ("view_stride_points", C.c_size_t), ("view_stride_faces", C.c_size_t)]


_vp, _i, _u, _f, _d, _sz, _i64 = C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_double, C.c_size_t, C.c_int64
_pvp, _pi, _pu, _pf, _psz, _p64 = (C.POINTER(t) for t in (_vp, _i, _u, _f, _sz, _i64))

# The C ABI as ctypes sees it, stated by hand and independently of include/sl3d.h (tests/test_binding.py holds one against the other):
# a row per exported function in the header's order -- (name, argtypes) or, where the function does not return an int status,
# (name, argtypes, restype).  A new function gets its row here and nothing else; load_library applies the table.
_PROTOTYPES = (
    ("sl3d_version", [], C.c_char_p),
    ("sl3d_strerror", [_i], C.c_char_p),
    ("sl3d_last_error", [_vp], C.c_char_p),
    ("sl3d_create", [C.POINTER(Config), _pvp]),
    ("sl3d_destroy", [_vp], None),
    ("sl3d_set_calibration", [_vp] + [_vp] * 8),
    ("sl3d_get_projection_matrices", [_vp, _vp, _vp]),
    ("sl3d_set_mask", [_vp, _i, _vp, _sz]),
    ("sl3d_set_masks", [_vp, _i, _i, _vp, _sz, _sz]),
    ("sl3d_set_masks_modulated", [_vp, _i, _i, _d, _vp, _sz, _sz]),
    ("sl3d_get_modulation", [_vp, _i, _i, _vp, _sz]),
    ("sl3d_set_mask_colrow", [_vp, _i, _vp]),
    ("sl3d_set_frames_range", [_vp, _i, _i, _i, _vp, _i, _sz]),
    ("sl3d_get_global_colrow", [_vp, _i, _i, _vp, _i, _i]),
    ("sl3d_set_frames", [_vp, _i, _i, _vp, _i, _sz]),
    ("sl3d_copy_view", [_vp, _i, _i]),
    ("sl3d_synth_view", [_vp, _i, _vp, C.c_uint64, _i, _i, _f, _f]),
    ("sl3d_get_frames", [_vp, _i, _i, _vp, _i, _sz]),
    ("sl3d_compute_wrapped_phase", [_vp, _i, _i]),
    ("sl3d_unwrap_phase", [_vp, _i, _i]),
    ("sl3d_compute_c_p_map", [_vp, _i]),
    ("sl3d_triangulate", [_vp, _i]),
    ("sl3d_repair_periods", [_vp, _i, _i, _i, _pu]),
    ("sl3d_triangulate_subpixel", [_vp, _i, _i, _d, _pu]),
    ("sl3d_get_residuals", [_vp, _i, _vp, _sz]),
    ("sl3d_get_correspondences_subpixel", [_vp, _i, _vp, _sz]),
    ("sl3d_run", [_vp, _i, _i]),
    ("sl3d_run_clouds", [_vp, _i, _i]),
    ("sl3d_get_cloud_counts", [_vp, _i, _i, _pvp, _psz, _p64]),
    ("sl3d_get_cloud_segments", [_vp, _i, _i, C.POINTER(CloudSegments), _p64]),
    ("sl3d_download_clouds", [_vp, _i, _i, _vp, _i64, _p64]),
    ("sl3d_register_clouds", [_vp, _i, _i, _f, _f, _f, _f, _vp, _i64, _p64]),
    ("sl3d_fused_kernel_name", [_vp, _i, _i, C.c_char_p, _sz]),
    ("sl3d_last_fused_kernel_name", [_vp, C.c_char_p, _sz]),
    ("sl3d_launch_counts", [_vp, _p64, _p64]),
    ("sl3d_camera_table_bytes_per_pixel", [_vp, _i]),
    ("sl3d_run_timed", [_vp, _i, _i, _pf]),
    ("sl3d_synchronize", [_vp]),
    ("sl3d_timer_start", [_vp]),
    ("sl3d_timer_stop", [_vp, _pf]),
    ("sl3d_get_valid_map", [_vp, _i, _i, _vp, _sz]),
    ("sl3d_get_wrapped_phase", [_vp, _i, _i, _vp, _sz]),
    ("sl3d_get_unwrapped_phase", [_vp, _i, _i, _vp, _sz]),
    ("sl3d_get_code", [_vp, _i, _i, _vp, _sz]),
    ("sl3d_get_debug_image", [_vp, _i, _i, _i, _vp, _sz]),
    ("sl3d_get_c_p_map", [_vp, _i, _vp]),
    ("sl3d_get_intersection_points", [_vp, _i, _vp]),
    ("sl3d_get_points", [_vp, _i, _vp, _vp]),
    ("sl3d_get_cloud", [_vp, _i, _vp, _i64, _p64]),
    ("sl3d_set_texture", [_vp, _i, _vp, _sz]),
    ("sl3d_get_cloud_rgb", [_vp, _i, _vp, _vp, _i64, _p64]),
    ("sl3d_compact", [_vp, _i, _pvp, _p64]),
    ("sl3d_compact_views", [_vp, _i, _i, _pvp, _psz, _p64]),
    ("sl3d_get_clouds", [_vp, _i, _i, _vp, _i64, _p64]),
    ("sl3d_mesh_views", [_vp, _i, _i, _f, C.POINTER(Mesh), _p64, _p64]),
    ("sl3d_get_meshes", [_vp, _i, _i, _f, _vp, _i64, _vp, _i64, _p64, _p64]),
    ("sl3d_mesh_normals", [_vp, _i, _i, _f, _pvp, _psz, _p64]),
    ("sl3d_get_mesh_normals", [_vp, _i, _i, _f, _vp, _i64, _p64]),
    ("sl3d_mesh_components", [_vp, _i, _i, _f, _pvp, _psz, _p64, _p64]),
    ("sl3d_get_mesh_components", [_vp, _i, _i, _f, _vp, _i64, _p64, _p64]),
    ("sl3d_mesh_views_filtered", [_vp, _i, _i, _f, _i64, C.POINTER(MeshFiltered), _p64, _p64]),
    ("sl3d_get_meshes_filtered", [_vp, _i, _i, _f, _i64, _vp, _vp, _i64, _vp, _i64, _p64, _p64]),
    ("sl3d_mesh_smooth", [_vp, _i, _i, _f, _i, _f, _f, _u, C.POINTER(MeshSmoothed), _p64]),
    ("sl3d_get_mesh_smoothed", [_vp, _i, _i, _f, _i, _f, _f, _u, _vp, _vp, _i64, _p64]),
    ("sl3d_mesh_views_lod", [_vp, _i, _i, _i, _f, _i64, _f, _u, C.POINTER(MeshLod), _p64, _p64]),
    ("sl3d_get_meshes_lod", [_vp, _i, _i, _i, _f, _i64, _f, _u, _vp, _vp, _vp, _i64, _vp, _i64, _p64, _p64]),
    ("sl3d_mesh_fill_holes", [_vp, _i, _i, _f, _i64, _i64, _f, _u, C.POINTER(MeshHoles), _p64, _p64, _p64, _p64]),
    ("sl3d_get_meshes_holes_filled", [_vp, _i, _i, _f, _i64, _i64, _f, _u, _vp, _vp, _vp, _i64, _vp, _i64, _p64, _p64, _p64, _p64]),
    ("sl3d_register_views", [_vp, _i, _i, _f, _f, _f, _f, _vp, _i64, _p64]),
    ("sl3d_transform_cloud", [_vp, _vp, _i64, _f, _f, _f, _f, _vp]),
    ("sl3d_host_alloc", [_sz], _vp),
    ("sl3d_host_free", [_vp], None),
    ("sl3d_process_views", [_vp, _i, _vp, _sz, _vp, _vp]),
    ("sl3d_undistort", [_vp, _vp, _sz, _i, _i, _i, _vp, _vp, _vp, _sz]),
    ("sl3d_set_frames_raw", [_vp, _i, _i, _vp, _i, _sz]),
    ("sl3d_pattern_counts", [_i, _i, _pi, _pi]),
    ("sl3d_generate_pattern", [_vp, _i, _i, _i, _vp, _sz, _pvp, _psz]),
    ("sl3d_get_device_buffers", [_vp, C.POINTER(DeviceBuffers)]),
    ("sl3d_download", [_vp, _vp, _vp, _sz]),
    ("sl3d_download_2d", [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    ("sl3d_group_create", [C.POINTER(Config), _pi, _i, _pvp]),
    ("sl3d_group_destroy", [_vp], None),
    ("sl3d_group_last_error", [_vp], C.c_char_p),
    ("sl3d_group_size", [_vp]),
    ("sl3d_group_stripe", [_vp, _i, _pi, _pi, _pi, _pvp]),
    ("sl3d_group_transport", [_vp], C.c_char_p),
    ("sl3d_group_set_calibration", [_vp] + [_vp] * 8),
    ("sl3d_group_set_mask", [_vp, _i, _vp, _sz]),
    ("sl3d_group_set_frames", [_vp, _i, _i, _vp, _i, _sz]),
    ("sl3d_group_run", [_vp, _i, _i]),
    ("sl3d_group_gather", [_vp, _i, _i]),
    ("sl3d_group_get_points", [_vp, _i, _vp, _vp]),
    ("sl3d_group_download_points", [_vp, _i, _i, _vp, _vp]),
    ("sl3d_group_process_views", [_vp, _i, _vp, _sz, _vp, _vp]),
    ("sl3d_group_get_device_buffers", [_vp, C.POINTER(DeviceBuffers)]),
    ("sl3d_group_run_clouds", [_vp, _i, _i]),
    ("sl3d_group_gather_clouds", [_vp, _i, _i, _p64]),
    ("sl3d_group_get_cloud", [_vp, _i, _vp, _i64, _p64]),
    ("sl3d_group_synchronize", [_vp]),
)
# every symbol include/sl3d.h declares (tests check the library exports all of them)
ABI_SYMBOLS = tuple(row[0] for row in _PROTOTYPES)
# the same for include/sl3d_fuse.h, the header of the exposure fusion (tests/test_exposure_flag.py holds one against the other)
_FUSE_PROTOTYPES = (
    ("sl3d_fuse_exposures", [_vp, _i, _i, _i, _i, _pu]),
    ("sl3d_get_exposure_map", [_vp, _i, _vp, _sz]),
)
FUSE_SYMBOLS = tuple(row[0] for row in _FUSE_PROTOTYPES)
# ... and for include/sl3d_filter.h, the header of the outlier filter (tests/test_outlier_flag.py)
_FILTER_PROTOTYPES = (
    ("sl3d_filter_outliers", [_vp, _i, _i, _i, _f, _i, _pu]),
    ("sl3d_get_support", [_vp, _i, _vp, _sz]),
)
FILTER_SYMBOLS = tuple(row[0] for row in _FILTER_PROTOTYPES)
# ... and for include/sl3d_voxel.h, the header of the voxel grid (tests/test_voxel_flag.py)
_VOXEL_PROTOTYPES = (
    ("sl3d_voxel_grid", [_vp, _vp, _i64, _f, _i64, _u, C.POINTER(Voxels), _p64]),
    ("sl3d_get_voxel_grid", [_vp, _vp, _vp, _vp, _i64, _p64]),
)
VOXEL_SYMBOLS = tuple(row[0] for row in _VOXEL_PROTOTYPES)
VOXEL_FIRST, VOXEL_CENTROID = 0, 1   # SL3D_VOXEL_FIRST, SL3D_VOXEL_CENTROID

# ... and for include/sl3d_align.h, the header of the turntable refinement (tests/test_align_flag.py)
_ALIGN_PROTOTYPES = (
    ("sl3d_align_sums", [_vp, _i, _i, _vp, _d, _d, _f, _f, _i, _vp]),
    ("sl3d_align_solve", [_vp, _i, _f, _d, _d, _vp, _vp, _vp]),
    ("sl3d_refine_turntable", [_vp, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i, C.POINTER(Turntable), C.POINTER(AlignIteration), _pi]),
    ("sl3d_get_align_camera", [_vp, _vp]),
)
ALIGN_SYMBOLS = tuple(row[0] for row in _ALIGN_PROTOTYPES)
ALIGN_WORDS = 12                     # SL3D_ALIGN_WORDS

# ... and for include/sl3d_align_plane.h, the header of its point-to-plane form (tests/test_align_plane_flag.py)
_ALIGN_PLANE_PROTOTYPES = (
    ("sl3d_align_normals", [_vp, _i, _i, _f]),
    ("sl3d_get_align_normals", [_vp, _i, _vp, _sz]),
    ("sl3d_align_plane_sums", [_vp, _i, _i, _vp, _d, _d, _f, _f, _f, _i, _vp]),
    ("sl3d_align_plane_solve", [_vp, _i, _f, _d, _d, _vp, _vp, _vp]),
    ("sl3d_refine_turntable_plane", [_vp, _i, _i, _f, _f, _f, _f, _f, _f, _f, _i, _i, C.POINTER(Turntable), C.POINTER(AlignIteration), _pi]),
)
ALIGN_PLANE_SYMBOLS = tuple(row[0] for row in _ALIGN_PLANE_PROTOTYPES)
ALIGN_PLANE_WORDS = 18               # SL3D_ALIGN_PLANE_WORDS

# ... and for include/sl3d_tsdf.h, the header of the TSDF volume (tests/test_tsdf_flag.py)
_TSDF_PROTOTYPES = (
    ("sl3d_tsdf_reset", [_vp, C.POINTER(TsdfVolume)]),
    ("sl3d_tsdf_integrate", [_vp, _i, _i, _i, _vp, _p64]),
    ("sl3d_tsdf_extract", [_vp, _i64, C.POINTER(TsdfSurface), _p64]),
    ("sl3d_get_tsdf", [_vp, _vp, _vp, _i64, _p64]),
    ("sl3d_get_tsdf_surface", [_vp, _vp, _vp, _vp, _i64, _p64]),
)
TSDF_SYMBOLS = tuple(row[0] for row in _TSDF_PROTOTYPES)

_lib = None


def load_library(path=None):
    """dlopen the product library; raises if it has not been built (no CPU fallback exists).

    Missing symbols have one rule: with SL3D_LIB set (another build of the library, A/B runs with tools/ab.sh) a function the loaded
    build lacks is skipped, whatever release it came with, and a later call to it fails with AttributeError; without SL3D_LIB any
    missing function raises here."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise Sl3dError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C 3dscan_amd/csrc` (there is no CPU fallback)")
    L = C.CDLL(p)
    for name, argtypes, *restype in _PROTOTYPES + _FUSE_PROTOTYPES + _FILTER_PROTOTYPES + _VOXEL_PROTOTYPES + _ALIGN_PROTOTYPES + _ALIGN_PLANE_PROTOTYPES + _TSDF_PROTOTYPES:
        try:
            fn = getattr(L, name)
        except AttributeError:
            if not os.environ.get("SL3D_LIB"):
                raise
            continue
        fn.argtypes, fn.restype = argtypes, restype[0] if restype else C.c_int
    if path is None:
        _lib = L
    return L


def pattern_counts(proj_extent, fringe_width):
    """(number of codes, number of bit planes) of 1/pattern_generator.cpp:224-229."""
    L = load_library()
    nc, npl = C.c_int(), C.c_int()
    rc = L.sl3d_pattern_counts(proj_extent, fringe_width, C.byref(nc), C.byref(npl))
    if rc != 0:
        raise Sl3dError("sl3d_pattern_counts: " + L.sl3d_strerror(rc).decode())
    return nc.value, npl.value


def _host_solve(symbol, words, sums, range, ox, oz, est):
    """a host-only solve (`symbol`) over the (n_pairs, words) int64 words of a pass"""
    L = load_library()
    w = np.ascontiguousarray(sums, dtype=np.int64).reshape(-1, words)
    e, out, stats = np.ascontiguousarray(est, dtype=np.float64).reshape(4), np.empty(4), np.empty(4)
    rc = getattr(L, symbol)(w.ctypes.data, len(w), range, ox, oz, e.ctypes.data, out.ctypes.data, stats.ctypes.data)
    if rc != 0:
        raise Sl3dError(symbol + ": " + L.sl3d_strerror(rc).decode())
    return out, dict(n=int(stats[0]), rms_xz=float(stats[1]), rms_y=float(stats[2]), degenerate=bool(stats[3]))


def align_solve(sums, range, ox, oz, est):
    """sl3d_align_solve: the closed-form solve over the (n_pairs, 12) int64 words of a pass (the rule: include/sl3d_align.h); host only, no
    context.  est: (c, s, tx, tz).  Returns (the new estimate float64[4], dict(n, rms_xz, rms_y, degenerate))."""
    return _host_solve("sl3d_align_solve", ALIGN_WORDS, sums, range, ox, oz, est)


def align_plane_solve(sums, range, ox, oz, est):
    """sl3d_align_plane_solve: the Gauss-Newton solve over the (n_pairs, 18) int64 words of a point-to-plane pass (the rule:
    include/sl3d_align_plane.h); host only, no context.  est: (c, s, tx, tz).  Returns (the new estimate float64[4], dict(n, rms_xz,
    rms_y, degenerate)): rms_xz carries rms_plane, rms_y is NaN."""
    return _host_solve("sl3d_align_plane_solve", ALIGN_PLANE_WORDS, sums, range, ox, oz, est)


def tsdf_bounds(cloud, voxel, margin=2):
    """(origin float32[3], dims (nx, ny, nz)) of the TSDF volume of edge `voxel` around a registered cloud ((n, 3), points that are not
    finite ignored) with `margin` voxels of room on every side: what Scanner.tsdf_reset takes."""
    p = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if not len(p):
        raise Sl3dError("tsdf_bounds: the cloud has no finite point")
    L = float(np.float32(voxel))
    origin = (np.floor(p.min(axis=0) / L) - margin).astype(np.float64) * L
    origin = origin.astype(np.float32)
    dims = np.ceil((p.max(axis=0) - origin.astype(np.float64)) / L).astype(np.int64) + margin
    return origin, tuple(int(max(d, 1)) for d in dims)


def _cut(flat, counts):
    """The per-view slices of an array that holds the views' rows back to back, counts[k] of view k."""
    ends = np.cumsum(counts, dtype=np.int64)
    return [flat[e - n:e] for n, e in zip(counts, ends)]


def _ptrs(arrs):
    """The void* array the C side takes for a list of planes."""
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


_XYZ, _RGB, _TRI, _IDS, _CNT = (np.float32, 3), (np.uint8, 3), (np.int32, 3), (np.int32,), (np.uint32,)   # an output array: (dtype, *shape of one row)


class _Handle:
    """What Scanner and Group share: the life of the handle, the status check, the calling idioms of the C ABI written once each, and
    the methods that differ by the symbol prefix alone."""
    _prefix = "sl3d_"

    def close(self):
        if getattr(self, "_h", None):
            getattr(self.L, self._prefix + "destroy")(self._h)
            self._h = None
        for p in getattr(self, "_pinned", []):
            self.L.sl3d_host_free(p)
        self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            last_error = getattr(self.L, self._prefix + "last_error")
            raise Sl3dError(f"{what}: {self.L.sl3d_strerror(rc).decode()}: {last_error(self._h).decode()}")

    def _call(self, name, *args):
        """<prefix><name>(handle, *args), checked."""
        name = self._prefix + name
        self._chk(getattr(self.L, name)(self._h, *args), name)

    def _planes(self, planes):
        """(the H x W uint8 planes as contiguous arrays -- keep them alive over the call --, their pointer array)"""
        arrs = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
        for a in arrs:
            assert a.shape == (self.H, self.W), a.shape
        return arrs, _ptrs(arrs)

    def _plane(self, fn, dtype, view, *pre, comps=1, tail=None):
        """A fresh (H, W) or (H, W, comps) image filled by fn(handle, view, *pre, image, *tail); tail: by default the row stride in elements."""
        shape = (self.H, self.W) if comps == 1 else (self.H, self.W, comps)
        out = np.empty(shape, dtype=dtype)
        self._chk(getattr(self.L, fn)(self._h, view, *pre, out.ctypes.data, *((self.W * comps,) if tail is None else tail)), fn)
        return out

    def _counts(self, fn, n_counts, first_view, n_views, *args):
        """fn(handle, first_view, n_views, *args, count arrays...) with n_counts arrays of n_views int64: the counts as lists of int."""
        counts = [(C.c_int64 * n_views)() for _ in range(n_counts)]
        self._chk(getattr(self.L, fn)(self._h, first_view, n_views, *args, *counts), fn)
        return [[int(c) for c in a] for a in counts]

    def _fill(self, fn, args, *specs):
        """Size then fill with one count: fn(handle, *args, outputs..., capacity, &n) is called with null outputs and capacity 0 for n,
        then with fresh arrays of n rows, one per spec (dtype, *shape of a row); returns the arrays."""
        n, f = C.c_int64(0), getattr(self.L, fn)
        self._chk(f(self._h, *args, *[None] * len(specs), 0, C.byref(n)), fn)
        outs = [np.empty((n.value,) + s[1:], dtype=s[0]) for s in specs]
        self._chk(f(self._h, *args, *[o.ctypes.data for o in outs], n.value, C.byref(n)), fn)
        return outs

    def _fill_views(self, fn, first_view, n_views, args, *groups, n_counts):
        """Size then fill for a batch of views: fn(handle, first_view, n_views, *args, vertex outputs..., vertex capacity[, face outputs...,
        face capacity], count arrays...) is called with null outputs and capacities 0 for the per-view counts, then with arrays of their
        sums.  groups: the vertex outputs and, where the function has them, the face outputs, each a list in the C order of (dtype,
        *shape of a row) for a fresh array, None for an output that is not requested (it stays null) or a 2-D array to fill; the first
        of a group is always requested.  Of the n_counts count arrays of n_views int64 the first holds the vertex counts, the second
        (with faces) the face counts.  Returns, per group, the list of its outputs cut per view (None for a null one), then the count arrays."""
        counts, f = [(C.c_int64 * n_views)() for _ in range(n_counts)], getattr(self.L, fn)

        def call(filled):
            outs = []
            for arrs in filled:
                outs += [None if a is None else a.ctypes.data for a in arrs] + [0 if arrs[0] is None else len(arrs[0])]
            self._chk(f(self._h, first_view, n_views, *args, *outs, *counts), fn)

        call([[None] * len(g) for g in groups])
        filled = []
        for g, c in zip(groups, counts):
            filled.append([s if s is None or isinstance(s, np.ndarray) else np.empty((sum(c),) + s[1:], dtype=s[0]) for s in g])
            assert all(a is None or len(a) >= sum(c) for a in filled[-1])
        call(filled)
        return (*[[None if a is None else _cut(a, c) for a in arrs] for arrs, c in zip(filled, counts)], counts)

    # ---- what Scanner and Group differ in by the prefix alone -----------------------------------
    def set_calibration(self, Kc, dc, rc, tc, Kp, dp, rp, tp):
        a = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in (Kc, dc, rc, tc, Kp, dp, rp, tp)]
        assert [v.size for v in a] == [9, 5, 3, 3, 9, 5, 3, 3]
        self._call("set_calibration", *[v.ctypes.data for v in a])

    def set_mask(self, full_frame_mask, view=0):
        m = np.ascontiguousarray(full_frame_mask, dtype=np.uint8)
        assert m.shape == (self.cfg.full_height, self.cfg.full_width), m.shape
        self._call("set_mask", view, m.ctypes.data, m.strides[0])

    def set_frames(self, axis, planes, view=0):
        arrs, ptrs = self._planes(planes)
        self._call("set_frames", view, axis, ptrs, len(arrs), arrs[0].strides[0])

    def points(self, view=0):
        xyz = np.empty((self.H, self.W, 3), dtype=np.float32)
        return xyz, self._plane(self._prefix + "get_points", np.uint8, view, xyz.ctypes.data, tail=())

    def cloud(self, view=0):
        return self._fill(self._prefix + "get_cloud", (view,), _XYZ)[0]

    def _process_views(self, frames, xyz, valid):
        """frames: the 4-D array, or per view a sequence of planes_per_view planes in which a plane the context does not read (the other
        axis of a one-axis scan, the inverse Gray planes under SL3D_FLAG_DIRECT_GRAY) may be None: its pointer goes down as NULL."""
        H, W = self.H, self.W
        if isinstance(frames, np.ndarray):
            n, ppv = frames.shape[:2]
            assert frames.shape[2:] == (H, W) and frames.dtype == np.uint8 and frames.strides[3] == 1 and frames.strides[2] >= W
            planes, stride = [frames[v, p] for v in range(n) for p in range(ppv)], frames.strides[2]
        else:
            n, stride = len(frames), W
            assert n >= 1 and len({len(v) for v in frames}) == 1, "every view lists planes_per_view planes (None for one that is not read)"
            planes = [None if p is None else np.ascontiguousarray(p, dtype=np.uint8) for v in frames for p in v]
            assert all(p is None or p.shape == (H, W) for p in planes)
        if xyz is None:
            xyz = np.empty((n, H, W, 3), dtype=np.float32)
        if valid is None:
            valid = np.empty((n, H, W), dtype=np.uint8)
        ptrs = (C.c_void_p * len(planes))(*[None if p is None else p.ctypes.data for p in planes])
        self._call("process_views", n, ptrs, stride, xyz.ctypes.data, valid.ctypes.data)
        return xyz, valid


class Scanner(_Handle):
    """One context = one GPU + one stream + the HBM-resident frame stacks of `max_views` views."""

    def __init__(self, width, height, proj_width, proj_height, n_gray_v, n_gray_h, fringe_width_v, fringe_width_h,
                 n_fringe=3, n_codes_v=0, n_codes_h=0, max_views=1, device=0, keep_stages=False,
                 full_size=None, origin=(0, 0), stream=None, eager_mask=False, serial_launches=False, subpixel=False, repaired=False,
                 anchored=False, only_axis=None, direct_gray=False):
        """eager_mask: SL3D_FLAG_EAGER_MASK -- every mask is prepared by k_mask_prepare when it is set; by default a timed context
        defers masks of up to 4 views to the next launch over them (the fused kernel evaluates the selection itself).
        subpixel: SL3D_FLAG_SUBPIXEL -- run() (and process_views) leaves the sub-pixel scan and its residual plane: what the per-stage
        calls and triangulate_subpixel() leave on a keep_stages context, as one launch per call on a timed one.
        repaired: SL3D_FLAG_REPAIR_PERIODS -- run() (and process_views) leaves the scan with the 2*Pi period jumps repaired: what one
        repair_periods(view, axis, 4) pass over each axis that has Gray planes, between unwrap_phase and compute_c_p_map, leaves on a
        keep_stages context, as one launch per call on a timed one.  (Not `repair_periods`: that name is the method.)  Other radii,
        several passes and the counts stay with repair_periods(); a Group refuses the flag.
        anchored: SL3D_FLAG_ANCHOR_PERIODS -- the sub-pixel scan (run(), triangulate_subpixel(), correspondences_subpixel()) takes the
        projector coordinates from the fringe period nearest the centre of the pixel's Gray cell, measured with pi instead of 22/7;
        validity, c_p_map and the stage planes stay as they are.  Needs subpixel=True and excludes repaired=True (and repair_periods()):
        the library refuses the other combinations.  Groups: flags=SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS.
        only_axis: None, or the one pattern direction the scan is made from -- 0: SL3D_FLAG_ONLY_VERTICAL (the projector column), 1:
        SL3D_FLAG_ONLY_HORIZONTAL (the row).  The frames of the other axis are never read (they need not be set, process_views does not
        upload them), a pixel is the intersection of its camera ray with the plane of the decoded coordinate, and there are no
        residuals.  Needs subpixel=True, an undistorted projector with a plain matrix, and excludes repaired=True; may be combined with
        anchored=True.  Groups: flags=SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ONLY_VERTICAL.
        direct_gray: SL3D_FLAG_DIRECT_GRAY -- stage 4 thresholds a Gray frame against the mean of the pixel's fringe frames, (2 * gray -
        (I0 + I2) >= 0), instead of against its inverse frame: no inverse Gray frame is read, so a coded axis needs F + N frames instead
        of F + 2 N.  set_frames() then also takes those F + N planes alone, and process_views() a per-view list of planes with None for
        the inverse ones.  Needs subpixel=True and excludes repaired=True (repair_periods() on a keep_stages scanner works); may be
        combined with keep_stages, anchored, only_axis, eager_mask and serial_launches.  Groups: flags=SL3D_FLAG_SUBPIXEL |
        SL3D_FLAG_DIRECT_GRAY."""
        if only_axis not in (None, 0, 1):
            raise ValueError("only_axis must be None, 0 or 1")
        self.L = load_library()
        fw, fh = full_size if full_size else (width, height)
        self.cfg = Config(width, height, fw, fh, origin[0], origin[1], proj_width, proj_height, n_fringe,
                          n_gray_v, n_gray_h, fringe_width_v, fringe_width_h, n_codes_v, n_codes_h,
                          max_views, device, (SL3D_FLAG_KEEP_STAGES if keep_stages else 0) | (SL3D_FLAG_EAGER_MASK if eager_mask else 0) |
                          (SL3D_FLAG_SERIAL_LAUNCHES if serial_launches else 0) | (SL3D_FLAG_SUBPIXEL if subpixel else 0) |
                          (SL3D_FLAG_REPAIR_PERIODS if repaired else 0) | (SL3D_FLAG_ANCHOR_PERIODS if anchored else 0) |
                          {None: 0, 0: SL3D_FLAG_ONLY_VERTICAL, 1: SL3D_FLAG_ONLY_HORIZONTAL}[only_axis] |
                          (SL3D_FLAG_DIRECT_GRAY if direct_gray else 0), stream)
        self.W, self.H = width, height
        self._h = C.c_void_p()
        rc = self.L.sl3d_create(C.byref(self.cfg), C.byref(self._h))
        if rc != 0:
            raise Sl3dError(f"sl3d_create: {self.L.sl3d_strerror(rc).decode()}: {self.L.sl3d_last_error(None).decode()}")

    # ---- inputs -------------------------------------------------------------------------------
    def projection_matrices(self):
        """(A_cam, A_proj): the 3x4 matrices K [R|t] the library derived from the calibration (T0, compute_A)."""
        a, b = np.zeros(12), np.zeros(12)
        self._chk(self.L.sl3d_get_projection_matrices(self._h, a.ctypes.data, b.ctypes.data), "sl3d_get_projection_matrices")
        return a.reshape(3, 4), b.reshape(3, 4)

    def _mask_args(self, m, first_view, n_views):
        """(number of views, address, row stride, view stride) of a mask argument m, a contiguous uint8 array: None, one full-frame mask
        that n_views views get (by default all from first_view on: view stride 0) or a stack [n][full_height][full_width]."""
        if m is None or m.ndim == 2:
            assert m is None or m.shape == (self.cfg.full_height, self.cfg.full_width), m.shape
            n, vs = (self.cfg.max_views - first_view if n_views is None else n_views), 0
        else:
            assert m.shape[1:] == (self.cfg.full_height, self.cfg.full_width), m.shape
            n, vs = m.shape[0], m.strides[0]
            assert n_views is None or n_views == n
        return (n, None, 0, vs) if m is None else (n, m.ctypes.data, m.strides[-2], vs)

    def set_masks(self, masks, first_view=0, n_views=None):
        """One launch for several views.  masks: one full-frame mask (every view gets it) or an array [n][full_height][full_width]."""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if os.environ.get("SL3D_LIB") and not hasattr(self.L, "sl3d_set_masks"):   # an older build under SL3D_LIB (A/B runs): view by view
            n = (self.cfg.max_views - first_view if n_views is None else n_views) if m.ndim == 2 else m.shape[0]
            for k in range(n):
                self.set_mask(m if m.ndim == 2 else m[k], view=first_view + k)
            return
        n, ptr, stride, vs = self._mask_args(m, first_view, n_views)
        self._chk(self.L.sl3d_set_masks(self._h, first_view, n, ptr, stride, vs), "sl3d_set_masks")

    def set_masks_device(self, dev_ptr, stride, view_stride, first_view=0, n_views=1):
        """Masks that already live in device memory (a raw address, e.g. torch.Tensor.data_ptr())."""
        self._chk(self.L.sl3d_set_masks(self._h, first_view, n_views, C.c_void_p(dev_ptr), stride, view_stride), "sl3d_set_masks")

    def set_masks_modulated(self, min_modulation, masks=None, first_view=0, n_views=None):
        """set_masks with the fringe-modulation test (sl3d_set_masks_modulated): a pixel stays selected iff its mask byte is 1 (no mask:
        every pixel) and the modulation gamma of both axes' fringes, as resident now, is > min_modulation.  masks: None, one full-frame
        mask (every view gets it) or an array [n][full_height][full_width].  Whole-frame contexts with 3 fringes only."""
        m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8)
        n, ptr, stride, vs = self._mask_args(m, first_view, n_views)
        self._chk(self.L.sl3d_set_masks_modulated(self._h, first_view, n, float(min_modulation), ptr, stride, vs), "sl3d_set_masks_modulated")

    def set_masks_modulated_device(self, min_modulation, dev_ptr, stride, view_stride, first_view=0, n_views=1):
        """set_masks_modulated with masks that already live in device memory (a raw address, e.g. torch.Tensor.data_ptr())."""
        self._chk(self.L.sl3d_set_masks_modulated(self._h, first_view, n_views, float(min_modulation), C.c_void_p(dev_ptr), stride, view_stride),
                  "sl3d_set_masks_modulated")

    def modulation(self, axis, view=0):
        """gamma of one axis (sl3d_get_modulation): float32 [H][W] of the window, NaN where the three fringe bytes are all 0."""
        return self._plane("sl3d_get_modulation", np.float32, view, axis)

    def set_mask_colrow(self, selected_region, view=0):
        """selected_region as the reference holds it: int32 array [full_width][full_height] ([col][row]), selected iff == 1."""
        m = np.ascontiguousarray(selected_region, dtype=np.int32)
        assert m.shape == (self.cfg.full_width, self.cfg.full_height), m.shape
        self._chk(self.L.sl3d_set_mask_colrow(self._h, view, m.ctypes.data), "sl3d_set_mask_colrow")

    def set_frames(self, axis, planes, view=0):
        """The F + 2 N planes of one axis; a direct_gray scanner also takes the F + N fringe and Gray planes alone (it reads no inverse
        plane): they go through sl3d_set_frames_range."""
        n_read = self.cfg.n_fringe + (self.cfg.n_gray_v if axis == 0 else self.cfg.n_gray_h)
        if self.cfg.flags & SL3D_FLAG_DIRECT_GRAY and len(planes) == n_read:
            return self.set_frames_range(axis, 0, planes, view=view)
        return super().set_frames(axis, planes, view=view)

    def set_frames_range(self, axis, first_plane, planes, view=0):
        arrs, ptrs = self._planes(planes)
        self._chk(self.L.sl3d_set_frames_range(self._h, view, axis, first_plane, ptrs, len(arrs), arrs[0].strides[0]), "sl3d_set_frames_range")

    def global_colrow(self, which, view=0, out=None, row0=0):
        """One of the reference's globals in its own [col][row] layout and type (sl3d_get_global_colrow); `out`: a [W][H_total(,3)]
        array this window's rows are written into at row offset row0 (default: a fresh [W][H] array)."""
        dt, comps = (np.float64, 3) if which == 9 else (np.float32, 1) if 3 <= which <= 6 else (np.int32, 1)
        if out is None:
            out = np.empty((self.W, self.H) + ((3,) if comps == 3 else ()), dtype=dt)
        assert out.dtype == dt and out.flags["C_CONTIGUOUS"] and out.shape[0] == self.W
        self._chk(self.L.sl3d_get_global_colrow(self._h, view, which, out.ctypes.data, out.shape[1], row0), "sl3d_get_global_colrow")
        return out

    def set_frames_raw(self, axis, planes, view=0):
        """set_frames for raw captures: undistorted on the device with the camera calibration (whole frames only)."""
        arrs, ptrs = self._planes(planes)
        self._chk(self.L.sl3d_set_frames_raw(self._h, view, axis, ptrs, len(arrs), arrs[0].strides[0]), "sl3d_set_frames_raw")

    def synth_view(self, view=0, plane=(0.0, 0.05, 0.05), seed=0x3D5CA11, view_id=None, noise=0, gain=0.8, offset=10.0):
        """Synthetic capture generated on the device into slot `view` (see 3dscan_amd/synth.py for the host twin)."""
        pl = np.asarray(plane, dtype=np.float64)
        self._chk(self.L.sl3d_synth_view(self._h, view, pl.ctypes.data, seed, view if view_id is None else view_id, noise, gain, offset),
                  "sl3d_synth_view")

    def frames(self, axis, view=0):
        n = self.cfg.n_fringe + 2 * (self.cfg.n_gray_v if axis == 0 else self.cfg.n_gray_h)
        arrs, ptrs = self._planes([np.empty((self.H, self.W), dtype=np.uint8) for _ in range(n)])
        self._chk(self.L.sl3d_get_frames(self._h, view, axis, ptrs, n, self.W), "sl3d_get_frames")
        return arrs

    def copy_view(self, src_view, dst_view):
        self._chk(self.L.sl3d_copy_view(self._h, src_view, dst_view), "sl3d_copy_view")

    def fuse_exposures(self, first_view, n_exposures, dst_view, saturation=255, counts=True):
        """sl3d_fuse_exposures: views first_view .. first_view + n_exposures - 1 hold one pattern set at n_exposures (1 .. 8) exposures;
        dst_view gets, per pixel, the bytes of the exposure with the fewest planes >= saturation, among those the best modulated, among
        those the first (the rule: include/sl3d_fuse.h).  Returns np.uint32[n_exposures + 1]: the pixels taken from each exposure, then the
        pixels clipped in every exposure; counts=False: the call stays asynchronous and returns None."""
        out = (C.c_uint32 * (max(n_exposures, 0) + 1))() if counts else None
        self._chk(self.L.sl3d_fuse_exposures(self._h, first_view, n_exposures, dst_view, saturation, out), "sl3d_fuse_exposures")
        return np.array(out, dtype=np.uint32) if counts else None

    def exposure_map(self, view=0):
        """The map the last fuse_exposures into `view` left: uint8 [H][W], the chosen exposure | 0x80 where that exposure clips."""
        return self._plane("sl3d_get_exposure_map", np.uint8, view)

    def filter_outliers(self, radius, max_dist, min_neighbours, first_view=0, n_views=1, counts=True):
        """sl3d_filter_outliers: every valid pixel of views first_view .. first_view + n_views - 1 that has fewer than min_neighbours valid
        pixels within max_dist (mm, 3-D) among the (2 * radius + 1)^2 - 1 pixels around it (radius 1 .. 4) loses its valid byte, its point
        becomes NaN (the rule: include/sl3d_filter.h).  In place: points(), cloud(), the meshes ... then see the filtered scan; run() over the
        view restores it.  min_neighbours=0 only writes the support planes.  Returns np.uint32[n_views][2]: per view the valid pixels on
        entry and the rejected ones; counts=False: the call stays asynchronous and returns None."""
        out = (C.c_uint32 * (2 * max(n_views, 1)))() if counts else None
        self._chk(self.L.sl3d_filter_outliers(self._h, first_view, n_views, radius, max_dist, min_neighbours, out), "sl3d_filter_outliers")
        return np.array(out, dtype=np.uint32).reshape(n_views, 2) if counts else None

    def support(self, view=0):
        """The plane the last filter_outliers over `view` left: uint8 [H][W], the number of valid neighbours within max_dist, 0xFF where the
        pixel was not valid."""
        return self._plane("sl3d_get_support", np.uint8, view)

    # ---- the reference's four stage entry points ----------------------------------------------
    def compute_wrapped_phase(self, pattern_type, view=0):
        self._chk(self.L.sl3d_compute_wrapped_phase(self._h, view, pattern_type), "sl3d_compute_wrapped_phase")

    def unwrap_phase(self, pattern_type, view=0):
        self._chk(self.L.sl3d_unwrap_phase(self._h, view, pattern_type), "sl3d_unwrap_phase")

    def _counted(self, fn, want_counts, n_pairs, *args):
        """fn(handle, *args, counts) with room for n_pairs pairs of uint32: the pairs as tuples of int, which makes the call wait; or, with
        want_counts=False, with null (the call stays asynchronous): None."""
        counts = (C.c_uint32 * (2 * n_pairs))() if want_counts else None
        self._chk(getattr(self.L, fn)(self._h, *args, counts), fn)
        return [(int(counts[2 * k]), int(counts[2 * k + 1])) for k in range(n_pairs)] if want_counts else None

    def repair_periods(self, axis, radius=4, view=0, want_counts=True):
        """sl3d_repair_periods between unwrap_phase and compute_c_p_map: whole 2*Pi periods taken out of the absolute phase of one axis
        against the lower median of the samples within `radius` pixels along the coded direction; (repaired, unrepairable) pixels of the pass.
        want_counts=False: the call stays asynchronous and returns None."""
        c = self._counted("sl3d_repair_periods", want_counts, 1, view, axis, radius)
        return c[0] if c else None

    def compute_c_p_map(self, view=0):
        self._chk(self.L.sl3d_compute_c_p_map(self._h, view), "sl3d_compute_c_p_map")

    def triangulate(self, view=0):
        self._chk(self.L.sl3d_triangulate(self._h, view), "sl3d_triangulate")

    def triangulate_subpixel(self, first_view=0, n_views=1, max_residual=float("inf"), want_counts=True):
        """sl3d_triangulate_subpixel in place of triangulate, after compute_c_p_map: stage 7 from the continuous projector coordinates
        (the doubles stage 5 rounds) for a batch of views in one launch, the reprojection residual of every solve kept as a plane
        (residuals); a finite max_residual rejects the pixels whose stored residual is not <= it.  Returns a list of
        (triangulated, rejected) per view; want_counts=False: the call stays asynchronous and returns None."""
        c = self._counted("sl3d_triangulate_subpixel", want_counts, max(n_views, 1), first_view, n_views, float(max_residual))
        return c[:n_views] if c else None

    def run_stages(self, view=0):
        """main()'s order (m_tech_project_console.cpp:372-395) through the per-stage kernels."""
        self.compute_wrapped_phase(0, view); self.compute_wrapped_phase(1, view)
        self.unwrap_phase(0, view); self.unwrap_phase(1, view)
        self.compute_c_p_map(view)
        self.triangulate(view)

    # ---- fused hot path -----------------------------------------------------------------------
    def run(self, first_view=0, n_views=1):
        self._chk(self.L.sl3d_run(self._h, first_view, n_views), "sl3d_run")

    def run_clouds(self, first_view=0, n_views=1):
        """The fused pass with the ordered compaction inside the kernel (sl3d_run_clouds); asynchronous."""
        self._chk(self.L.sl3d_run_clouds(self._h, first_view, n_views), "sl3d_run_clouds")

    def cloud_counts(self, first_view=0, n_views=1, want_device_copy=True):
        """(device address of the first CONTIGUOUS cloud, points between clouds, [count per view]) after run_clouds; synchronises.
        want_device_copy=False: counts only (address None) -- segmented clouds then need no gap-closing launch."""
        counts = (C.c_int64 * n_views)()
        ptr, stride = C.c_void_p(), C.c_size_t()
        self._chk(self.L.sl3d_get_cloud_counts(self._h, first_view, n_views, C.byref(ptr) if want_device_copy else None, C.byref(stride), counts),
                  "sl3d_get_cloud_counts")
        return ptr.value, stride.value, [int(c) for c in counts]

    def cloud_segments(self, first_view=0, n_views=1):
        """(CloudSegments, [count per view]): the segmented clouds of the last run_clouds where they lie in HBM."""
        seg = CloudSegments()
        return (seg, *self._counts("sl3d_get_cloud_segments", 1, first_view, n_views, C.byref(seg)))

    def download_clouds(self, first_view=0, n_views=1, out=None):
        """Host copies of the clouds of the last run_clouds: list of (n_k, 3) float32 arrays (views of `out`, a flat float32 buffer --
        pinned for the zero-copy route -- or of a fresh array)."""
        assert out is None or out.dtype == np.float32
        xyz = _XYZ if out is None else out.reshape(-1)[:out.size // 3 * 3].reshape(-1, 3)
        (clouds,), _ = self._fill_views("sl3d_download_clouds", first_view, n_views, (), [xyz], n_counts=1)
        return clouds

    def download_cloud_into(self, view, out):
        """ONE call of sl3d_download_clouds for one view into `out` (flat float32 buffer; capacity = out.size // 3 points): the number
        of valid points of the view (which may exceed the capacity: then the first `capacity` points were written).  With a pinned
        buffer behind a run_clouds of a few views this is the route without a scan launch (the gap-closing kernel scans on entry)."""
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        counts = (C.c_int64 * 1)()
        self._chk(self.L.sl3d_download_clouds(self._h, view, 1, out.ctypes.data, out.size // 3, counts), "sl3d_download_clouds")
        return int(counts[0])

    def register_clouds(self, first_view, n_views, tx, ty, tz, rot_step):
        """register_views on the clouds of the last run_clouds (rotation applied while the segments are concatenated)."""
        return self._fill("sl3d_register_clouds", (first_view, n_views, tx, ty, tz, rot_step), _XYZ)[0]

    def fused_clouds(self, first_view=0, n_views=1):
        """run_clouds + host copies: list of (n_k, 3) float32 arrays in the reference's scan order."""
        self.run_clouds(first_view, n_views)
        ptr, stride, counts = self.cloud_counts(first_view, n_views)
        out = []
        for k, n in enumerate(counts):
            a = np.empty((n, 3), dtype=np.float32)
            if n:
                self._d2h(a, ptr + 12 * k * stride)
            out.append(a)
        return out

    def _d2h(self, arr, dev_ptr):
        """Device -> host copy of an address the library handed out (sl3d_download)."""
        self._chk(self.L.sl3d_download(self._h, arr.ctypes.data, dev_ptr, arr.nbytes), "sl3d_download")

    def fused_kernel_name(self, n_views=1, clouds=False):
        """The k_fused instantiation a launch over n_views views runs, as rocprofv3 prints it."""
        if os.environ.get("SL3D_LIB") and not hasattr(self.L, "sl3d_fused_kernel_name"):
            return "(a build without sl3d_fused_kernel_name)"
        buf = C.create_string_buffer(256)
        self._chk(self.L.sl3d_fused_kernel_name(self._h, n_views, 1 if clouds else 0, buf, len(buf)), "sl3d_fused_kernel_name")
        return buf.value.decode()

    def camera_table_bytes_per_pixel(self, n_views=1):
        """Bytes per pixel a launch of n_views views reads from the camera-side table (once per launch); None with a build that cannot say."""
        if not hasattr(self.L, "sl3d_camera_table_bytes_per_pixel"):
            return None
        n = self.L.sl3d_camera_table_bytes_per_pixel(self._h, n_views)
        if n < 0:
            self._chk(n, "sl3d_camera_table_bytes_per_pixel")
        return n

    def launch_counts(self):
        """(fused launches that went to the context's stream, ... to its launch lanes)"""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.L.sl3d_launch_counts(self._h, C.byref(a), C.byref(b)), "sl3d_launch_counts")
        return a.value, b.value

    def last_fused_kernel_name(self):
        """The k_fused instantiation the last fused launch of this context ran."""
        if os.environ.get("SL3D_LIB") and not hasattr(self.L, "sl3d_last_fused_kernel_name"):
            return "(a build without sl3d_last_fused_kernel_name)"
        buf = C.create_string_buffer(256)
        self._chk(self.L.sl3d_last_fused_kernel_name(self._h, buf, len(buf)), "sl3d_last_fused_kernel_name")
        return buf.value.decode()

    def run_timed(self, first_view=0, n_views=1):
        ms = C.c_float(0)
        self._chk(self.L.sl3d_run_timed(self._h, first_view, n_views, C.byref(ms)), "sl3d_run_timed")
        return ms.value

    def timer_start(self):
        self._chk(self.L.sl3d_timer_start(self._h), "sl3d_timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        self._chk(self.L.sl3d_timer_stop(self._h, C.byref(ms)), "sl3d_timer_stop")
        return ms.value

    def synchronize(self):
        self._chk(self.L.sl3d_synchronize(self._h), "sl3d_synchronize")

    # ---- outputs ------------------------------------------------------------------------------
    def valid_map(self, which=VALID_MERGED, view=0):
        return self._plane("sl3d_get_valid_map", np.uint8, view, which)

    def wrapped_phase(self, axis, view=0):
        return self._plane("sl3d_get_wrapped_phase", np.float32, view, axis)

    def unwrapped_phase(self, axis, view=0):
        return self._plane("sl3d_get_unwrapped_phase", np.float32, view, axis)

    def code(self, axis, view=0):
        return self._plane("sl3d_get_code", np.int32, view, axis)

    def debug_image(self, stage, axis, view=0):
        return self._plane("sl3d_get_debug_image", np.uint8, view, stage, axis)

    def c_p_map(self, view=0):
        return self._plane("sl3d_get_c_p_map", np.int64, view, comps=2, tail=())

    def intersection_points(self, view=0):
        return self._plane("sl3d_get_intersection_points", np.float64, view, comps=3, tail=())

    def residuals(self, view=0):
        """The reprojection residual (undistorted pixels, camera and projector together) of every pixel the last triangulate_subpixel
        over the view triangulated; NaN elsewhere.  On a Scanner(subpixel=True) the last run() over the view writes it too -- every
        pixel of the view: the residual where the scan is valid, NaN elsewhere; before the first run() the call raises."""
        return self._plane("sl3d_get_residuals", np.float32, view)

    def correspondences_subpixel(self, view=0):
        """(H, W, 2) float64: the continuous projector coordinates (xs, ys) stage 5 rounds into c_p_map; NaN where either axis is invalid."""
        return self._plane("sl3d_get_correspondences_subpixel", np.float64, view, comps=2, tail=(self.W,))

    def download_views(self, first_view, n_views, xyz, valid):
        """Dense results of views [first_view, first_view + n_views) into caller arrays (n, H, W, 3) f32 / (n, H, W) u8 (pinned
        for full-rate DMA): one 2-D copy per view and plane, one wait."""
        assert xyz.shape == (n_views, self.H, self.W, 3) and valid.shape == (n_views, self.H, self.W)
        b = self.device_buffers()
        for k in range(n_views):
            self._chk(self.L.sl3d_download_2d(self._h, xyz[k].ctypes.data, self.W * 12, b.points + (first_view + k) * b.points_view_stride,
                                              b.points_pitch, self.W * 12, self.H), "sl3d_download_2d")
            self._chk(self.L.sl3d_download_2d(self._h, valid[k].ctypes.data, self.W, b.valid + (first_view + k) * b.valid_view_stride,
                                              b.valid_pitch, self.W, self.H), "sl3d_download_2d")
        self.synchronize()

    def compact_views(self, first_view, n_views):
        """Batched device compaction (three launches for all views); returns the per-view counts, clouds stay in HBM."""
        return self._counts("sl3d_compact_views", 1, first_view, n_views, None, None)[0]

    def clouds(self, first_view, n_views):
        """The compacted clouds of a batch of views as a list of (n_k, 3) float32 arrays."""
        (clouds,), _ = self._fill_views("sl3d_get_clouds", first_view, n_views, (), [_XYZ], n_counts=1)
        return clouds

    def mesh_device(self, max_edge, first_view=0, n_views=1):
        """sl3d_mesh_views: the meshes of a batch of views left in HBM; returns (Mesh, vertex counts, face counts)."""
        m = Mesh()
        return (m, *self._counts("sl3d_mesh_views", 2, first_view, n_views, float(max_edge), C.byref(m)))

    def meshes(self, max_edge, first_view=0, n_views=1):
        """The meshes of a batch of views: a list of (xyz float32 (n, 3), faces int32 (m, 3)); xyz is the view's compacted cloud (the
        valid pixels in scan order), a face three indices into it.  Neighbouring valid pixels are connected unless an edge longer than
        max_edge (mm; float('inf'): no test) lies between them (include/sl3d.h: the exact definition)."""
        (xyz,), (faces,), _ = self._fill_views("sl3d_get_meshes", first_view, n_views, (float(max_edge),), [_XYZ], [_TRI], n_counts=2)
        return list(zip(xyz, faces))

    def mesh(self, max_edge, view=0):
        """(xyz, faces) of one view (meshes)."""
        return self.meshes(max_edge, view, 1)[0]

    def mesh_normals_device(self, max_edge, first_view=0, n_views=1):
        """sl3d_mesh_normals: the vertex normals of the meshes of a batch of views left in HBM; returns (device address, stride between
        the views in float triples, vertex counts)."""
        dev, stride = C.c_void_p(), C.c_size_t()
        counts = self._counts("sl3d_mesh_normals", 1, first_view, n_views, float(max_edge), C.byref(dev), C.byref(stride))
        return (dev.value, stride.value, *counts)

    def meshes_normals(self, max_edge, first_view=0, n_views=1):
        """The vertex normals of meshes(max_edge, first_view, n_views): a list of (n_k, 3) float32 arrays, row i the unit normal of
        vertex i -- the normalised sum of the area-weighted normals of the faces around it, zero for a vertex in no face.  The
        orientation follows the faces; nothing is flipped towards the camera (include/sl3d.h: the exact definition)."""
        (normals,), _ = self._fill_views("sl3d_get_mesh_normals", first_view, n_views, (float(max_edge),), [_XYZ], n_counts=1)
        return normals

    def mesh_normals(self, max_edge, view=0):
        """(n, 3) float32 normals of the vertices of mesh(max_edge, view) (meshes_normals)."""
        return self.meshes_normals(max_edge, view, 1)[0]

    def mesh_components_device(self, max_edge, first_view=0, n_views=1):
        """sl3d_mesh_components: the component labels of the meshes of a batch of views left in HBM; returns (device address, stride
        between the views in labels, vertex counts, component counts)."""
        dev, stride = C.c_void_p(), C.c_size_t()
        counts = self._counts("sl3d_mesh_components", 2, first_view, n_views, float(max_edge), C.byref(dev), C.byref(stride))
        return (dev.value, stride.value, *counts)

    def meshes_components(self, max_edge, first_view=0, n_views=1):
        """The connected components of meshes(max_edge, first_view, n_views): a list of (n_k,) int32 arrays, entry i the smallest vertex
        id of the component of vertex i (two vertices are connected iff they share a face; a vertex in no face is a component of its
        own).  The roots are the i with labels[i] == i (include/sl3d.h: the exact definition)."""
        (labels,), _ = self._fill_views("sl3d_get_mesh_components", first_view, n_views, (float(max_edge),), [_IDS], n_counts=2)
        return labels

    def mesh_components(self, max_edge, view=0):
        """(n,) int32 component labels of the vertices of mesh(max_edge, view) (meshes_components)."""
        return self.meshes_components(max_edge, view, 1)[0]

    def mesh_filtered_device(self, max_edge, min_vertices, first_view=0, n_views=1):
        """sl3d_mesh_views_filtered: the filtered meshes of a batch of views left in HBM; returns (MeshFiltered, vertex counts, face
        counts)."""
        m = MeshFiltered()
        return (m, *self._counts("sl3d_mesh_views_filtered", 2, first_view, n_views, float(max_edge), int(min_vertices), C.byref(m)))

    def meshes_filtered(self, max_edge, min_vertices, first_view=0, n_views=1):
        """meshes(max_edge, first_view, n_views) without the components of fewer than min_vertices vertices: a list of (xyz float32
        (n, 3), faces int32 (m, 3), vertex_ids int32 (n,)); the kept vertices in order, the original faces among them with the new ids,
        vertex_ids[i] the id new vertex i has in mesh() -- mesh_normals(...)[vertex_ids] and cloud_rgb()[1][vertex_ids] are the normals
        and colours of the filtered mesh (include/sl3d.h: the exact definition)."""
        args = (float(max_edge), int(min_vertices))
        (xyz, ids), (faces,), _ = self._fill_views("sl3d_get_meshes_filtered", first_view, n_views, args, [_XYZ, _IDS], [_TRI], n_counts=2)
        return list(zip(xyz, faces, ids))

    def mesh_filtered(self, max_edge, min_vertices, view=0):
        """(xyz, faces, vertex_ids) of one view (meshes_filtered)."""
        return self.meshes_filtered(max_edge, min_vertices, view, 1)[0]

    @staticmethod
    def _smooth_args(max_edge, iterations, lam, mu, fix_boundary, normals):
        flags = (SL3D_SMOOTH_FIX_BOUNDARY if fix_boundary else 0) | (SL3D_SMOOTH_NORMALS if normals else 0)
        return float(max_edge), int(iterations), float(lam), float(mu), flags

    def mesh_smoothed_device(self, max_edge, first_view=0, n_views=1, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, normals=False):
        """sl3d_mesh_smooth: the smoothed vertices (and normals) of the meshes of a batch of views left in HBM; returns (MeshSmoothed,
        vertex counts)."""
        m = MeshSmoothed()
        args = self._smooth_args(max_edge, iterations, lam, mu, fix_boundary, normals)
        return (m, *self._counts("sl3d_mesh_smooth", 1, first_view, n_views, *args, C.byref(m)))

    def meshes_smoothed(self, max_edge, first_view=0, n_views=1, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, normals=False):
        """The vertices of meshes(max_edge, first_view, n_views) after `iterations` Taubin iterations over the 1-ring (one step with lam,
        one with mu; mu = 0: plain Laplacian smoothing): a list of (n_k, 3) float32 arrays, or of (vertices, normals) pairs with
        normals=True -- the normals of the smoothed mesh.  Faces and vertex ids are those of meshes(); fix_boundary keeps the vertices of
        edges with one face where they are (include/sl3d.h: the exact definition)."""
        args = self._smooth_args(max_edge, iterations, lam, mu, fix_boundary, normals)
        (xyz, nrm), _ = self._fill_views("sl3d_get_mesh_smoothed", first_view, n_views, args, [_XYZ, _XYZ if normals else None], n_counts=1)
        return list(zip(xyz, nrm)) if normals else xyz

    def mesh_smoothed(self, max_edge, view=0, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, normals=False):
        """(n, 3) float32 smoothed vertices of mesh(max_edge, view), or (vertices, normals) with normals=True (meshes_smoothed)."""
        return self.meshes_smoothed(max_edge, view, 1, iterations, lam, mu, fix_boundary, normals)[0]

    @staticmethod
    def _lod_args(step, max_edge, min_vertices, lod_edge, mean, normals):
        flags = (SL3D_LOD_MEAN if mean else 0) | (SL3D_LOD_NORMALS if normals else 0)
        return int(step), float(max_edge), int(min_vertices), float(lod_edge), flags

    def mesh_lod_device(self, step, lod_edge, first_view=0, n_views=1, max_edge=float("inf"), min_vertices=1, mean=False, normals=False):
        """sl3d_mesh_views_lod: the level-of-detail meshes of a batch of views left in HBM; returns (MeshLod, vertex counts, face
        counts)."""
        m = MeshLod()
        args = self._lod_args(step, max_edge, min_vertices, lod_edge, mean, normals)
        return (m, *self._counts("sl3d_mesh_views_lod", 2, first_view, n_views, *args, C.byref(m)))

    def meshes_lod(self, step, lod_edge, first_view=0, n_views=1, max_edge=float("inf"), min_vertices=1, mean=False, normals=False):
        """One vertex per step x step pixel block of every view, meshed over the coarse grid with the cell rules of meshes() and
        lod_edge as the edge bar: a list of (xyz float32 (n, 3), faces int32 (m, 3), vertex_ids int32 (n,)), with normals=True of
        (xyz, faces, vertex_ids, normals).  A block's vertex is the candidate nearest its centre -- the candidates: the vertices of
        meshes_filtered(max_edge, min_vertices), all valid pixels for min_vertices = 1 --, with mean=True the mean of the block's
        candidates within lod_edge of it.  vertex_ids[i] is the id the representative has in cloud() / mesh(): cloud_rgb()[1][vertex_ids]
        and mesh_smoothed(...)[vertex_ids] are the colours and the smoothed positions (include/sl3d.h: the exact definition)."""
        args = self._lod_args(step, max_edge, min_vertices, lod_edge, mean, normals)
        (xyz, ids, nrm), (faces,), _ = self._fill_views("sl3d_get_meshes_lod", first_view, n_views, args,
                                                        [_XYZ, _IDS, _XYZ if normals else None], [_TRI], n_counts=2)
        return list(zip(xyz, faces, ids, *([nrm] if normals else [])))

    def mesh_lod(self, step, lod_edge, view=0, max_edge=float("inf"), min_vertices=1, mean=False, normals=False):
        """(xyz, faces, vertex_ids) of one view, with normals=True (xyz, faces, vertex_ids, normals) (meshes_lod)."""
        return self.meshes_lod(step, lod_edge, view, 1, max_edge, min_vertices, mean, normals)[0]

    @staticmethod
    def _fill_args(max_edge, min_vertices, max_hole, fill_edge, normals):
        return float(max_edge), int(min_vertices), int(max_hole), float(fill_edge), SL3D_FILL_NORMALS if normals else 0

    def mesh_fill_holes_device(self, max_hole, fill_edge, first_view=0, n_views=1, max_edge=float("inf"), min_vertices=1, normals=False):
        """sl3d_mesh_fill_holes: the hole-filled meshes of a batch of views left in HBM; returns (MeshHoles, vertex counts, face
        counts, hole counts, filled-pixel counts)."""
        m = MeshHoles()
        args = self._fill_args(max_edge, min_vertices, max_hole, fill_edge, normals)
        return (m, *self._counts("sl3d_mesh_fill_holes", 4, first_view, n_views, *args, C.byref(m)))

    def meshes_fill_holes(self, max_hole, fill_edge, first_view=0, n_views=1, max_edge=float("inf"), min_vertices=1, normals=False, stats=False):
        """The meshes of every view with their small interior holes filled: a list of (xyz float32 (n, 3), faces int32 (m, 3),
        vertex_ids int32 (n,)), with normals=True of (xyz, faces, vertex_ids, normals); with stats=True every tuple ends in
        (n_holes, n_filled).  A hole is a 4-connected component of at most max_hole non-candidate pixels that touches no border of the
        window -- the candidates: the vertices of meshes_filtered(max_edge, min_vertices), all valid pixels for min_vertices = 1.  A hole
        pixel is interpolated between the nearest candidates of its row and of its column; a span whose mean sample spacing exceeds
        fill_edge is not used, so a depth step is not bridged.  vertex_ids[i] is the id the vertex has in cloud() / mesh(), -1 for a
        filled vertex (include/sl3d.h: the exact definition)."""
        args = self._fill_args(max_edge, min_vertices, max_hole, fill_edge, normals)
        (xyz, ids, nrm), (faces,), (_, _, nh, nfl) = self._fill_views("sl3d_get_meshes_holes_filled", first_view, n_views, args,
                                                                      [_XYZ, _IDS, _XYZ if normals else None], [_TRI], n_counts=4)
        out = [xyz, faces, ids] + ([nrm] if normals else [])
        if stats:
            out.append([(int(a), int(b)) for a, b in zip(nh, nfl)])
        return list(zip(*out))

    def mesh_fill_holes(self, max_hole, fill_edge, view=0, max_edge=float("inf"), min_vertices=1, normals=False, stats=False):
        """(xyz, faces, vertex_ids) of one view, with normals=True (xyz, faces, vertex_ids, normals), with stats=True followed by
        (n_holes, n_filled) (meshes_fill_holes)."""
        return self.meshes_fill_holes(max_hole, fill_edge, view, 1, max_edge, min_vertices, normals, stats)[0]

    def set_texture(self, bgr, view=0):
        """The colour image save_point_cloud() takes r,g,b from: (H, W, 3) uint8, B,G,R order (cvLoadImage)."""
        t = np.ascontiguousarray(bgr, dtype=np.uint8)
        assert t.shape == (self.H, self.W, 3), t.shape
        self._chk(self.L.sl3d_set_texture(self._h, view, t.ctypes.data, t.strides[0]), "sl3d_set_texture")

    def cloud_rgb(self, view=0):
        """(n,3) float32 xyz and (n,3) uint8 r,g,b of the valid pixels in the reference's scan order."""
        return tuple(self._fill("sl3d_get_cloud_rgb", (view,), _XYZ, _RGB))

    def register_views(self, first_view, n_views, tx, ty, tz, rot_step):
        """register_point_clouds(): rotate view k by k*rot_step degrees about Y through (tx,ty,tz), concatenate."""
        return self._fill("sl3d_register_views", (first_view, n_views, tx, ty, tz, rot_step), _XYZ)[0]

    def align_camera(self):
        """sl3d_get_align_camera: float64[26] = Rc (9), tc (3), Kc (9), dc (5) exactly as a correspondence pass uses them."""
        cam = np.empty(26)
        self._chk(self.L.sl3d_get_align_camera(self._h, cam.ctypes.data), "sl3d_get_align_camera")
        return cam

    def align_sums(self, first_view, n_views, est, ox, oz, range, max_dist, window=2):
        """sl3d_align_sums: one correspondence pass between the consecutive views first_view .. first_view + n_views - 1 (pair j: source
        view first_view + j + 1, target first_view + j) at the estimate est = (c, s, tx, tz) -- cosine and sine of the step, the axis
        point -- quantised about (ox, oz) (the rule: include/sl3d_align.h).  Returns the (n_views - 1, 12) int64 words."""
        e = np.ascontiguousarray(est, dtype=np.float64).reshape(4)
        out = np.zeros((max(n_views - 1, 1), ALIGN_WORDS), dtype=np.int64)
        self._chk(self.L.sl3d_align_sums(self._h, first_view, n_views, e.ctypes.data, ox, oz, range, max_dist, window, out.ctypes.data), "sl3d_align_sums")
        return out[:n_views - 1]

    def _refine(self, symbol, iterations, *args):
        """a refinement (`symbol`, args its arguments between the context and the outputs): the dict refine_turntable documents"""
        out, done = Turntable(), C.c_int(0)
        log = (AlignIteration * max(iterations, 1))()
        self._chk(getattr(self.L, symbol)(self._h, *args, C.byref(out), log, C.byref(done)), symbol)
        return dict(tx=np.float32(out.tx), ty=np.float32(out.ty), tz=np.float32(out.tz), rot_step=np.float32(out.rot_step),
                    est=np.array(out.est[:], dtype=np.float64), n=int(out.n), sources=int(out.sources), rms_xz=float(out.rms_xz), rms_y=float(out.rms_y),
                    degenerate=bool(out.degenerate), n_done=done.value,
                    log=[dict(est=np.array(e.est[:], dtype=np.float64), n=int(e.n), sources=int(e.sources), rms_xz=float(e.rms_xz), rms_y=float(e.rms_y))
                         for e in log[:done.value]])

    def refine_turntable(self, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, window=2, iterations=20):
        """sl3d_refine_turntable: the axis point and the step of register_views / register_clouds refined from the views' own overlap,
        from the rough (tx, ty, tz, rot_step): up to `iterations` rounds of pass and solve.  Returns a dict: tx, ty, tz, rot_step (float32
        values, ready for register_views), est (c, s, tx, tz in float64), n, sources, rms_xz, rms_y of the last pass, degenerate, n_done
        and log -- per iteration made a dict(est, n, sources, rms_xz, rms_y) with the estimate its pass used."""
        return self._refine("sl3d_refine_turntable", iterations, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, window, iterations)

    def align_normals(self, first_view, n_views, normal_edge):
        """sl3d_align_normals: the dense normals of the views first_view .. first_view + n_views - 1 from each pixel's four neighbours
        within normal_edge (the rule: include/sl3d_align_plane.h); asynchronous."""
        self._chk(self.L.sl3d_align_normals(self._h, first_view, n_views, normal_edge), "sl3d_align_normals")

    def align_normal_plane(self, view):
        """sl3d_get_align_normals: (H, W, 3) float32, NaN where a pixel has no normal."""
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        self._chk(self.L.sl3d_get_align_normals(self._h, view, out.ctypes.data, out.strides[0]), "sl3d_get_align_normals")
        return out

    def align_plane_sums(self, first_view, n_views, est, ox, oz, range, max_dist, normal_edge, window=2):
        """sl3d_align_plane_sums: the normals of the target views and one point-to-plane pass between the consecutive views (pairs and
        estimate as align_sums).  Returns the (n_views - 1, 18) int64 words: accepted pairs, the upper triangle of the moments of the
        five fixed-point features, sources, sources lost to a missing normal."""
        e = np.ascontiguousarray(est, dtype=np.float64).reshape(4)
        out = np.zeros((max(n_views - 1, 1), ALIGN_PLANE_WORDS), dtype=np.int64)
        self._chk(self.L.sl3d_align_plane_sums(self._h, first_view, n_views, e.ctypes.data, ox, oz, range, max_dist, normal_edge, window,
                                               out.ctypes.data), "sl3d_align_plane_sums")
        return out[:n_views - 1]

    def refine_turntable_plane(self, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, normal_edge, window=2, iterations=20):
        """sl3d_refine_turntable_plane: refine_turntable with the point-to-plane error metric -- the residual along the target's surface
        normal, normals from neighbours within normal_edge.  The dict of refine_turntable: rms_xz carries rms_plane, rms_y is NaN."""
        return self._refine("sl3d_refine_turntable_plane", iterations, first_view, n_views, tx, ty, tz, rot_step, range, max_dist, normal_edge, window,
                            iterations)

    def voxel_grid_device(self, leaf, min_points=1, centroid=True, cloud=None):
        """sl3d_voxel_grid: one point per occupied cell of a grid of edge `leaf` over the registered cloud the last register_views /
        register_clouds left on the device, or over `cloud` ((n, 3) float32 on the host), left in HBM; returns (Voxels, [points in, points
        dropped, occupied cells, cells kept])."""
        a = None if cloud is None else np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        v, counts = Voxels(), (C.c_int64 * 4)()
        self._chk(self.L.sl3d_voxel_grid(self._h, None if a is None else a.ctypes.data, 0 if a is None else len(a), leaf, int(min_points),
                                         VOXEL_CENTROID if centroid else VOXEL_FIRST, C.byref(v), counts), "sl3d_voxel_grid")
        return v, [int(c) for c in counts]

    def voxel_grid(self, leaf, min_points=1, centroid=True, cloud=None, stats=False):
        """The voxel grid of voxel_grid_device on the host: (xyz float32 (m, 3), first int32 (m,), count uint32 (m,)) of the cells that
        hold at least min_points points, in order of first appearance -- xyz the cell's centroid (centroid=False: its first point), first
        the index of its first point in the cloud (colours, normals, the source view are gathered through it), count its points (the rule:
        include/sl3d_voxel.h).  stats=True appends [points in, points dropped, occupied cells, cells kept]."""
        _, counts = self.voxel_grid_device(leaf, min_points, centroid, cloud)
        out = tuple(self._fill("sl3d_get_voxel_grid", (), _XYZ, _IDS, _CNT))
        return out + (counts,) if stats else out

    def tsdf_reset(self, origin, voxel, trunc, dims):
        """sl3d_tsdf_reset: defines the TSDF volume -- origin (3 floats), the voxel edge, the truncation distance, dims (nx, ny, nz) -- and
        clears it (the rule: include/sl3d_tsdf.h); asynchronous."""
        v = TsdfVolume((C.c_float * 3)(*[float(o) for o in origin]), voxel, trunc, (C.c_int32 * 3)(*[int(d) for d in dims]))
        self._chk(self.L.sl3d_tsdf_reset(self._h, C.byref(v)), "sl3d_tsdf_reset")
        self._tsdf_dims = tuple(int(d) for d in dims)

    def tsdf_integrate(self, first_view, n_views, est, first_step=0):
        """sl3d_tsdf_integrate: the views first_view .. first_view + n_views - 1 of the dense result, the turntable indices first_step ..,
        voted into the volume at the estimate est = (c, s, tx, tz) (refine_turntable's "est").  Returns [samples taken, voxels with
        weight > 0]."""
        e = np.ascontiguousarray(est, dtype=np.float64).reshape(4)
        counts = (C.c_int64 * 2)()
        self._chk(self.L.sl3d_tsdf_integrate(self._h, first_view, n_views, first_step, e.ctypes.data, counts), "sl3d_tsdf_integrate")
        return [int(c) for c in counts]

    def tsdf_extract_device(self, min_weight=1):
        """sl3d_tsdf_extract: the oriented points of the zero level over the voxels of weight >= min_weight, left in HBM; returns
        (TsdfSurface, [voxels, known voxels, crossings])."""
        out, counts = TsdfSurface(), (C.c_int64 * 3)()
        self._chk(self.L.sl3d_tsdf_extract(self._h, int(min_weight), C.byref(out), counts), "sl3d_tsdf_extract")
        return out, [int(c) for c in counts]

    def tsdf_extract(self, min_weight=1, stats=False):
        """The surface of tsdf_extract_device on the host: (xyz float32 (m, 3), normals float32 (m, 3), edge int32 (m,)), edge = 3 * v0 +
        axis of the crossing's edge -- weights are gathered through it.  stats=True appends [voxels, known voxels, crossings]."""
        _, counts = self.tsdf_extract_device(min_weight)
        out = tuple(self._fill("sl3d_get_tsdf_surface", (), _XYZ, _XYZ, _IDS))
        return out + (counts,) if stats else out

    def tsdf_volume(self):
        """sl3d_get_tsdf: (sum int32, weight uint32), each shaped (nz, ny, nx)."""
        s, w = self._fill("sl3d_get_tsdf", (), (np.int32,), (np.uint32,))
        nx, ny, nz = self._tsdf_dims
        return s.reshape(nz, ny, nx), w.reshape(nz, ny, nx)

    def pinned(self, shape, dtype):
        """numpy array in pinned host memory (sl3d_host_alloc); freed when the Scanner is closed."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.L.sl3d_host_alloc(n)
        if not p:
            raise Sl3dError("sl3d_host_alloc failed")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return np.frombuffer((C.c_char * n).from_address(p), dtype=dtype).reshape(shape)

    def process_views(self, frames, xyz=None, valid=None):
        """frames: (n_views, planes_per_view, H, W) uint8 host array (pinned for full overlap), or per view a list of planes_per_view
        planes with None for a plane the context does not read (direct_gray: the inverse Gray planes); returns (xyz, valid)."""
        return self._process_views(frames, xyz, valid)

    def undistort(self, image, K, dist):
        """cvUndistort2 on an (H, W) or (H, W, 3) uint8 image (any size), on the device."""
        a = np.ascontiguousarray(image, dtype=np.uint8)
        cn = 1 if a.ndim == 2 else a.shape[2]
        out = np.empty_like(a)
        Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).ravel())
        dd = np.ascontiguousarray(np.asarray(dist, dtype=np.float64).ravel())
        self._chk(self.L.sl3d_undistort(self._h, a.ctypes.data, a.strides[0], a.shape[1], a.shape[0], cn, Kd.ctypes.data, dd.ctypes.data,
                                        out.ctypes.data, out.strides[0]), "sl3d_undistort")
        return out

    def generate_pattern(self, kind, axis, index):
        """One projector pattern of generate_pattern() (1/pattern_generator.cpp): (proj_height, proj_width) uint8."""
        out = np.empty((self.cfg.proj_height, self.cfg.proj_width), dtype=np.uint8)
        self._chk(self.L.sl3d_generate_pattern(self._h, kind, axis, index, out.ctypes.data, out.strides[0], None, None), "sl3d_generate_pattern")
        return out

    def transform_cloud(self, xyz, theta_deg, tx, ty, tz):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(a)
        self._chk(self.L.sl3d_transform_cloud(self._h, a.ctypes.data, len(a), theta_deg, tx, ty, tz, out.ctypes.data), "sl3d_transform_cloud")
        return out

    def device_buffers(self):
        b = DeviceBuffers()
        self._chk(self.L.sl3d_get_device_buffers(self._h, C.byref(b)), "sl3d_get_device_buffers")
        return b


class Group(_Handle):
    """sl3d_group_*: n row stripes of one frame window, stripe i on HIP device devices[i], assembled on stripe 0's GPU
    (RCCL send/recv between GPUs, device copies inside one)."""
    _prefix = "sl3d_group_"

    def __init__(self, width, height, proj_width, proj_height, n_gray_v, n_gray_h, fringe_width_v, fringe_width_h, devices,
                 n_fringe=3, max_views=1, full_size=None, origin=(0, 0), flags=0):
        self.L = load_library()
        fw, fh = full_size if full_size else (width, height)
        self.cfg = Config(width, height, fw, fh, origin[0], origin[1], proj_width, proj_height, n_fringe,
                          n_gray_v, n_gray_h, fringe_width_v, fringe_width_h, 0, 0, max_views, 0, flags, None)
        self.W, self.H = width, height
        devs = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        rc = self.L.sl3d_group_create(C.byref(self.cfg), devs, len(devices), C.byref(self._h))
        if rc != 0:
            raise Sl3dError(f"sl3d_group_create: {self.L.sl3d_strerror(rc).decode()}: {self.L.sl3d_group_last_error(None).decode()}")

    @property
    def transport(self):
        return self.L.sl3d_group_transport(self._h).decode()

    def stripes(self):
        """[(row0, rows, device, ctx handle)] of every stripe."""
        out = []
        for k in range(self.L.sl3d_group_size(self._h)):
            r0, n, d, h = C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
            self._chk(self.L.sl3d_group_stripe(self._h, k, C.byref(r0), C.byref(n), C.byref(d), C.byref(h)), "sl3d_group_stripe")
            out.append((r0.value, n.value, d.value, h))
        return out

    def run(self, first_view=0, n_views=1):
        self._chk(self.L.sl3d_group_run(self._h, first_view, n_views), "sl3d_group_run")

    def gather(self, first_view=0, n_views=1):
        self._chk(self.L.sl3d_group_gather(self._h, first_view, n_views), "sl3d_group_gather")

    def download_points(self, first_view=0, n_views=1, xyz=None, valid=None):
        """Every stripe's rows straight into the caller's dense host images (no gather to the root): (n, H, W, 3) f32, (n, H, W) u8."""
        if xyz is None:
            xyz = np.empty((n_views, self.H, self.W, 3), dtype=np.float32)
        if valid is None:
            valid = np.empty((n_views, self.H, self.W), dtype=np.uint8)
        assert xyz.shape == (n_views, self.H, self.W, 3) and valid.shape == (n_views, self.H, self.W)
        self._chk(self.L.sl3d_group_download_points(self._h, first_view, n_views, xyz.ctypes.data, valid.ctypes.data), "sl3d_group_download_points")
        return xyz, valid

    def process_views(self, frames, xyz=None, valid=None):
        """frames: (n_views, planes_per_view, H, W) uint8 host array (pinned for concurrent DMA); returns (xyz, valid) dense images."""
        return self._process_views(frames, xyz, valid)

    def run_clouds(self, first_view=0, n_views=1):
        self._chk(self.L.sl3d_group_run_clouds(self._h, first_view, n_views), "sl3d_group_run_clouds")

    def gather_clouds(self, first_view=0, n_views=1):
        return self._counts("sl3d_group_gather_clouds", 1, first_view, n_views)[0]

    def synchronize(self):
        self._chk(self.L.sl3d_group_synchronize(self._h), "sl3d_group_synchronize")
