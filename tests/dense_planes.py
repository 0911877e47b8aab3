"""Write crafted arrays into a context's dense planes (points, valid), so that a GPU test controls the input of every kernel that reads
them -- the mesh, normal, component and smoothing kernels and the compaction -- instead of taking whatever a decode produces.

put_dense uses the addresses, pitches and view strides sl3d_get_device_buffers hands out (Scanner.device_buffers()) and nothing else of
the library.  Call it behind sc.run() and sc.synchronize(): then no launch is pending, and a mesh call reads what was put.  The bytes are
copied as bytes (integer views), so a NaN keeps its sign and payload.  The padding columns [W, pitch) are left alone unless pad_valid /
pad_xyz ask for a fill."""
import ctypes as C

import numpy as np

_HIP_H2D = 1  # hipMemcpyHostToDevice


class _Raw:
    """a device allocation the library owns, described for torch through __cuda_array_interface__"""

    def __init__(self, address, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(int(s) for s in shape), typestr=typestr, data=(int(address), False), version=2, strides=None)


def _loaded_hip():
    """the HIP runtime this process has loaded already (the one torch brought along), through ctypes"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime is loaded in this process"
    lib = C.CDLL(sorted(paths)[0])
    lib.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    lib.hipMemcpy2D.restype = C.c_int
    lib.hipDeviceSynchronize.restype = C.c_int
    return lib


def _copy_rows(address, pitch_bytes, rows, first_byte, src):
    """src: C-contiguous (rows, n) uint8 -> n bytes of every row of the pitched device plane at `address`, from byte `first_byte` of the row"""
    assert src.dtype == np.uint8 and src.ndim == 2 and src.shape[0] == rows and src.flags["C_CONTIGUOUS"]
    n = src.shape[1]
    if n == 0:
        return
    assert first_byte + n <= pitch_bytes
    try:
        import torch
        plane = torch.as_tensor(_Raw(address, (rows, pitch_bytes), "|u1"), device="cuda")
        assert plane.data_ptr() == address and plane.dtype == torch.uint8
    except Exception:                                     # this torch cannot wrap a foreign address: a pitched copy through the runtime it loaded
        hip = _loaded_hip()
        rc = hip.hipMemcpy2D(C.c_void_p(address + first_byte), pitch_bytes, C.c_void_p(src.ctypes.data), n, n, rows, _HIP_H2D)
        assert rc == 0, f"hipMemcpy2D: {rc}"
        assert hip.hipDeviceSynchronize() == 0
        return
    plane[:, first_byte:first_byte + n].copy_(torch.from_numpy(src))
    torch.cuda.synchronize()


def dense_layout(sc, view):
    """(points address, points pitch in bytes, valid address, valid pitch in bytes, pitch in pixels) of one view"""
    b = sc.device_buffers()
    assert 0 <= view < sc.cfg.max_views and b.points_pitch == 12 * b.valid_pitch and b.valid_pitch >= sc.W
    return b.points + view * b.points_view_stride, b.points_pitch, b.valid + view * b.valid_view_stride, b.valid_pitch, b.valid_pitch


def put_dense(sc, view, xyz, valid, pad_xyz=None, pad_valid=None):
    """xyz: (H, W, 3) float32, valid: (H, W) uint8 of 0/1 -> the dense planes of `view`.  pad_valid (0 or 1) / pad_xyz (a float32 value):
    the fill of the padding columns [W, pitch) of the valid / points plane."""
    H, W = sc.H, sc.W
    xyz, valid = np.ascontiguousarray(xyz), np.ascontiguousarray(valid)
    assert xyz.dtype == np.float32 and xyz.shape == (H, W, 3) and valid.dtype == np.uint8 and valid.shape == (H, W)
    assert valid.max(initial=0) <= 1
    p_addr, p_pitch, v_addr, v_pitch, pitch = dense_layout(sc, view)
    _copy_rows(p_addr, p_pitch, H, 0, xyz.view(np.uint8).reshape(H, 12 * W))
    _copy_rows(v_addr, v_pitch, H, 0, valid)
    if pad_xyz is not None:
        pad = np.full((H, pitch - W, 3), pad_xyz, np.float32)
        _copy_rows(p_addr, p_pitch, H, 12 * W, pad.view(np.uint8).reshape(H, 12 * (pitch - W)))
    if pad_valid is not None:
        assert pad_valid in (0, 1)
        _copy_rows(v_addr, v_pitch, H, W, np.full((H, pitch - W), pad_valid, np.uint8))


def check_put(sc, view, xyz, valid):
    """the helper's own test: points() returns exactly what was written, and the compacted cloud is xyz[valid == 1], payloads included"""
    got_xyz, got_valid = sc.points(view)
    assert np.array_equal(got_valid, valid)
    assert np.array_equal(got_xyz.view(np.uint32), np.ascontiguousarray(xyz).view(np.uint32))
    cloud, want = sc.cloud(view), np.ascontiguousarray(xyz[valid == 1])
    assert cloud.shape == want.shape and np.array_equal(cloud.view(np.uint32), want.view(np.uint32))
