"""The Gray decode of SL3D_FLAG_DIRECT_GRAY (include/sl3d.h) restated in NumPy, int32, written from the comment above the flag
alone (shared by tests/test_direct_gray_arith.py and tests/test_gpu_direct_gray.py).  Per axis of a pixel, with gray_i the byte of Gray
plane i (most significant first) and I0, I2 fringe bytes 0 and 2 of the same axis of the same view:

    G_i  = (2 * gray_i - (I0 + I2) >= 0)              ties -> 1
    b_i  = b_(i-1) xor G_i,  b_(-1) = 0               4/phase_unwrap.cpp:187-191
    code = sum b_i 2^(N-1-i)                          :193

Everything behind the code is what it always was, and is taken from the restatements that exist: absolute() is the float stage 4 forms
from the shifted wrapped phase and the code; tests/subpixel_reference.py, tests/anchor_reference.py and tests/one_axis_reference.py take it
from there.  as_inverse_coded() turns a plane list into one whose Gray planes are the bits (0 / 255) and whose inverse planes are their
complements: ANY inverse-based decoder -- the oracle -- run on it decodes by the direct rule, stage planes, validity and points included."""
import numpy as np


def bits(gray, i0, i2):
    """[G_i] as (H, W) int32 arrays of 0 / 1, from the Gray planes and fringe planes 0 and 2 (uint8)."""
    s = i0.astype(np.int32) + i2.astype(np.int32)
    return [(2 * g.astype(np.int32) - s >= 0).astype(np.int32) for g in gray]


def code(gray, i0, i2):
    """stage 4's code on every pixel (int32; 0 without Gray planes)."""
    b = np.zeros(i0.shape, np.int32)
    c = np.zeros(i0.shape, np.int32)
    for g in bits(gray, i0, i2):
        b = b ^ g
        c = c * 2 + b
    return c


def inverse_code(gray, inv):
    """The same chain over the reference's own bit, (gray_i - inverse_i >= 0): what an unflagged context decodes."""
    assert len(gray) == len(inv) >= 1
    b = np.zeros(gray[0].shape, np.int32)
    c = np.zeros(gray[0].shape, np.int32)
    for g, n in zip(gray, inv):
        b = b ^ (g.astype(np.int32) - n.astype(np.int32) >= 0).astype(np.int32)
        c = c * 2 + b
    return c


def split(planes, n_fringe, n_gray):
    """(fringe, gray, inverse) of one axis's plane list; the inverse part may be missing."""
    return list(planes[:n_fringe]), list(planes[n_fringe:n_fringe + n_gray]), list(planes[n_fringe + n_gray:])


def code_of_planes(planes, n_fringe, n_gray):
    fr, gray, _ = split(planes, n_fringe, n_gray)
    return code(gray, fr[0], fr[2])


def read_planes(planes, n_fringe, n_gray):
    """The F + N planes of an axis such a context reads."""
    return list(planes[:n_fringe + n_gray])


def as_inverse_coded(planes, n_fringe, n_gray):
    """F + 2 N planes on which (gray_i - inverse_i >= 0) IS G_i: Gray plane i = 255 G_i, inverse plane i = 255 - that."""
    fr, gray, _ = split(planes, n_fringe, n_gray)
    g = [(255 * b).astype(np.uint8) for b in bits(gray, fr[0], fr[2])]
    return fr + g + [(255 - p).astype(np.uint8) for p in g]


def absolute(w, code_plane):
    """The absolute phase stage 4 forms from the shifted wrapped phase (float32) and the code: (float)(w + code * 2 * 22 / 7) in double."""
    assert w.dtype == np.float32
    return (w.astype(np.float64) + ((code_plane.astype(np.float64) * 2.0) * 22.0) / 7.0).astype(np.float32)
