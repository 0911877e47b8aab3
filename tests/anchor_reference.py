"""The anchored projector coordinate of SL3D_FLAG_ANCHOR_PERIODS (include/sl3d.h) restated in NumPy, float64, written from the
definition alone (shared by tests/test_anchor_arith.py and tests/test_gpu_anchor.py).  Per axis of a pixel, in this order:

    P2 = (2.0 * 22.0) / 7.0      TWOPI = 2.0 * 3.141592653589793      INV = 0.15915494309189535
    c_F = 0.0 (3 steps), 0.75 * (3.141592653589793 - 22.0 / 7.0) (4 steps)
    a  = (double)w + c_F                               w: the float stage 4 leaves in the wrapped-phase plane (Pi added), code: its int
    m  = rint((((double)code + 0.5) * P2 - a) * INV)   round half to even (np.rint)
    xs = (double)fw * ((a + TWOPI * m) / P2)

where stage 4's loop runs (frame columns 1..fullW-2 on the vertical axis, frame rows 1..fullH-2 on the horizontal one) on an axis with
Gray planes; elsewhere the coordinate stays (double)fw * ((double)unwrapped / P2).  NumPy evaluates each operation as one IEEE double
operation, none fused, which is what the definition asks of every route."""
import numpy as np

P2 = (2.0 * 22.0) / 7.0
TWOPI = 2.0 * 3.141592653589793
INV = 0.15915494309189535


def phase_offset(n_fringe):
    return 0.75 * (3.141592653589793 - 22.0 / 7.0) if n_fringe == 4 else 0.0


def period(w, code, n_fringe=3, offset=None):
    """m: the fringe period nearest the centre of Gray cell `code` (float64, integral)."""
    a = w.astype(np.float64) + (phase_offset(n_fringe) if offset is None else offset)
    return np.rint(((code.astype(np.float64) + 0.5) * P2 - a) * INV)


def coordinate(w, code, fw, n_fringe=3, offset=None):
    """xs of the formula, element by element.  offset: c_F, if not the definition's (the test of the 4-step constant)."""
    assert w.dtype == np.float32 and code.dtype.kind == "i"
    a = w.astype(np.float64) + (phase_offset(n_fringe) if offset is None else offset)
    m = np.rint(((code.astype(np.float64) + 0.5) * P2 - a) * INV)
    return np.float64(fw) * ((a + TWOPI * m) / P2)


def applies(axis, shape, origin, full, n_gray):
    """(H, W) bool: the pixels of a window of `shape` (H, W) at `origin` (col0, row0) of a frame `full` (W, H) where the formula applies."""
    H, W = shape
    if n_gray <= 0:
        return np.zeros((H, W), bool)
    if axis == 0:
        g = origin[0] + np.arange(W)
        return np.broadcast_to(((g >= 1) & (g <= full[0] - 2))[None, :], (H, W)).copy()
    g = origin[1] + np.arange(H)
    return np.broadcast_to(((g >= 1) & (g <= full[1] - 2))[:, None], (H, W)).copy()


def correspondences(w, code, unw, valid_axis, fw, n_fringe, n_gray, origin, full):
    """(H, W, 2) float64 (xs, ys) of an anchored context; NaN where either per-axis valid byte is not 1.  w, code, unw, valid_axis, fw,
    n_gray: pairs (vertical, horizontal) of the planes stage 4 leaves and of the configuration."""
    out = []
    for axis in (0, 1):
        assert unw[axis].dtype == np.float32
        plain = np.float64(fw[axis]) * (unw[axis].astype(np.float64) / P2)
        where = applies(axis, unw[axis].shape, origin, full, n_gray[axis])
        with np.errstate(invalid="ignore", over="ignore"):
            anchored = coordinate(w[axis], code[axis].astype(np.int64), fw[axis], n_fringe)
        out.append(np.where(where, anchored, plain))
    xy = np.stack(out, axis=-1)
    xy[~((valid_axis[0] == 1) & (valid_axis[1] == 1))] = np.nan
    return xy
