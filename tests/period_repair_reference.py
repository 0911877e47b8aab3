"""NumPy restatement of sl3d_repair_periods (include/sl3d.h), applied literally: plain loops over the at most 17 values of a
neighbourhood, an insertion sort, np.rint in float64.  Nothing here is derived from the kernels or from 3dscan_amd/csrc/sl3d_period.h."""
import numpy as np

TWO_PI_REF = (2.0 * 22.0) / 7.0   # the divisor as stage 5 writes it


def samples(valid, axis):
    """Samples of an axis: valid byte 1 and inside the range where stage 4 defines the absolute phase (window coordinates)."""
    H, W = valid.shape
    s = np.zeros((H, W), dtype=bool)
    if axis == 0:
        s[:, 1:W - 1] = valid[:, 1:W - 1] == 1
    else:
        s[1:H - 1, :] = valid[1:H - 1, :] == 1
    return s


def _lower_median(vals):
    s = []
    for v in vals:            # insertion sort, ascending
        k = len(s)
        s.append(v)
        while k > 0 and s[k - 1] > v:
            s[k] = s[k - 1]
            k -= 1
        s[k] = v
    return s[(len(s) - 1) // 2]


def _line(code, wrapped, unw, smp, radius, n_gray, in_place):
    """One row (vertical axis) or column (horizontal axis): returns (code', unwrapped', repaired, unrepairable)."""
    L = len(unw)
    code_out, unw_out = code.copy(), unw.copy()
    src = unw_out if in_place else unw      # in_place: a sweep that sees its own repairs (NOT the definition; for the Jacobi test)
    rep = unrep = 0
    for p in range(L):
        if not smp[p]:
            continue
        S = [src[q] for q in range(max(0, p - radius), min(L - 1, p + radius) + 1) if smp[q]]
        if len(S) < radius + 1:
            continue
        m = _lower_median(S)
        j = int(np.rint((np.float64(src[p]) - np.float64(m)) / np.float64(TWO_PI_REF)))
        if j == 0:
            continue
        k = int(code[p]) - j
        if k < 0 or k >= (1 << n_gray):
            unrep += 1
            continue
        code_out[p] = k
        unw_out[p] = np.float32(np.float64(wrapped[p]) + ((np.float64(k) * 2.0) * 22.0) / 7.0)
        rep += 1
    return code_out, unw_out, rep, unrep


def repair_periods(code, wrapped, unwrapped, valid, axis, radius, n_gray, in_place=False):
    """One pass over one axis of one view.  code int32, wrapped / unwrapped float32, valid uint8, all [H][W] of the window, as stage 4
    left them.  Returns (code', unwrapped', repaired, unrepairable); the inputs are not modified."""
    assert 1 <= radius <= 8 and axis in (0, 1)
    assert code.dtype == np.int32 and wrapped.dtype == np.float32 and unwrapped.dtype == np.float32
    smp = samples(valid, axis)
    code_out, unw_out = code.copy(), unwrapped.copy()
    rep = unrep = 0
    H, W = valid.shape
    for i in range(H if axis == 0 else W):
        sl = np.s_[i, :] if axis == 0 else np.s_[:, i]
        c, u, a, b = _line(code[sl], wrapped[sl], unwrapped[sl], smp[sl], radius, n_gray, in_place)
        code_out[sl], unw_out[sl] = c, u
        rep += a
        unrep += b
    return code_out, unw_out, rep, unrep


def interior(valid, axis, radius):
    """The samples that have at least `radius` samples on each side within their run (a run: consecutive samples along the coded
    direction): where a shifted Gray edge must be repaired completely."""
    smp = samples(valid, axis)
    out = np.zeros_like(smp)
    H, W = valid.shape
    for i in range(H if axis == 0 else W):
        sl = np.s_[i, :] if axis == 0 else np.s_[:, i]
        line = smp[sl]
        res = np.zeros(len(line), dtype=bool)
        p = 0
        while p < len(line):
            if not line[p]:
                p += 1
                continue
            q = p
            while q < len(line) and line[q]:
                q += 1
            if q - p > 2 * radius:
                res[p + radius:q - radius] = True
            p = q
        out[sl] = res
    return out
