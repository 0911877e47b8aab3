"""NumPy restatement of the exposure fusion (sl3d_fuse_exposures; the rule as include/sl3d_fuse.h states it), written as the lexicographic rule
-- fewest clipped planes, then the largest score, then the smallest exposure index -- and not through the packed key the kernel takes the
maximum of; and the three-band scene the tests fuse: a capture whose window columns are cut into three bands of reflectance 1, 1/4, 1/16,
seen at the gains 0.8, 3.2 and 12.8.

Shared by tests/test_exposure_arith.py (CPU) and tests/test_gpu_exposure.py."""
import numpy as np

ONLY_VERTICAL, ONLY_HORIZONTAL, DIRECT_GRAY = 1024, 2048, 4096      # SL3D_FLAG_* of include/sl3d.h
GAINS = (0.8, 3.2, 12.8)
RHO = (1.0, 0.25, 0.0625)


def coded_axes(flags):
    return (0,) if flags & ONLY_VERTICAL else (1,) if flags & ONLY_HORIZONTAL else (0, 1)


def axis_base(F, N_v, axis):
    """first plane of an axis in planes_per_view: fringe[0..F), gray[0..N), inverse[0..N) of the vertical axis, then of the horizontal"""
    return 0 if axis == 0 else F + 2 * N_v


def planes_in_use(F, N_v, N_h, flags):
    """indices (into planes_per_view) of the planes the fusion reads and writes"""
    out = []
    for a in coded_axes(flags):
        N = (N_v, N_h)[a]
        out += list(range(axis_base(F, N_v, a), axis_base(F, N_v, a) + F + (N if flags & DIRECT_GRAY else 2 * N)))
    return out


def score(F, fringe):
    """S of one axis: fringe [F][...] integer planes"""
    i = [f.astype(np.int64) for f in fringe]
    t1, t2 = (i[3] - i[1], i[0] - i[2]) if F == 4 else (i[0] - i[2], 2 * i[1] - i[0] - i[2])
    return t1 * t1 + t2 * t2


def fuse(stack, F, N_v, N_h, flags, saturation):
    """stack: uint8 [E][planes_per_view][H][W].  Returns (fused [planes_per_view][H][W] -- the planes not in use are 0 --, map uint8 [H][W],
    counts uint32 [E + 1])."""
    E, ppv = stack.shape[:2]
    assert ppv == 2 * F + 2 * N_v + 2 * N_h and F in (3, 4) and 1 <= E <= 8 and 1 <= saturation <= 256
    use = planes_in_use(F, N_v, N_h, flags)
    n = (stack[:, use] >= saturation).sum(axis=1)                                     # [E][H][W]
    q = None
    for a in coded_axes(flags):
        b = axis_base(F, N_v, a)
        s = np.stack([score(F, stack[e, b:b + F]) for e in range(E)])
        q = s if q is None else np.minimum(q, s)
    cand = n == n.min(axis=0)                                                          # the fewest clipped planes
    cand &= q == np.where(cand, q, -1).max(axis=0)                                     # among those the largest score
    choice = np.argmax(cand, axis=0)                                                   # among those the smallest e
    clipped = np.take_along_axis(n, choice[None], axis=0)[0] > 0
    fused = np.zeros(stack.shape[1:], np.uint8)
    fused[use] = np.take_along_axis(stack[:, use], choice[None, None], axis=0)[0]
    counts = np.array([int((choice == e).sum()) for e in range(E)] + [int(clipped.sum())], np.uint32)
    return fused, (choice | np.where(clipped, 0x80, 0)).astype(np.uint8), counts


def capture_stack(cap):
    """the planes of a synth.make_capture as [planes_per_view][H][W]"""
    return np.stack(list(cap["planes_v"]) + list(cap["planes_h"]))


def three_band_scene(synth, W, H, PW, PH, N, fw, F, noise=0, **kw):
    """dict(stack [3][planes_per_view][H][W]: exposure e has gain GAINS[e]; base: the capture at gain 0.8; band [H][W]: the band index of a
    pixel; lit, mask, cal: the capture's).  Exposure e's frame in band b is the capture at gain GAINS[e] * RHO[b], offset 10, the same view and
    seed throughout: the scalings are powers of two, so the product is exactly 0.8 once per band, at e == b."""
    caps = {}
    for g in sorted({ge * r for ge in GAINS for r in RHO}):
        caps[g] = synth.make_capture(W, H, PW, PH, N, N, fw, fw, n_fringe=F, noise=noise, gain=g, offset=10.0, **kw)
    assert GAINS[1] * RHO[1] == 0.8 and GAINS[2] * RHO[2] == 0.8
    edges = [0, W // 3, 2 * W // 3, W]
    band = np.zeros((H, W), np.int64)
    stack = np.empty((3,) + capture_stack(caps[0.8]).shape, np.uint8)
    for b in range(3):
        cols = slice(edges[b], edges[b + 1])
        band[:, cols] = b
        for e in range(3):
            stack[e][:, :, cols] = capture_stack(caps[GAINS[e] * RHO[b]])[:, :, cols]
    c = caps[0.8]
    return dict(stack=stack, base=capture_stack(c), band=band, lit=c["lit"], mask=c["mask"], cal=c["cal"])
