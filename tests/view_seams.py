"""The inputs of the view-seam tests (tests/test_view_seam_cases.py on the CPU, tests/test_gpu_view_seams.py on the device): NumPy only.

A context stacks the planes of its views without a gap, so for a kernel that walks a vertical neighbourhood of view v "row -1" is the
last row of view v - 1 and "row H" the first row of view v + 1: finite, valid data inside the allocation.  The builders here put into
those two rows exactly what a reader that forgot the row clip would like best, and the `extended_*` functions give a view as such a
reader sees it, so that the restatements (tests/align_reference.py, tests/align_plane_reference.py, tests/tsdf_reference.py) can say
what it would compute.

seam_views(cam, W, H, col0, row0, V, seed, est_pass) -> points, valid, pads, marks       (the two correspondence passes)
extended_target(points, valid, j, side) -> tp, tv, row0 shift;  extended_plane(planes, j, side) -> the same for any per-view plane
seam_surfaces(cam, W, H, col0, row0, V) -> points, valid, est, pads                      (the normals, the TSDF volume)
extended_views(points, valid, side) -> points, valid, row0 shift                          (every view with its neighbour's row)
seam_volume(points) -> vol"""
import numpy as np

import align_reference as AR

F8 = np.float64
EST_OFFSET = np.array([0.0, 0.0, 0.05, -0.03])                              # a pass runs at another estimate than the one that made the views
STEP_DEG = 0.2
CENTRE_SOURCES = 3                                                          # per pair and side
OFF_SURFACE = 12.0                                                          # mm off the surface along the ray: beyond max_dist of every real point
NORMAL_EDGE = 32.0                                                          # above (H + 1) pixel footprints of every shape the tests use
SIDES = ("above", "below")


def made_estimate(cam, step_deg=STEP_DEG):
    """the estimate align_reference.crafted_views makes its views with"""
    axis = AR.to_world(cam, np.array([2.0, 0.0, 104.0]))
    return AR.estimate(step_deg, float(axis[0]), float(axis[2]))


def pass_estimate(cam):
    return made_estimate(cam) + EST_OFFSET


def halves(W):
    """the columns that take the poison below (and the sources of row H) and those that take the poison above: disjoint"""
    assert W >= 2
    return np.arange(0, (W + 1) // 2), np.arange((W + 1) // 2, W)


def _few(cols):
    """up to CENTRE_SOURCES columns spread over `cols`, at most half of them (but one): the other sources of the half stay real"""
    n = min(CENTRE_SOURCES, max(1, len(cols) // 2))
    return cols[np.unique(np.linspace(0, len(cols) - 1, n).astype(int))]


def _surface_depth(c, r, col0, row0):
    return 100.0 + 3.0 * np.sin(0.3 * (c + col0)) + 2.0 * np.cos(0.4 * (r + row0))        # (crafted_views' own, continued past the frame)


def _landing(p, est_pass):
    """where the float32 source p lands under the pass's estimate, as the float32 a plane can hold"""
    return AR.turn(np.asarray(p, np.float32).astype(F8), est_pass).astype(np.float32)


def centre_source(cam, col0, row0, c, r, est_pass, off=OFF_SURFACE):
    """a source whose centre pixel under est_pass is exactly window pixel (c, r) -- r may be -1 or H -- `off` mm behind the surface, so
    that no real point of the target is within a pass's max_dist of it; None if the float32 point does not confirm the pixel"""
    P = AR.backproject(cam, 1, 1, col0 + c, row0 + r, _surface_depth(c, r, col0, row0) + off)[0, 0]
    p = AR.turn(P, est_pass, inverse=True).astype(np.float32)
    cc, rr, ok = AR.centre(AR.step(p[None], est_pass), cam, col0, row0)
    return p if bool(ok[0]) and (int(cc[0]), int(rr[0])) == (c, r) else None


def seam_views(cam, W, H, col0, row0, V, seed, est_pass):
    """align_reference.crafted_views with poison behind both seams of every pair j (target view j, source view j + 1) that has the
    neighbour:

    below, in the first row of view j + 1 (the target's row H), on the columns halves(W)[0]: the point turn(p, est_pass) of the source's
    own bottom-row pixel of that column under valid = 1 -- the very spot that source lands on, at distance 0;
    above (j >= 1), in the last row of view j - 1 (the target's row -1), on the columns halves(W)[1]: the same for the source's top-row
    pixel.

    A few bottom-row pixels of the source (columns of the first half) are first replaced by sources whose centre is exactly (c, H), a few
    top-row pixels (second half, j >= 1) by sources whose centre is exactly (c, -1) -- centre_source: far from every real point, behind
    the surface for even j and before it for odd j, since the target of pair j holds the like sources of pair j - 1 -- so that the
    rule above puts their landing points at (row H, c) and (row -1, c): a pass of window 0 without the row clip finds them, and a clipped
    pass of any window finds nothing for them.
    Rows that serve two pairs stay as built; what a row of one pair is built from is never a row another pair writes (the halves).

    Returns points (V, H, W, 3) float32, valid (V, H, W) uint8, pads (per view (H, 3) float32: the spot the row's last source lands on
    under est_pass, for the padding columns) and marks: per pair dict(below=[columns of the sources of row H], above=[.. of row -1])."""
    assert V >= 4 and H >= 2
    points, valid, _, crafted_pads = AR.crafted_views(cam, W, H, col0, row0, V, seed)
    lo, hi = halves(W)
    marks = []
    for j in range(V - 1):
        src = j + 1
        mark = dict(below=[], above=[])
        off = OFF_SURFACE if j % 2 == 0 else -OFF_SURFACE
        for c in _few(lo):
            p = centre_source(cam, col0, row0, int(c), H, est_pass, off)
            if p is not None:
                points[src][H - 1, c], valid[src][H - 1, c] = p, 1
                mark["below"].append(int(c))
        if j >= 1:
            for c in _few(hi):
                p = centre_source(cam, col0, row0, int(c), -1, est_pass, off)
                if p is not None:
                    points[src][0, c], valid[src][0, c] = p, 1
                    mark["above"].append(int(c))
        points[src][0, lo], valid[src][0, lo] = _landing(points[src][H - 1, lo], est_pass), 1
        if j >= 1:
            points[j - 1][H - 1, hi], valid[j - 1][H - 1, hi] = _landing(points[src][0, hi], est_pass), 1
        marks.append(mark)
    pads = [_landing(points[v + 1][:, W - 1], est_pass) for v in range(V - 1)] + [crafted_pads[V - 1]]
    return points, valid, pads, marks


def extended_plane(planes, j, side, fill=None):
    """view j of the stack `planes` (V, H, W, ..) as a reader without the row clip sees it: H + 1 rows, the last row of view j - 1 on top
    (side "above") or the first row of view j + 1 at the bottom ("below"); `fill` where there is no such view (None: there must be one)"""
    other, row = (j - 1, -1) if side == "above" else (j + 1, 0)
    assert side in SIDES and (fill is not None or 0 <= other < len(planes))
    extra = planes[other][row][None] if 0 <= other < len(planes) else np.full_like(planes[j][:1], fill)
    return np.concatenate([extra, planes[j]] if side == "above" else [planes[j], extra], axis=0)


def row_shift(side):
    """what to add to row0 for the extended view: its first row is window row -1 on the side "above" """
    return -1 if side == "above" else 0


def extended_target(points, valid, j, side):
    """the target of pair j with its neighbour's row: (tp (H + 1, W, 3), tv (H + 1, W), the shift of row0)"""
    return extended_plane(points, j, side), extended_plane(valid, j, side), row_shift(side)


def extended_views(points, valid, side):
    """every view with its neighbour's row, an invalid row of NaN where there is no neighbour: (V, H + 1, W, 3), (V, H + 1, W), shift"""
    V = len(points)
    return (np.stack([extended_plane(points, v, side, fill=np.nan) for v in range(V)]),
            np.stack([extended_plane(valid, v, side, fill=0) for v in range(V)]), row_shift(side))


def extended_both(points, valid, v):
    """view v (it has both neighbours) with both rows: H + 2 rows from window row -1 on"""
    return (np.concatenate([points[v - 1][-1:], points[v], points[v + 1][:1]], axis=0),
            np.concatenate([valid[v - 1][-1:], valid[v], valid[v + 1][:1]], axis=0))


def seam_surfaces(cam, W, H, col0, row0, V):
    """V smooth turntable views, every pixel valid: a gently waved surface (0.6 mm across the columns, 0.4 mm across the rows: flatter
    than crafted_views', so that the depths of any four pixels of neighbouring rows -- also of rows H + 1 pixels apart -- lie well within
    a truncation distance), each view the one before turned back by the step.  Then, from the views as first made, the first row of view
    v + 1 becomes the linear continuation 2 row[H - 1] - row[H - 2] of view v and the last row of view v - 1 the continuation
    2 row[0] - row[1] of view v (a one-row view continues as it is): who crosses a seam finds the surface going on.
    Returns points, valid, the estimate that made the views, pads (per view (H, 3): the row's last point again)."""
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = 100.0 + 0.6 * np.sin(0.3 * (c + col0)) + 0.4 * np.cos(0.4 * (r + row0))
    est = made_estimate(cam)
    made = [AR.backproject(cam, W, H, col0, row0, depth)]
    for _ in range(1, V):
        made.append(AR.turn(made[-1], est, inverse=True))
    points = np.stack(made).astype(np.float32)
    valid = np.ones((V, H, W), np.uint8)
    first = lambda m: 2.0 * m[0] - m[min(1, H - 1)]
    last = lambda m: 2.0 * m[H - 1] - m[max(H - 2, 0)]
    for v in range(V):
        if v + 1 < V:
            points[v + 1][0] = last(made[v]).astype(np.float32)
        if v >= 1:
            points[v - 1][H - 1] = first(made[v]).astype(np.float32)
    pads = [points[v][:, W - 1].copy() for v in range(V)]
    return points, valid, est, pads


VOXEL, TRUNC, REACH = np.float32(0.3), np.float32(1.5), 2.0


def seam_volume(points):
    """a volume about the box of the middle view's points, REACH mm wider on every side -- past the frame's top and bottom rows, whose
    continuations the view's own first and last row hold: voxels project to the cells fv = -1 and fv = H - 1 of every view, and past
    them.  The voxel is below a pixel's footprint, the truncation five voxels."""
    p = points[len(points) // 2].astype(F8).reshape(-1, 3)
    lo, hi = p.min(axis=0) - REACH, p.max(axis=0) + REACH
    dims = tuple(int(d) for d in np.ceil((hi - lo) / float(VOXEL)))
    return dict(origin=lo.astype(np.float32), voxel=VOXEL, trunc=TRUNC, dims=dims)
