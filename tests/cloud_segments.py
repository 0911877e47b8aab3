"""Write crafted segments -- counts and point slots -- into a context's segmented clouds, so that a GPU test controls the input of every
consumer of sl3d_run_clouds' output (k_seg_scan, k_seg_close and the host routes around them) instead of taking what k_fused<..., CMODE = 2>
wrote from a decode.  The counterpart of tests/dense_planes.py, whose byte copy it uses.

arm() launches sl3d_run_clouds over at most 4 views, which leaves every one of them Scan::PENDING (no k_seg_scan ran: whoever consumes the
view scans), and waits; put_segments() then replaces what the launch wrote.  The addresses come from Scanner.cloud_segments and nothing
else of the library: the buffers are allocated by the first run_clouds and stay where they are, so the layout is read once (that call
scans, hence arm() launches again behind it).

A view's n_segs = 4 * tiles can exceed its real segments (the s with 256 * s < pitch * H), and the consumers read a segment's slots wherever
its count says -- behind the last view that is past the allocation.  put_segments therefore asserts segment_cases.check_bounds on everything
it writes; no test may write counts another way."""
import numpy as np

import segment_cases as SC
from dense_planes import _copy_rows

SEG = SC.SEG


def segment_layout(sc, first_view, n_views):
    """addresses and strides of the segmented clouds of views [first_view, first_view + n_views), from Scanner.cloud_segments (which scans
    views that are pending: arm again behind it)"""
    seg, _ = sc.cloud_segments(first_view, n_views)
    pitch, px, n_segs, _ = SC.geometry(sc.W, sc.H)
    assert (seg.n_segments, seg.segment_points, seg.view_stride_points, seg.view_stride_segments) == (n_segs, SEG, px, n_segs)
    return dict(xyz=int(seg.xyz), counts=int(seg.counts), offsets=int(seg.offsets), n_segs=n_segs, stride_points=px, stride_segs=n_segs,
                first_view=first_view, n_views=n_views)


def _layout(sc):
    """the layout of all views, read once per context (behind a run_clouds: the buffers exist from the first one on)"""
    lay = getattr(sc, "_crafted_segment_layout", None)
    if lay is None:
        lay = sc._crafted_segment_layout = segment_layout(sc, 0, sc.cfg.max_views)
    return lay


def arm(sc, first_view, n_views):
    """run_clouds over at most 4 views -- every one Scan::PENDING afterwards -- then synchronize()"""
    assert 1 <= n_views <= 4 and 0 <= first_view and first_view + n_views <= sc.cfg.max_views
    sc.run_clouds(first_view, n_views)
    sc.synchronize()
    if getattr(sc, "_crafted_segment_layout", None) is None:
        _layout(sc)                                        # (scanned the views: launch again)
        sc.run_clouds(first_view, n_views)
        sc.synchronize()


def _address(sc, view):
    lay = _layout(sc)
    assert 0 <= view < lay["n_views"]
    return (lay["xyz"] + 12 * view * lay["stride_points"], lay["counts"] + 4 * view * lay["stride_segs"],
            lay["offsets"] + 8 * view * lay["stride_segs"])


def _put_bytes(address, arr):
    b = np.ascontiguousarray(arr).view(np.uint8).reshape(1, -1)
    _copy_rows(address, b.shape[1], 1, 0, b)


def put_segments(sc, view, counts, xyz=None, fill=None):
    """counts: uint32[n_segs] -> the view's segment counts; xyz: float32[n_segs * 256, 3] -> its point slots (the pitch * H slots the view
    owns: the rows behind them are not written); fill: a float32 value for every slot behind a count (needs xyz).  Bytes are copied as
    bytes.  Call it behind arm(): no launch is pending then."""
    W, H = sc.W, sc.H
    _, px, n_segs, _ = SC.geometry(W, H)
    counts = np.ascontiguousarray(counts)
    SC.check_bounds(W, H, counts)                        # (dtype, length, <= 256, <= pitch*H - 256*s, 0 behind the last real segment)
    a_xyz, a_counts, _ = _address(sc, view)
    if xyz is not None:
        xyz = np.ascontiguousarray(xyz)
        assert xyz.dtype == np.float32 and xyz.shape == (n_segs * SEG, 3), (xyz.dtype, xyz.shape)
        if fill is not None:
            xyz = SC.with_fill(W, H, counts, xyz, fill)
        _put_bytes(a_xyz, xyz[:px])
    else:
        assert fill is None, "fill goes into the slots that are written: pass xyz"
    _put_bytes(a_counts, counts)


def read_segments(sc, view, want_xyz=True):
    """(counts uint32[n_segs], offsets uint64[n_segs], slots float32[pitch * H, 3] or None) as they lie in the device now"""
    _, px, n_segs, _ = SC.geometry(sc.W, sc.H)
    a_xyz, a_counts, a_offsets = _address(sc, view)
    counts, offsets = np.empty(n_segs, np.uint32), np.empty(n_segs, np.uint64)
    sc._d2h(counts, a_counts)
    sc._d2h(offsets, a_offsets)
    xyz = None
    if want_xyz:
        xyz = np.empty((px, 3), np.float32)
        sc._d2h(xyz, a_xyz)
    return counts, offsets, xyz


def check_put(sc, view, counts, xyz=None, fill=None):
    """the helper's own test: the device holds exactly the bytes that were put"""
    _, px, _, _ = SC.geometry(sc.W, sc.H)
    got_counts, _, got_xyz = read_segments(sc, view, want_xyz=xyz is not None)
    assert np.array_equal(got_counts, counts)
    if xyz is not None:
        want = SC.with_fill(sc.W, sc.H, counts, xyz, fill) if fill is not None else np.ascontiguousarray(xyz)
        assert np.array_equal(got_xyz.view(np.uint32), want[:px].view(np.uint32))
