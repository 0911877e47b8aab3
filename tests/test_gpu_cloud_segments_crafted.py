"""GPU tests (-m gpu) of the consumers of the segmented clouds on crafted segments (tests/segment_cases.py, written into a context by
tests/cloud_segments.py): k_seg_scan, the three k_seg_close forms (plain, SCAN, REG) and the host routes around them --
sl3d_get_cloud_counts, sl3d_get_cloud_segments, sl3d_download_clouds (pinned, pageable, SL3D_ZEROCOPY=0, clamped), sl3d_register_clouds --
with the per-view Scan::{PENDING, TOTAL_ONLY, DONE} state that decides which of them scans.  The other GPU suites feed these consumers only
what k_fused<..., CMODE = 2> wrote from a decode; here nobody but the test wrote the input, so a failure is the consumer's.
tests/test_segment_cases.py asserts, on the CPU, that the cases contain what they are built for.

The reference of every comparison is the NumPy restatement of the CRAFTED counts and slots (the long views: crafted counts over the slots as
the arming decode left them, downloaded once).  Everything is compared bit for bit, no tolerance; a copied NaN keeps its sign and payload.
The one exception: a NaN that the registration's arithmetic PRODUCES is compared as "a NaN", as in the mesh suite."""
import itertools
import os

import numpy as np
import pytest

import segment_cases as SC
from cloud_segments import arm, check_put, put_segments, read_segments
from conftest import pkg

pytestmark = pytest.mark.gpu

# the decode that only allocates and arms: 1 Gray plane per axis -- the fewest a context decodes -- over a 64 x 64 projector, fringe width 32
N_GRAY, FRINGE, PW, PH = 1, 32, 64, 64
UNTOUCHED = np.float32(-7.0)       # what a destination holds before a download: still there just past the points it received


def _context(shape, V, serial=False, masks=None):
    """a context of V synthetic views, decoded by nobody yet"""
    S, syn = pkg("scanner"), pkg("synth")
    W, H = shape
    sc = S.Scanner(W, H, PW, PH, N_GRAY, N_GRAY, FRINGE, FRINGE, max_views=V, serial_launches=serial)
    sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, PW, PH)))
    for v in range(V):
        sc.set_mask(syn.default_mask(W, H) if masks is None else masks[v], view=v)
        sc.synth_view(v, plane=(1.5 * v, 0.05, 0.04 - 0.005 * v), view_id=v, noise=0)
    return sc


class Expect:
    """one view's crafted input and what the restatement says about it"""

    def __init__(self, shape, name, counts, xyz, fill=SC.SENTINEL):
        self.name, self.counts = name, counts
        self.slots = SC.with_fill(*shape, counts, xyz, fill) if fill is not None else xyz      # as they lie in the device
        self.offsets, self.total, self.cloud = SC.restate(counts, self.slots)
        assert not SC.holds_sentinel(self.cloud)


def _same(got, want, tag, produced=False):
    n = SC.bits_differ(got, want, produced)
    assert n == 0, (tag, f"{n} of {want.size} values differ")
    assert not SC.holds_sentinel(got), (tag, "a slot behind a count reached an output")


def _packed(sc, ptr, stride, k, n):
    a = np.empty((n, 3), np.float32)
    if n:
        sc._d2h(a, ptr + 12 * k * stride)
    return a


class Consumers:
    """every consumer over crafted views [first, first + len(exp)) of one context, each against the restatement; `count` tallies comparisons"""

    def __init__(self, sc, shape, pin):
        self.sc, self.shape, self.pin = sc, shape, pin
        self.px = SC.geometry(*shape)[1]
        self.count = 0

    def put(self, first, exp, rearm=True):
        if rearm:
            arm(self.sc, first, len(exp))
        for k, e in enumerate(exp):
            put_segments(self.sc, first + k, e.counts, e.slots)

    def _into(self, view, e, out, capacity, tag):
        out[:3 * (min(capacity, e.total) + 1)] = UNTOUCHED
        n = self.sc.download_cloud_into(view, out[:3 * capacity])
        assert n == e.total, (tag, n, e.total)
        m = min(capacity, e.total)
        _same(out[:3 * m].reshape(m, 3), SC.clamped(e.cloud, capacity), tag)
        assert (out[3 * m:3 * m + 3] == UNTOUCHED).all(), (tag, "written past the points")
        self.count += 1

    def roomy(self, view, e):
        """one view into pinned memory with room for every slot: k_seg_close<SCAN> on a view that is not scanned, the offsets array otherwise"""
        self._into(view, e, self.pin, self.px, (e.name, "pinned roomy"))

    def clamped(self, view, e, capacity):
        self._into(view, e, self.pin, capacity, (e.name, "pinned clamped", capacity))

    def pageable(self, view, e):
        self._into(view, e, np.empty(3 * (self.px + 1), np.float32), self.px, (e.name, "pageable"))

    def counts(self, first, exp, device_copy):
        ptr, stride, got = self.sc.cloud_counts(first, len(exp), want_device_copy=device_copy)
        assert got == [e.total for e in exp], ("cloud_counts", device_copy, [e.name for e in exp])
        assert (ptr is not None) == device_copy
        for k, e in enumerate(exp):
            if device_copy:
                _same(_packed(self.sc, ptr, stride, k, e.total), e.cloud, (e.name, "contiguous device copy"))
            self.count += 1
        return ptr, stride

    def segments(self, first, exp):
        seg, got = self.sc.cloud_segments(first, len(exp))
        assert got == [e.total for e in exp], ("cloud_segments", [e.name for e in exp])
        for k, e in enumerate(exp):
            cnt, off, _ = read_segments(self.sc, first + k, want_xyz=False)
            assert np.array_equal(cnt, e.counts), (e.name, "counts changed")
            assert off.dtype == np.uint64 and np.array_equal(off, e.offsets), (e.name, "offsets")
            self.count += 1

    def download(self, first, exp, pinned, zerocopy=True):
        tag = ("download_clouds", "pinned" if pinned else "pageable", zerocopy)
        total = sum(e.total for e in exp)
        if pinned:
            self.pin[:3 * (total + 1)] = UNTOUCHED
        if not zerocopy:
            os.environ["SL3D_ZEROCOPY"] = "0"
        try:
            got = self.sc.download_clouds(first, len(exp), out=self.pin if pinned else None)
        finally:
            os.environ.pop("SL3D_ZEROCOPY", None)
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            _same(g, e.cloud, tag + (e.name,))
            self.count += 1
        if pinned:
            assert (self.pin[3 * total:3 * total + 3] == UNTOUCHED).all(), tag

    def register(self, first, exp, t, rot_step, want=None):
        got = self.sc.register_clouds(first, len(exp), *t, rot_step)
        if want is None:
            want = SC.registered([e.cloud for e in exp], t, rot_step)
        _same(got, want, ("register_clouds", t, rot_step, [e.name for e in exp]), produced=True)
        self.count += 1


def _triples():
    return [pytest.param(shape, i, id=f"{shape[0]}x{shape[1]}-{i}") for shape in SC.SMALL_SHAPES for i in range(len(SC.CASE_LIST) // 3)]


@pytest.mark.parametrize("shape,index", _triples())
def test_crafted_segments(shape, index):
    """three different cases in views 0..2 of one context; every consumer against the restatement, the views armed and written again before
    each; then every consumer over (1, 2), which leaves view 0's outputs and segments as they were"""
    exp = [Expect(shape, *case) for case in SC.triples_of(shape)[index]]
    _, px, n_segs, _ = SC.geometry(*shape)
    with _context(shape, 3) as sc:
        pin = sc.pinned((3 * (3 * px + 1),), np.float32)
        C = Consumers(sc, shape, pin)
        C.put(0, exp)
        for v, e in enumerate(exp):                               # (behind all three puts: no put touched a neighbour)
            check_put(sc, v, e.counts, e.slots)
        for v, e in enumerate(exp):                               # all three still pending
            C.roomy(v, e)
        caps = [SC.capacities(e.counts, e.offsets, e.total, SC.seam_segments(*shape, e.counts)) for e in exp]
        for i in range(max(len(c) for c in caps)):
            C.put(0, exp)
            for v, e in enumerate(exp):
                if i < len(caps[v]):
                    C.clamped(v, e, caps[v][i])
        C.put(0, exp)
        for v, e in enumerate(exp):
            C.pageable(v, e)
        for device_copy in (True, False):
            C.put(0, exp)
            C.counts(0, exp, device_copy)
        C.put(0, exp)
        C.segments(0, exp)
        for pinned, zerocopy in ((True, True), (False, True), (True, False)):
            C.put(0, exp)
            C.download(0, exp, pinned, zerocopy)
        for t, step in SC.REG_SETTINGS:
            C.put(0, exp)
            C.register(0, exp, t, step)
        # ---- calls over (1, 2) leave view 0 alone ----
        C.put(0, exp)
        ptr, stride = C.counts(0, exp, True)
        C.segments(0, exp)
        view0 = (_packed(sc, ptr, stride, 0, exp[0].total).tobytes(), read_segments(sc, 0)[1].tobytes())
        sub = exp[1:]
        for consume in (lambda: C.counts(1, sub, True), lambda: C.counts(1, sub, False), lambda: C.segments(1, sub),
                        lambda: C.download(1, sub, True), lambda: C.download(1, sub, False), lambda: C.download(1, sub, True, zerocopy=False),
                        lambda: C.register(1, sub, *SC.REG_SETTINGS[0]), lambda: (C.roomy(1, sub[0]), C.roomy(2, sub[1]))):
            C.put(1, sub)
            consume()
        assert view0 == (_packed(sc, ptr, stride, 0, exp[0].total).tobytes(), read_segments(sc, 0)[1].tobytes())
        check_put(sc, 0, exp[0].counts, exp[0].slots)
        for v, e in enumerate(exp):                               # and no consumer wrote a segment
            check_put(sc, v, e.counts, e.slots if v else None)
    print(f"{shape[0]}x{shape[1]} triple {index} ({', '.join(e.name for e in exp)}): {C.count} comparisons with the restatement")
    assert C.count > 40


ORDER_CONSUMERS = ("roomy", "clamped", "pageable", "counts", "segments", "register")


@pytest.mark.parametrize("serial", [False, True], ids=["launch-lanes", "serial-launches"])
def test_consumer_orders(serial):
    """every ordered triple of six consumers on one armed, crafted view of the 256-segment shape: 120 sequences, each behind its own
    arm + put, so that a consumer meets the view PENDING, TOTAL_ONLY or DONE in every way the others can leave it"""
    shape = SC.ORDER_SHAPE
    cases = SC.cases_of(shape)
    e = Expect(shape, *cases[5])
    neighbour = Expect(shape, *cases[1])
    assert e.name == "random-finite" and neighbour.name == "full-finite"
    _, px, n_segs, _ = SC.geometry(*shape)
    t, step = SC.REG_SETTINGS[0]
    want_reg = SC.registered([e.cloud], t, step)
    capacity = int(e.offsets[n_segs // 2])                          # ends exactly on a segment seam
    assert 0 < capacity < e.total
    sequences = list(itertools.permutations(ORDER_CONSUMERS, 3))
    assert len(sequences) == 120
    with _context(shape, 2, serial=serial) as sc:
        C = Consumers(sc, shape, sc.pinned((3 * (px + 1),), np.float32))
        run = {"roomy": lambda: C.roomy(1, e), "clamped": lambda: C.clamped(1, e, capacity), "pageable": lambda: C.pageable(1, e),
               "counts": lambda: C.counts(1, [e], True), "segments": lambda: C.segments(1, [e]),
               "register": lambda: C.register(1, [e], t, step, want=want_reg)}
        C.put(0, [neighbour, e])
        for seq in sequences:
            # a series of ten small launches over alternating views: where there are launch lanes, the ninth and the tenth -- the one that
            # arms view 1 -- go to a lane (LanePolicy::LANES_AFTER = 8, sl3d_lanes.h), and the first consumer has to join them
            for _ in range(4):
                sc.run_clouds(0, 1)
                sc.run_clouds(1, 1)
            sc.run_clouds(0, 1)
            arm(sc, 1, 1)
            C.put(0, [neighbour, e], rearm=False)                   # view 0: a full neighbour whose points must never appear
            for name in seq:
                try:
                    run[name]()
                except AssertionError as err:
                    raise AssertionError(f"sequence {seq}, consumer {name}: {err}") from err
        check_put(sc, 0, neighbour.counts, neighbour.slots)
        check_put(sc, 1, e.counts, e.slots)
        lanes = sc.launch_counts()
    print(f"{'serial launches' if serial else 'launch lanes'}: {len(sequences)} sequences, {C.count} comparisons; fused launches (stream, lanes) = {lanes}")
    assert C.count == 3 * len(sequences)
    assert lanes[1] == 0 if serial else lanes[1] >= 2 * len(sequences), lanes


LONG_PAIRS = (("seams", "random"), ("block4", "seams"), ("last_only", "first_only"))


@pytest.mark.parametrize("shape", SC.LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_views_through_the_scan(shape):
    """k_seg_scan where no decode of the suite takes it: a non-empty part 7, a second chunk per part (the prefetch, the second s_wave buffer,
    the carry across chunks), a part 7 of two chunks (the total is the carry behind its last chunk), a third chunk.  Crafted counts over the slots as the arming decode left them, a different pattern in each of two
    views: sl3d_get_cloud_segments (k_seg_scan; then the plain gap-closing copy over its offsets) and sl3d_get_cloud_counts with the device
    copy on pending views (k_seg_close<SCAN>)"""
    W, H = shape
    _, px, n_segs, n_real = SC.geometry(W, H)
    pats = SC.count_patterns(W, H)
    with _context(shape, 2) as sc:
        C = Consumers(sc, shape, None)
        arm(sc, 0, 2)
        raw = [read_segments(sc, v)[2] for v in range(2)]
        assert all(r.shape == (n_segs * SC.SEG, 3) for r in raw)
        for names in LONG_PAIRS:
            exp = [Expect(shape, n, pats[n], raw[v], fill=None) for v, n in enumerate(names)]
            for scan_kernel in (True, False):
                arm(sc, 0, 2)
                for v, e in enumerate(exp):
                    put_segments(sc, v, e.counts)
                if scan_kernel:
                    C.segments(0, exp)
                C.counts(0, exp, True)
    print(f"{W}x{H}: n_segs {n_segs}, (parts, chunks, last chunk) = {SC.scan_layout(n_segs)}, {C.count} comparisons")


def test_large_launch_scans_long_views():
    """k_seg_scan behind the fused kernel at two chunks per part: ONE launch over 5 views of 4096 x 2325 from a real decode; every cloud equals
    xyz[valid] of the dense pass, every offsets array the exclusive scan of its counts"""
    syn = pkg("synth")
    shape = W, H = 4096, 2325
    _, px, n_segs, _ = SC.geometry(W, H)
    assert SC.scan_layout(n_segs) == (5, 2, 336)
    masks = [syn.default_mask(W, H) for _ in range(5)]
    masks[1][:, :W // 2] = 0
    masks[2][:] = 0
    masks[3][H // 3:H // 2, W // 4:W // 2] = 0
    masks[3][np.random.default_rng(3).random((H, W)) < 0.02] = 0
    with _context(shape, 5, masks=masks) as sc:
        sc.run(0, 5)
        want = []
        for v in range(5):
            xyz, valid = sc.points(v)
            want.append(np.ascontiguousarray(xyz[valid == 1]))
        del xyz, valid
        sc.run_clouds(0, 5)
        seg, counts = sc.cloud_segments(0, 5)
        assert counts == [len(w) for w in want] and counts[2] == 0 and min(counts[0], counts[1], counts[3], counts[4]) > 0
        print(f"{W}x{H}, 5 views in one launch: {counts} points of {px} slots each")
        for v in range(5):
            cnt, off, _ = read_segments(sc, v, want_xyz=False)
            incl = np.cumsum(cnt.astype(np.uint64), dtype=np.uint64)
            assert int(incl[-1]) == counts[v] and np.array_equal(off, np.concatenate([np.zeros(1, np.uint64), incl[:-1]])), v
            assert v == 2 or (cnt[4096:8192].any() and cnt[32768:].any())          # counts in a second chunk and in the last part
        ptr, stride, c2 = sc.cloud_counts(0, 5)
        assert c2 == counts
        for v in range(5):
            got = _packed(sc, ptr, stride, v, counts[v])
            assert got.shape == want[v].shape and np.array_equal(got.view(np.uint32), want[v].view(np.uint32)), v
