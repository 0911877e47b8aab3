"""GPU tests (-m gpu) of the radius outlier filter past the first block of k_outlier_apply and on the tile edges of k_outlier_support
(DESIGN 4u), against the NumPy restatement (tests/outlier_reference.py), bit for bit -- support plane, valid, points (as uint32) and
counts.  The inputs are the table of tests/outlier_block_cases.py; tests/test_outlier_block_cases.py asserts on the CPU that every apply
block of a `mixed` case rejects some samples and keeps others, so a block that did not run, ran at another block's offset or stored its
counts over another block's fails here.  The padding columns are poisoned as in tests/test_gpu_outliers.py wherever the pitch exceeds W.

1. Every case of the table: one block with every run full (64x128), a second block that ends in run 0 (64x129, 257x33 -- the seam inside
   a row, one column in the last tile and the last quad), in a later run (130x80), three blocks (130x125; min_neighbours 0 and the largest
   min_neighbours of radius 4 under +inf there), one row of 8240 and one column of 2060 pixels, and the shapes whose window edge is a tile
   edge (64x8, 128x16, 65x8, 64x9).  Where the lower edge is a tile edge the next view holds the same planes: the row behind the window's
   last is then the content's first, and the `torus` content puts points within max_dist there.
2. A batch of views 1 .. 5 of 7 over the three-block shape, `none_valid` among them: each view its own restatement and counts, the two
   views outside keep every byte, support plane included.
3. Jacobi across the seam of two apply blocks: a row of samples loses exactly its two ends per call.
4. KEEP_STAGES on a two-block shape: intersection_points is +0.0 under exactly the rejected pixels."""
import numpy as np
import pytest

import outlier_block_cases as BC
import outlier_reference as OR
from test_gpu_outliers import _context, _filter_and_check, _put, _same_as, _state

pytestmark = pytest.mark.gpu


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_table_cases_equal_the_restatement(shape):
    W, H = shape
    cases = BC.cases_of(shape)
    twice = "edge_h" in cases[0][6]                                     # the same planes in the next view: what lies behind the last row
    with _context(W, H, V=2 if twice else 1) as sc:
        for case in cases:
            _, _, radius, max_dist, min_n, name, labels = case
            xyz, valid = BC.content(name, W, H)
            if twice:
                _put(sc, 1, xyz, valid)
            want = _filter_and_check(sc, xyz, valid, radius, max_dist, min_n, case[:6])
            assert want["counts"] == tuple(np.sum(BC.block_counts(case), axis=0))
            if "mixed" in labels:
                assert 0 < want["counts"][1] < want["counts"][0]
            if min_n == 0:
                assert want["counts"][1] == 0 and want["counts"][0] > 0
            if twice:                                                   # the view behind: its own result, the first view's row above its first
                _put(sc, 0, xyz, valid)
                counts = sc.filter_outliers(radius, max_dist, min_n, first_view=0, n_views=2)
                for v in (0, 1):
                    _same_as(sc, v, want, counts[v], (case[:6], "view", v))


# ---- 2. a batch over three blocks ------------------------------------------------------------------------------------------------------------
def test_a_batch_adds_every_block_of_every_view_into_its_own_words():
    (W, H), V = BC.BATCH_SHAPE, 7
    assert BC.n_apply_blocks(W, H) == 3
    names = ["torus", "holes", "step", "none_valid", "all_valid", "corners", "step"]        # views 0 .. 6; the batch is views 1 .. 5
    content = [BC.content(n, W, H) for n in names]
    with _context(W, H, V=V) as sc:
        for v, (xyz, valid) in enumerate(content):
            _put(sc, v, xyz, valid)
        for v in (0, 6):                                                # the views outside get a support plane of their own first
            sc.filter_outliers(1, 1.0, 0, first_view=v)
        outside = {v: _state(sc, v) + (sc.support(v),) for v in (0, 6)}
        counts = sc.filter_outliers(2, 1.5, 8, first_view=1, n_views=5)
        assert counts.shape == (5, 2)
        for k, v in enumerate(range(1, 6)):
            want = OR.filter_outliers(*content[v], 2, 1.5, 8)
            _same_as(sc, v, want, counts[k], ("view", v, names[v]))
        assert tuple(counts[2]) == (0, 0), "none_valid: every block of the view adds 0"
        assert len({tuple(c) for c in counts.tolist()}) == 5, "the views differ"
        for v, before in outside.items():
            after = _state(sc, v) + (sc.support(v),)
            assert all(np.array_equal(a, b) for a, b in zip(after, before)), ("view outside the batch", v)
        # once more with counts over all seven views and nothing to reject: the samples of every block of every view
        counts = sc.filter_outliers(1, 1.0, 0, first_view=0, n_views=V)
        for v in range(V):
            xyz, valid = _after(content[v], 2, 1.5, 8) if 1 <= v <= 5 else content[v]
            _same_as(sc, v, OR.filter_outliers(xyz, valid, 1, 1.0, 0), counts[v], ("second call, view", v))


def _after(planes, radius, max_dist, min_n):
    """(xyz, valid) as a filter call leaves them"""
    f = OR.filter_outliers(*planes, radius, max_dist, min_n)
    return f["bits"].view(np.float32), f["valid"]


# ---- 3. Jacobi across the seam of two apply blocks -------------------------------------------------------------------------------------------
def test_a_line_across_the_block_seam_loses_its_two_ends_per_call():
    W, H = 257, 33
    cells = BC.seam_row_cells(W, H)
    assert {int(BC.apply_block(W, r, c)) for r, c in cells} == {0, 1}
    xyz, valid = OR.jacobi_line(H, W, cells)
    with _context(W, H) as sc:
        _put(sc, 0, xyz, valid, pad=0)
        left = list(cells)
        for call in range(3):
            counts = sc.filter_outliers(1, 1.0, 2)
            assert tuple(counts[0]) == (len(left), 2), (call, counts)
            ends, left = (left[0], left[-1]), left[1:-1]
            assert int(BC.apply_block(W, *ends[0])) == 0 and int(BC.apply_block(W, *ends[1])) == 1, "one end in each block"
            got_v, got_b = _state(sc)
            want_v = np.zeros((H, W), np.uint8)
            for r, c in left:
                want_v[r, c] = 1
            assert np.array_equal(got_v, want_v), (call, "an in-place sweep eats the line")
            gone = (valid == 1) & (want_v == 0)
            assert (got_b[gone] == OR.NAN_BITS).all() and np.array_equal(got_b[~gone], xyz.view(np.uint32)[~gone])
            s = sc.support()
            assert all(s[r, c] == 2 for r, c in left) and all(s[r, c] == 1 for r, c in ends)      # the support as it was on entry
            assert (s == OR.NO_SAMPLE).sum() == W * H - len(left) - 2


# ---- 4. KEEP_STAGES over two blocks ----------------------------------------------------------------------------------------------------------
def test_keep_stages_zeroes_intersection_points_under_the_rejected_pixels_of_every_block():
    case = (257, 33) + OR.PARAMS[1] + ("holes",)
    W, H, radius, max_dist, min_n, name = case
    xyz, valid = BC.content(name, W, H)
    blocks = BC.apply_blocks(W, H)
    with _context(W, H, keep=True) as sc:
        before = sc.intersection_points()
        assert before.dtype == np.float64 and before.shape == (H, W, 3)
        assert all((before[blocks == b] != 0).any() for b in (0, 1)), "the decode left something to zero in both blocks"
        want = _filter_and_check(sc, xyz, valid, radius, max_dist, min_n, case)
        rejected = want["rejected"]
        assert all((rejected & (blocks == b)).any() and (~rejected & (blocks == b)).any() for b in (0, 1))
        ip = sc.intersection_points()
        assert (ip[rejected] == 0).all() and not np.signbit(ip[rejected]).any()
        assert np.array_equal(ip[~rejected].view(np.uint64), before[~rejected].view(np.uint64))
        assert (before[rejected] != 0).any(), "the rejected pixels held something"
