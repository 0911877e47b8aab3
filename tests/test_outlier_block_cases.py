"""CPU test of the outlier filter's inputs past the first block (tests/outlier_block_cases.py): the table contains what its cases are
labelled with, by the restatement (tests/outlier_reference.py) and the launch geometry read from the text of sl3d_outlier.hip alone.
These are the conditions that keep tests/test_gpu_outlier_blocks.py from passing emptily: a block of k_outlier_apply that did not run,
ran at the wrong offset or stored its counts instead of adding them then differs from the restatement in bytes or in counts."""
import re

import numpy as np
import pytest

import outlier_block_cases as BC
import outlier_reference as OR

IDS = ["%dx%d-r%d-%s-%s" % (c[0], c[1], c[2], c[4], c[5]) for c in BC.CASES]
MULTI = [c for c in BC.CASES if "multi" in c[6]]
MIXED = [c for c in BC.CASES if "mixed" in c[6]]
EDGES = [c for c in BC.CASES if {"edge_w", "edge_h"} & set(c[6])]


def _ids(cases):
    return [IDS[BC.CASES.index(c)] for c in cases]


def test_the_constants_are_the_kernel_source_s():
    """read from the text, and the text still states the rule apply_block restates"""
    with open(BC.SOURCE) as f:
        src = f.read()
    assert (BC.RUNS, BC.TILE_W, BC.TILE_H) == (8, 64, 8), "the table below was chosen for these: choose its shapes anew"
    assert BC.BLOCK_QUADS == 2048 and BC.RUN_QUADS == 256
    assert re.search(r"t = \(blockIdx\.x \* OUTLIER_APPLY_RUNS \+ run\) \* 256u \+ threadIdx\.x;", src)
    assert re.search(r"row = \(int\)\(t / \(unsigned\)lpr\)", src) and re.search(r"lpr = \(W \+ 3\) / 4;", src)
    assert src.count("__launch_bounds__(256)") == 2
    assert re.search(r"\+ 256 \* OUTLIER_APPLY_RUNS - 1\) / \(256 \* OUTLIER_APPLY_RUNS\)", src)


def test_apply_block_is_the_quad_rule():
    for W, H in ((5, 3), (257, 33), (1, 2060), (8240, 1)):
        lpr = -(-W // 4)
        want = np.array([[(r * lpr + c // 4) // (256 * BC.RUNS) for c in range(W)] for r in range(H)])
        assert np.array_equal(BC.apply_blocks(W, H), want) and BC.apply_block(W, H - 1, W - 1) == BC.n_apply_blocks(W, H) - 1
    assert BC.apply_block(257, 31, 131) == 0 and BC.apply_block(257, 31, 132) == 1          # the seam of 257 x 33 lies inside row 31
    assert BC.apply_block(1, 2047, 0) == 0 and BC.apply_block(1, 2048, 0) == 1              # lpr == 1: a block is 2048 rows


def test_the_table_holds_every_block_count_and_shape_of_the_issue():
    shapes = {c[:2]: set(c[6]) for c in BC.CASES}
    assert set(shapes) == set(BC.SHAPES) and max(W * H for W, H in shapes) == BC.LARGEST == 16250
    for (W, H), labels in shapes.items():
        q, n = BC.quads(W, H), BC.n_apply_blocks(W, H)
        assert ("multi" in labels) == (n >= 2), (W, H)
        assert ("exact_multiple" in labels) == (q % BC.BLOCK_QUADS == 0), (W, H)
        assert ("break_in_run_0" in labels) == (n >= 2 and BC.last_run(W, H) == 0 and q % BC.BLOCK_QUADS != 0), (W, H)
        assert ("break_in_a_later_run" in labels) == (n >= 2 and 0 < BC.last_run(W, H) and q % BC.BLOCK_QUADS != 0), (W, H)
        assert ("three_blocks" in labels) == (n >= 3), (W, H)
        assert ("edge_w" in labels) == (W % BC.TILE_W == 0) and ("edge_h" in labels) == (H % BC.TILE_H == 0), (W, H)
        assert ("line" in labels) == (min(W, H) == 1), (W, H)
    for kind in BC.BLOCK_KINDS:
        assert any(kind in labels for labels in shapes.values()), kind
    assert BC.quads(64, 128) == 2048 and BC.n_apply_blocks(64, 128) == 1 and BC.last_run(64, 128) == BC.RUNS - 1      # every run full, no break
    assert BC.quads(64, 129) == 2064 and BC.quads(257, 33) == 2145 and BC.quads(130, 125) == 4125 and BC.quads(130, 80) == 2640
    assert BC.apply_blocks(257, 33)[31].tolist().count(0) == 132                                   # the seam in the middle of a row
    assert (BC.n_apply_blocks(130, 125), (BC.apply_blocks(130, 125) == 1).sum()) == (3, 2048 * 4 - 2 * 62)      # two of them full (130 = 4 * 32 + 2)
    # the line shapes: a few dozen quads in the second block, the support grid 129 tiles wide / 258 tiles high
    assert BC.support_grid(*BC.ROW_SHAPE) == (129, 1) and BC.support_grid(*BC.COLUMN_SHAPE) == (1, 258)
    assert 12 <= BC.quads(*BC.ROW_SHAPE) - 2048 <= 48 and 12 <= BC.quads(*BC.COLUMN_SHAPE) - 2048 <= 48
    # widths that leave one column in the last tile and in the last quad; a tile edge both ways, and one row or column past it
    assert 257 % BC.TILE_W == 1 and 65 % BC.TILE_W == 1 and 257 % 4 == 1
    assert {(64, 8), (128, 16), (65, 8), (64, 9)} <= set(shapes)
    assert BC.support_grid(64, 8) == (1, 1) and BC.support_grid(65, 8) == (2, 1) and BC.support_grid(64, 9) == (1, 2) and BC.support_grid(128, 16) == (2, 2)
    # the rules the issue asks for once each, on the three-block shape
    rules = [c[2:6] for c in BC.cases_of(BC.BATCH_SHAPE)]
    assert any(r[2] == 0 for r in rules) and (4, BC.INF, OR.max_support(4), "all_valid") in rules
    assert BC.n_apply_blocks(*BC.BATCH_SHAPE) >= 3


@pytest.mark.parametrize("case", MIXED, ids=_ids(MIXED))
def test_every_block_of_a_mixed_case_rejects_and_keeps(case):
    per_block = BC.block_counts(case)
    assert len(per_block) == BC.n_apply_blocks(*case[:2])
    for b, (samples, rejected) in enumerate(per_block):
        assert 0 < rejected < samples, (b, samples, rejected)
    if "line" not in case[6]:
        assert all(rejected >= 2 and samples - rejected >= 17 for samples, rejected in per_block), per_block


def test_the_figures_of_the_issue():
    by = {c[:6]: BC.block_counts(c) for c in MIXED}
    assert by[(130, 125, 1, 1.0, 3, "holes")] == [(4045 + 1535, 1535), (4110 + 1508, 1508), (38 + 35, 35)]
    assert by[(64, 129, 4, 2.5, 20, "step")] == [(7324 + 622, 622), (57 + 6, 6)]
    # all valid at radius 4 leaves the last block of 257 x 33 without a rejection: it is not the mixed case there
    assert BC.block_counts((257, 33) + OR.PARAMS[4] + ("all_valid", ()))[1][1] == 0
    # a line under PARAMS loses every sample: why the line shapes have rules of their own
    for shape in (BC.ROW_SHAPE, BC.COLUMN_SHAPE):
        samples, rejected = BC.restated(shape + OR.PARAMS[2] + ("holes", ()))["counts"]
        assert samples == rejected > 0


@pytest.mark.parametrize("case", MULTI, ids=_ids(MULTI))
def test_no_proper_subset_of_the_blocks_adds_up_to_the_counts(case):
    """what a plain store in place of the atomic add, or a block that did not run, would leave"""
    per_block, total = BC.block_counts(case), BC.restated(case)["counts"]
    assert len(per_block) >= 2 and tuple(np.sum(per_block, axis=0)) == total
    if case[5] == "none_valid":
        assert total == (0, 0)                                              # every block adds 0: the words stay as the host zeroed them
        return
    assert total not in BC.subset_sums(per_block)
    assert all(samples > 0 for samples, _ in per_block)
    if case[4] == 0:
        assert total[1] == 0


@pytest.mark.parametrize("case", EDGES, ids=_ids(EDGES))
def test_the_tile_edge_cases_would_count_what_lies_beyond_the_edge(case):
    W, H, radius, max_dist, min_n, name, labels = case
    xyz, valid = BC.content(name, W, H)
    support = OR.support_plane(xyz, valid, radius, max_dist)
    sample = valid == 1
    r, c = np.mgrid[0:H, 0:W]
    assert ("edge_w" in labels) == (W % BC.TILE_W == 0) and ("edge_h" in labels) == (H % BC.TILE_H == 0)
    if name != "torus":
        return
    assert BC.rolls(W, H) == (W // 2 if "edge_w" in labels else 0, H // 2 if "edge_h" in labels else 0)
    for label, near, kw in (("edge_w", (c >= W - radius) | (c < radius), dict(columns=True, rows=False)),
                            ("edge_h", (r >= H - radius) | (r < radius), dict(columns=False, rows=True))):
        if label not in labels:
            continue
        beyond = BC.support_beyond(xyz, valid, radius, max_dist, **kw)
        assert np.array_equal(beyond[~near], support[~near]) and (beyond[sample] >= support[sample]).all()
        more = sample & near & (beyond > support)
        # on both sides of the edge, and some of them change the decision
        side = (c >= W - radius) if label == "edge_w" else (r >= H - radius)
        assert (more & side).any() and (more & ~side).any()
        assert (more & (support < min_n) & (beyond >= min_n)).any(), "a sample the rule rejects and an unclipped neighbourhood would keep"


def test_support_beyond_is_the_restatement_where_nothing_is_continued():
    xyz, valid = BC.content("torus", 64, 8)
    assert np.array_equal(BC.support_beyond(xyz, valid, 2, 1.5, False, False), OR.support_plane(xyz, valid, 2, 1.5))
    # continued by columns, pixel (r, W - 1) sees (r + 1, 0): one valid pixel each, one spacing apart by construction of the content
    x = np.zeros((3, 16, 3), np.float32)
    v = np.zeros((3, 16), np.uint8)
    v[0, 15] = v[1, 0] = 1
    got = BC.support_beyond(x, v, 1, 1.0, True, False)
    assert got[0, 15] == 1 and got[1, 0] == 1 and OR.support_plane(x, v, 1, 1.0)[0, 15] == 0


def test_the_seam_line_straddles_the_two_blocks():
    W, H = 257, 33
    cells = BC.seam_row_cells(W, H)
    assert len(cells) == 10 and len({r for r, _ in cells}) == 1 and cells[0][0] == 31
    assert [int(BC.apply_block(W, r, c)) for r, c in cells] == [0] * 5 + [1] * 5
    assert [c for _, c in cells] == list(range(127, 137))
    xyz, valid = OR.jacobi_line(H, W, cells)
    left = list(cells)
    for _ in range(3):                                                       # each call removes exactly the two ends
        f = OR.filter_outliers(xyz, valid, 1, 1.0, 2)
        assert f["counts"] == (len(left), 2) and f["rejected"][left[0]] and f["rejected"][left[-1]]
        left, valid = left[1:-1], f["valid"]
    assert BC.apply_block(W, *left[0]) == 0 and BC.apply_block(W, *left[-1]) == 1
