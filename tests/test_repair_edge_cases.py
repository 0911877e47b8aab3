"""CPU tests of the inputs tests/test_gpu_repair_edges.py runs the period repair on (k_period_jumps<AXIS, R>, k_period_apply,
k_repair_fused<SUB>): EF.REPAIR_CASES and the three view captures under the masks A, B, C of tests/edge_frames.py.

These are conditions on the INPUTS, asserted on the NumPy restatement (tests/period_repair_reference.py) applied to the oracle's planes
(EF.stage_planes) alone, so that a GPU test can never pass for want of a branch: dense and large jumps, runs shorter than radius + 1, neighbourhoods clipped
by the window, an axis with one sample line, a window column that carries an absolute phase and is no sample, medians that are ties
between different periods (where the lower and the upper median decide differently), a valid set that moves through the repair, and
selected pixels of the views A and B on both sides of every seam of k_repair_fused's 64 x 16 tile.  If a seed fails one, the seed or the
shape changes, never the condition.  The counts are printed.

The unrepairable branch (k' outside 0 .. 2^N - 1) is NOT among them: the median keeps k' in range on random inputs (a handful of pixels
in all cases together, printed by test_unrepairable_pixels_are_counted_and_printed and not asserted on).  That branch stays with the
border_* cases of tests/period_cases.py."""
import numpy as np
import pytest

import edge_frames as EF
import period_repair_reference as PR

RADII = (1, 4, 8)
FLAT = ("flat_17", "flat_0", "flat_255")
COLS, ROWS = 64, 16            # the tile of k_repair_fused (tests/test_repair_fused_cases.py holds it against the source)


def _upper_median(vals):
    s = sorted(vals)
    return s[len(s) // 2]


def _analyse(o, axis, radius):
    """Per pixel, walked as the definition reads: n (the samples of the neighbourhood; -1 off the samples), clipped (the window cuts the
    neighbourhood), tie (the lower median's value occurs more than once among them), j (0 where n < radius + 1)."""
    unw, smp = o["unw"][axis], PR.samples(o["valid_axis"][axis], axis)
    if axis == 1:
        unw, smp = unw.T, smp.T
    n = np.full(smp.shape, -1)
    clipped, tie, j = np.zeros(smp.shape, bool), np.zeros(smp.shape, bool), np.zeros(smp.shape, np.int64)
    L = smp.shape[1]
    for line in range(smp.shape[0]):
        for p in np.nonzero(smp[line])[0]:
            S = [unw[line, q] for q in range(max(0, p - radius), min(L - 1, p + radius) + 1) if smp[line, q]]
            n[line, p], clipped[line, p] = len(S), p - radius < 0 or p + radius > L - 1
            m = PR._lower_median(S)
            tie[line, p] = S.count(m) > 1
            if len(S) >= radius + 1:
                j[line, p] = int(np.rint((np.float64(unw[line, p]) - np.float64(m)) / PR.TWO_PI_REF))
    out = dict(n=n, clipped=clipped, tie=tie, j=j, samples=smp)
    return {k: v.T for k, v in out.items()} if axis == 1 else out


def _with_upper_median(monkeypatch, o, radius):
    """Per axis: the codes one pass leaves under the lower median (the definition), and how many of them the upper median changes."""
    lower = EF.repair(o, radius)["code"]
    monkeypatch.setattr(PR, "_lower_median", _upper_median)
    upper = EF.repair(o, radius)["code"]
    monkeypatch.undo()
    return [int((lower[a] != upper[a]).sum()) for a in (0, 1)]


# ---- random bytes, every pixel selected ------------------------------------------------------------------------------------------------------
def test_random_frames_hold_dense_and_large_jumps_and_move_the_valid_set():
    c = ("random", "base", 1.0)
    o = EF.oracle_scan(*c)
    for radius in RADII:
        counts = EF.restated_repair(*c, radius)["counts"][0]
        for a in (0, 1):
            s = int(PR.samples(o["valid_axis"][a], a).sum())
            assert counts[a][0] > s / 2, (radius, a, counts[a], s)
            an = _analyse(o, a, radius)
            assert int((an["j"] != 0).sum()) == sum(counts[a]), "the walk of this module is the restatement's"
            big = int(np.abs(an["j"]).max())
            print(f"random / base / 1.0, radius {radius}, axis {a}: {counts[a][0]} of {s} samples repaired, {counts[a][1]} unrepairable, max |j| {big}")
            assert big >= (64, 32)[a]
    after = EF.restated_repaired_scan(*c)["valid"]
    assert np.array_equal(EF.restated_repaired_scan(*c)["valid_before"], o["valid"]), "EF.stage5 is the oracle's stage 5"
    moved = int((after != o["valid"]).sum())
    print(f"merged valid: {int((o['valid'] == 1).sum())} before, {int((after == 1).sum())} after the repair, {moved} pixels change side")
    assert moved > 500


# ---- flat frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FLAT)
def test_flat_frames_repair_nothing_and_every_median_is_a_tie(name):
    o = EF.oracle_scan(name, "base", 1.0)
    for radius in RADII:
        assert EF.restated_repair(name, "base", 1.0, radius)["counts"][0] == ((0, 0), (0, 0))
        for a in (0, 1):
            an = _analyse(o, a, radius)
            assert an["samples"].sum() > 3000 and an["tie"][an["samples"]].all() and not an["j"].any()


# ---- the mask that holds the value 2 -----------------------------------------------------------------------------------------------------------
def test_the_mask_with_the_value_2_leaves_short_runs_and_clipped_neighbourhoods():
    c = ("random", "base", 0.9)
    o, mask = EF.oracle_scan(*c), EF.case(*c)["mask"]
    assert (mask == 2).sum() > 50
    for a in (0, 1):
        an = _analyse(o, a, 4)
        smp = an["samples"]
        short, clipped = int((smp & (an["n"] < 5)).sum()), int((smp & an["clipped"]).sum())
        print(f"random / base / 0.9, axis {a}: {int(smp.sum())} samples, {short} with n < 5 at radius 4, {clipped} with a clipped neighbourhood")
        assert short > 100 and clipped > 10
        assert not smp[mask == 2].any() and not (o["valid_axis"][a][mask == 2] == 1).any(), "no pixel under a 2 is a sample"


# ---- the degenerate axes ---------------------------------------------------------------------------------------------------------------------
def test_one_sample_row_repairs_nothing():
    c = ("random", "130x3", 1.0)
    o = EF.oracle_scan(*c)
    for radius in range(1, 9):
        an = _analyse(o, 1, radius)
        assert an["samples"].sum() > 100 and (an["n"][an["samples"]] == 1).all(), "no horizontal-axis sample has n >= 2"
        counts = EF.restated_repair(*c, radius)["counts"][0]
        assert counts[1] == (0, 0) and counts[0][0] > 0, (radius, counts)


def test_three_sample_rows_are_below_radius_plus_1():
    c = ("random", "64x5", 0.5)
    for radius in (4, 8):
        counts = EF.restated_repair(*c, radius)["counts"][0]
        assert counts[1] == (0, 0) and counts[0][0] > 0, (radius, counts)


# ---- the window --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.9, 1.0])
def test_window_border_lines_carry_a_phase_and_are_no_samples(p):
    """Stage 4's loop runs by FRAME coordinates: window column 0 is frame column 37 and window row 0 is frame row 5, so both carry an
    absolute phase -- and neither is a sample, which is defined by WINDOW coordinates; likewise the last column and row
    (EF.stage_planes: the oracle on the grown window, the valid byte of stage 3 over the whole frame).  Under the 0.9 mask stage 3 leaves
    no pixel of the first column selected: hence the 1.0 window, on which every line is asserted."""
    o = EF.stage_planes("random", "window", p)
    (W, H), (col0, row0), (fullW, fullH) = EF.SHAPES["window"]
    assert 1 <= col0 and col0 + W - 1 <= fullW - 2 and 1 <= row0 and row0 + H - 1 <= fullH - 2
    for a, lines in ((0, (np.s_[:, 0], np.s_[:, W - 1])), (1, (np.s_[0, :], np.s_[H - 1, :]))):
        sel, unw = o["valid_axis"][a], o["unw"][a]
        on = [int(((sel[line] == 1) & (unw[line] != 0)).sum()) for line in lines]
        print(f"window / {p}, axis {a}: {on} selected pixels of the first / last {'column' if a == 0 else 'row'} carry an absolute phase")
        assert all(not PR.samples(sel, a)[line].any() for line in lines)
        assert min(on) > 0 or (p == 0.9 and a == 0)
        # ... and they lie within reach of samples: counted as samples they would enter medians
        smp = PR.samples(sel, a)
        near = [smp[:, 1:5].any(), smp[:, W - 5:W - 1].any()] if a == 0 else [smp[1:5].any(), smp[H - 5:H - 1].any()]
        assert all(near)


# ---- ties between different periods --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.9])
def test_steps_frames_are_ties_between_different_periods(p, monkeypatch):
    c = ("steps", "base", p)
    o = EF.oracle_scan(*c)
    for a in (0, 1):
        sel = o["valid_axis"][a] == 1
        assert set(np.unique(o["code"][a][sel]).tolist()) == {0, 1, 2, 3} and len(np.unique(o["w"][a][PR.samples(o["valid_axis"][a], a)])) == 1
    seen = set()
    for radius in RADII:
        r = EF.restated_repair(*c, radius, 2)
        for a in (0, 1):
            an = _analyse(o, a, radius)
            seen |= set(np.unique(an["j"]).tolist())
            considered = an["samples"] & (an["n"] >= radius + 1)
            assert an["tie"][considered].any() and (an["j"][an["tie"]] != 0).any(), "a tie at the median, and a jump decided by one"
            print(f"steps / base / {p}, radius {radius}, axis {a}: first pass {r['counts'][0][a]}, second pass {r['counts'][1][a]}")
            assert r["counts"][1][a][0] > 0, "a second pass repairs more: the pass is a Jacobi pass"
            if p == 1.0:
                assert r["counts"][0][a][0] > 1000
    assert seen == set(range(-3, 4)), seen
    changed = _with_upper_median(monkeypatch, o, 4)
    print(f"steps / base / {p}: the upper median changes {changed} codes")
    assert min(changed) >= 1


@pytest.mark.parametrize("c", [("random", "base", 0.9), ("noise3", "base", 1.0), ("random", "window", 0.9), ("random", "window", 1.0)], ids=lambda c: "-".join(map(str, c)))
def test_the_upper_median_is_another_repair(c, monkeypatch):
    changed = _with_upper_median(monkeypatch, EF.stage_planes(*c), 4)
    print(f"{c}: the upper median changes {changed} codes")
    assert min(changed) >= 1


# ---- the three views under A, B, C -------------------------------------------------------------------------------------------------------------
def test_views_a_and_b_repair_at_the_seams_and_view_c_repairs_nothing():
    masks = EF.view_masks()
    counts = [EF.restated_view_repair(v, 4)["counts"][0] for v in range(3)]
    print(f"repaired (vertical, horizontal) at radius 4: A {counts[0][0][0]} / {counts[0][1][0]}, B {counts[1][0][0]} / {counts[1][1][0]}, C {counts[2][0][0]} / {counts[2][1][0]}")
    for v in (0, 1):
        assert counts[v][0][0] > 0 and counts[v][1][0] > 0
    assert counts[2] == ((0, 0), (0, 0))
    oc = EF.oracle_view_scan(2)
    for a in (0, 1):
        an = _analyse(oc, a, 4)
        assert an["samples"].sum() >= 30 and (an["n"][an["samples"]] == 1).all(), "C's selected pixels are isolated"
    # the seams of k_repair_fused's tile on the base shape: column 64, rows 16 and 32; A ends at row 26
    for v, row_seams in ((0, (ROWS,)), (1, (ROWS, 2 * ROWS))):
        o = EF.oracle_view_scan(v)
        assert np.array_equal(o["valid_axis"][0], EF.selected(masks[v]))
        smp_v, smp_h = PR.samples(o["valid_axis"][0], 0), PR.samples(o["valid_axis"][1], 1)
        assert smp_v[:, COLS - 4:COLS].any() and smp_v[:, COLS:COLS + 4].any(), (v, "column", COLS)
        for r in row_seams:
            assert smp_h[r - 4:r].any() and smp_h[r:r + 4].any(), (v, "row", r)
    # ... and repaired pixels beside them, so that a halo quad staged under another view's mask bits changes a result: both sides of column
    # 64 in A and of row 32 in B (B's rows 32..35 lie under a halo of rows 28..31, where A selects nothing), the low side of row 16 in B
    rep = [[EF.restated_view_repair(v, 4)["code"][a] != EF.oracle_view_scan(v)["code"][a] for a in (0, 1)] for v in (0, 1)]
    assert rep[0][0][:, COLS - 4:COLS].any() and rep[0][0][:, COLS:COLS + 4].any()
    assert rep[1][1][2 * ROWS - 4:2 * ROWS].any() and rep[1][1][2 * ROWS:2 * ROWS + 4].any() and rep[1][1][ROWS - 4:ROWS].any()


# ---- what is not asserted ----------------------------------------------------------------------------------------------------------------------
def test_unrepairable_pixels_are_counted_and_printed():
    total = 0
    for c in EF.REPAIR_CASES:
        per = {radius: [n[1] for n in EF.restated_repair(*c, radius)["counts"][0]] for radius in RADII}
        total += sum(sum(v) for v in per.values())
        print(f"{c}: unrepairable (vertical, horizontal) per radius {per}")
    print(f"unrepairable pixels in all cases together: {total}")


def test_what_each_case_is_there_for():
    """EF.REPAIRS: per case, whether one radius-4 pass repairs pixels on the (vertical, horizontal) axis -- what the GPU tests assert of the
    device's counts before they compare a scan."""
    assert set(EF.REPAIRS) == set(EF.REPAIR_CASES)
    for c, want in EF.REPAIRS.items():
        counts = EF.restated_repair(*c, 4)["counts"][0]
        assert tuple(n[0] > 0 for n in counts) == want, (c, counts)
