"""CPU test of the captures tests/test_gpu_repair_fused.py runs k_repair_fused on (SL3D_FLAG_REPAIR_PERIODS).

The crafted seams of tests/period_cases.py sit at rows 7|8 and 31|32 and at columns 63|64 and 255|256: the tiles of k_period_jumps, not
those of k_repair_fused (64 columns x 16 rows, both axes in one block).  What the new kernel can get wrong at a seam is the halo it
decodes itself: the quad left and right of every tile row for the vertical axis, the four rows above and below the tile for the horizontal
one.  So, from the NumPy restatement (tests/period_repair_reference.py) at radius 4 over the oracle's stage-4 planes: every seam between two
tiles of the new kernel, in EVERY pair of tiles that share it, has on each side a repaired pixel whose neighbourhood holds a sample on
the other side -- in the grid cases or the fuzz cases, which the GPU test compares bit for bit.  A halo that was staged wrong (another
row, another column, +infinity) then changes a median that decides a repair."""
import functools
import os
import re

import numpy as np

from conftest import ROOT

import period_cases as PC
import period_repair_reference as PR

RADIUS = 4
COLS, ROWS = 64, 16            # the tile of k_repair_fused
CAPTURES = ("grid", "grid_window") + PC.FUZZ_SEEDS


def test_the_tile_is_the_kernels():
    src = open(os.path.join(ROOT, "3dscan_amd", "csrc", "sl3d_repair_fused.hip")).read()
    m = re.search(r"RPF_COLS\s*=\s*(\d+)\s*,\s*RPF_ROWS\s*=\s*(\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (COLS, ROWS)
    assert re.search(r"#define\s+SL3D_REPAIR_FUSED_RADIUS\s+4\b", open(os.path.join(ROOT, "3dscan_amd", "csrc", "sl3d_internal.h")).read())


@functools.lru_cache(maxsize=None)
def _repaired(name):
    """Per axis: (the pixels one pass at radius 4 repairs, the samples) of a capture."""
    case = PC.make_fuzz_case(name) if isinstance(name, int) else PC.make_grid_case(name)
    out = []
    for axis, (code, wrapped, unw, valid) in enumerate(PC.oracle_stage4(case)):
        code2, _, rep, _ = PR.repair_periods(code, wrapped, unw, valid, axis, RADIUS, case["N"])
        assert rep == int((code2 != code).sum()) and rep > 0
        out.append((code2 != code, PR.samples(valid, axis)))
    return out


def _reaches_across(rep, smp, seam, lo_side):
    """Along the lines of [lines][coded direction] planes: a repaired pixel on one side of seam - 1 | seam with a sample on the other side
    within RADIUS of it."""
    for line in range(rep.shape[0]):
        for p in (range(seam - RADIUS, seam) if lo_side else range(seam, min(seam + RADIUS, rep.shape[1]))):
            if not rep[line, p]:
                continue
            other = range(seam, min(p + RADIUS, rep.shape[1] - 1) + 1) if lo_side else range(max(p - RADIUS, 0), seam)
            if any(smp[line, q] for q in other):
                return True
    return False


def test_every_seam_of_the_new_tile_is_covered_both_ways():
    W, H = PC.make_grid_case("grid")["W"], PC.make_grid_case("grid")["H"]
    assert W > 4 * COLS and H > 4 * ROWS and W % COLS and H % ROWS, "several tiles both ways, partial last tiles"
    missing = []
    for axis in (0, 1):
        # vertical axis: neighbourhoods run along a row and cross the COLUMN seams, in every tile row; horizontal: the transpose
        along, across, size, lines = (COLS, ROWS, W, H) if axis == 0 else (ROWS, COLS, H, W)
        for seam in range(along, size, along):
            for t0 in range(0, lines, across):
                for lo_side in (True, False):
                    found = False
                    for name in CAPTURES:
                        rep, smp = _repaired(name)[axis]
                        if axis == 1:
                            rep, smp = rep.T, smp.T
                        if _reaches_across(rep[t0:t0 + across], smp[t0:t0 + across], seam, lo_side):
                            found = True
                            break
                    if not found:
                        missing.append((axis, seam, t0, "low side" if lo_side else "high side"))
    assert not missing, missing


def test_the_fuzz_views_differ_and_repair_on_both_axes():
    reps = [_repaired(seed) for seed in PC.FUZZ_SEEDS]
    for axis in (0, 1):
        assert len({r[axis][0].tobytes() for r in reps}) == len(reps)
        assert all(r[axis][0].sum() > 1000 for r in reps)
