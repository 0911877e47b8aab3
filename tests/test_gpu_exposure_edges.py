"""GPU tests (-m gpu) of the edges of k_fuse_exposures' launch against the NumPy restatement (tests/exposure_reference.py), bit for
bit -- frames in use, map and counts.  The inputs are those of tests/exposure_cases.py; tests/test_exposure_cases.py asserts on the CPU
what each of them holds.

1. The shapes 1x1, 5x1, 1x9, 65x3, 253x2: one window pixel in a row's last quad, with and without whole padding quads behind it, one row,
   less than a wave -- E = 1, 3, 8, saturation 255 and 200, F = 3 and 4.  The counts tell whether the lone pixel was taken for a window pixel.
2. The banded stack at E = 8: every exposure 0 .. 7 on whole quads (the one-exposure path of pass 2 with every e0) and two exposures in
   the quad at every band edge (the byte-select path beside it); sources in views 1 .. 8 and 2 .. 9, dst_view below and above them.
3. Every byte 255 at (N_v, N_h) = (16, 16), F = 4: the largest clip count the key holds, n = 72; then 71 against 72.
4. Saturations 2, 127, 128, 129, 254 over bytes drawn from {s - 1, s, s + 1, 0, 255}: both sides of the switch of exp_clip_test."""
import numpy as np
import pytest

import exposure_cases as XC
import exposure_reference as XR
from test_gpu_exposure import _check_fusion, _download, _ppv, _scanner, _upload

pytestmark = pytest.mark.gpu


# ---- 1. small frames, one pixel in the last quad -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4])
@pytest.mark.parametrize("shape", XC.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_small_frames_and_a_lone_pixel_in_the_last_quad(shape, F):
    (W, H), N = shape, (6, 5)
    stack = XC._crafted(W, H, _ppv(F, N), 2000 * W + 10 * H + F)
    with _scanner(W, H, N, F, max_views=10) as sc:                      # exposures in views 1 .. 8, dst_view 0 (below) or 9 (above)
        for e in range(8):
            _upload(sc, 1 + e, stack[e], F, N)
        k = 0
        for E in (1, 3, 8):
            for sat in (255, 200):
                first = 1 if k % 2 == 0 else 9 - E
                src = stack[first - 1:first - 1 + E]
                _, m = _check_fusion(sc, src, first, E, (0, 9)[k // 2 % 2], sat, F, N, 0, (shape, F, E, sat, first))
                assert m.shape == (H, W)
                k += 1
        for e in range(8):
            assert np.array_equal(_download(sc, 1 + e), stack[e]), ("source view", 1 + e)


# ---- 2. every exposure on whole quads, two exposures in the quads between --------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4])
def test_banded_stack_takes_both_paths_of_pass_two(F):
    (W, H), N = XC.BAND_SHAPE, (6, 5)
    stack, band = XC.banded(W, H, F, N)
    with _scanner(W, H, N, F, max_views=11) as sc:
        for first, dsts in ((1, (0, 9)), (2, (0, 1, 10))):              # the sources do not start at view 0; dst_view below and above them
            for e in range(8):
                _upload(sc, first + e, stack[e], F, N)
            for dst in dsts:
                _, m = _check_fusion(sc, stack, first, 8, dst, 255, F, N, 0, ("banded", F, first, dst))
                assert np.array_equal(m & 7, band) and np.array_equal((m & 0x80) != 0, band % 4 == 3)
            for e in range(8):
                assert np.array_equal(_download(sc, first + e), stack[e]), ("source view", first + e)
        # fewer exposures, from the middle: the bands of the others go to whoever is next best
        _, m = _check_fusion(sc, stack[2:7], 4, 5, 0, 255, F, N, 0, ("banded, exposures 2 .. 6", F))
        assert np.array_equal((m & 7)[(band >= 2) & (band <= 6)], band[(band >= 2) & (band <= 6)] - 2)


# ---- 3. the largest clip count ---------------------------------------------------------------------------------------------------------------
def test_every_plane_clipped_in_every_exposure():
    (W, H), F, N = (67, 9), XC.FULL_F, XC.FULL_N
    every, one = XC.full_clip(W, H)
    E = len(every)
    dented = one[E - 1, F + 11] == 254
    with _scanner(W, H, N, F, max_views=E + 2) as sc:
        for e in range(E):
            _upload(sc, 1 + e, every[e], F, N)
        got, m = _check_fusion(sc, every, 1, E, 0, 255, F, N, 0, "n = 72 in every exposure")
        assert (m == 0x80).all() and (got == 255).all()
        _upload(sc, E, one[E - 1], F, N)                                # one byte of 254 on half the pixels of the last exposure
        for dst in (E + 1, 0):
            got, m = _check_fusion(sc, one, 1, E, dst, 255, F, N, 0, ("n = 71 against 72", dst))
            assert np.array_equal(m, np.where(dented, 0x80 | (E - 1), 0x80)) and np.array_equal(got[F + 11] == 254, dented)
        _check_fusion(sc, one, 1, E, 0, 256, F, N, 0, "saturation 256: nothing clips, every score is 0")


# ---- 4. saturations around the switch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4])
def test_saturations_on_both_sides_of_the_switch(F):
    (W, H), N = (67, 9), (6, 5)
    with _scanner(W, H, N, F, max_views=6) as sc:
        for s in XC.EDGE_SATURATIONS:
            stack = XC.crafted_from(XC.saturation_alphabet(s), W, H, _ppv(F, N), 100 + s)[:4]
            for e in range(4):
                _upload(sc, 1 + e, stack[e], F, N)
            maps = {sat: _check_fusion(sc, stack, 1, 4, (0, 5)[sat % 2], sat, F, N, 0, ("alphabet of", s, "saturation", sat, F))[1] for sat in (s - 1, s, s + 1)}
            assert not np.array_equal(maps[s], maps[s - 1]) and not np.array_equal(maps[s], maps[s + 1]), s
