"""The crafted inputs of the exposure fusion's device tests (tests/test_gpu_exposure.py, tests/test_gpu_exposure_edges.py); inputs only, no
scanner.  tests/test_exposure_cases.py asserts on the CPU, with the restatement tests/exposure_reference.py, what each generator is there for.

_crafted          bytes of the alphabet {0, 10, 200, 254, 255} with pooled plane vectors and two identical pairs of exposures
crafted_from      the same construction over any alphabet: saturation_alphabet(s) = {s - 1, s, s + 1, 0, 255}
EDGE_SHAPES       frames narrower than a quad, shorter than a wave, one row high, W = 1 (mod 4) with and without whole padding quads
banded            eight exposures, exposure k strictly the best on the columns of band k -- by its clip count on the even bands, by its score
                  alone on the odd ones --, the band edges off the multiples of 4
full_clip         every byte 255 in every exposure at the largest plane count, (N_v, N_h) = (16, 16), F = 4: n = 72 everywhere; and the same
                  with one Gray byte of 254 in one exposure on half the pixels"""
import functools

import numpy as np

ALPHABET = np.array([0, 10, 200, 254, 255], np.uint8)
# (W, H): one pixel; two quads, the second with one pixel inside; one column; 17 quads a row and three whole padding quads behind them
# (pitch 80); 64 quads a row, the last with one pixel inside, no whole quad behind it (pitch 256)
EDGE_SHAPES = ((1, 1), (5, 1), (1, 9), (65, 3), (253, 2))
EDGE_SATURATIONS = (2, 127, 128, 129, 254)
BAND_SHAPE = (67, 9)
FULL_N, FULL_F = (16, 16), 4


def pitch(W):
    return (W + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def crafted_from(alphabet, W, H, ppv, seed):
    """uint8 [8][ppv][H][W] over `alphabet` (a tuple of bytes): half the pixels of an exposure take one of six pooled plane vectors (equal clip
    counts AND equal scores across exposures are frequent), the others independent bytes; exposure 2 is exposure 0 and exposure 6 is
    exposure 3."""
    alphabet = np.array(alphabet, np.uint8)
    rng = np.random.default_rng(seed)
    stack = alphabet[rng.integers(0, len(alphabet), (8, ppv, H, W))]
    pool = alphabet[rng.integers(0, len(alphabet), (6, ppv))]
    pooled = pool[rng.integers(0, 6, (8, H, W))].transpose(0, 3, 1, 2)                 # [8][ppv][H][W]
    stack = np.where(rng.random((8, 1, H, W)) < 0.5, pooled, stack)
    stack[2], stack[6] = stack[0], stack[3]
    stack.setflags(write=False)
    return stack


def _crafted(W, H, ppv, seed):
    """crafted_from over {0, 10, 200, 254, 255}"""
    return crafted_from(tuple(int(b) for b in ALPHABET), W, H, ppv, seed)


def saturation_alphabet(s):
    """the bytes around a saturation, and the two ends"""
    return (s - 1, s, s + 1, 0, 255)


def band_edges(W):
    """nine columns 0 .. W: eight bands of about W / 8 columns, no inner edge on a multiple of 4"""
    edges = [int(round(k * W / 8)) for k in range(9)]
    return [e + 1 if 0 < e < W and e % 4 == 0 else e for e in edges]


@functools.lru_cache(maxsize=None)
def banded(W, H, F, N, seed=0):
    """(stack uint8 [8][ppv][H][W], band int [H][W]).  Fringe bytes are 100 .. 120 (scores below 2 100) or, for a well modulated exposure,
    (250, 10, 10(, 10)) on both axes (score 115 200 at F = 3, 57 600 at F = 4); Gray bytes are {0, 10, 200, 254} or, clipped, 255.
      band k even  exposure k: no byte clipped, a small score; every other exposure: one to three clipped Gray bytes and the large score --
                   the clip count decides against the score
      band 1, 5    nobody clips, exposure k alone has the large score
      band 3, 7    every exposure has exactly one clipped Gray byte, exposure k alone has the large score: chosen and flagged clipped"""
    ppv = 2 * F + 2 * N[0] + 2 * N[1]
    rng = np.random.default_rng([W, H, F, N[0], N[1], seed])
    edges = band_edges(W)
    band = np.zeros((H, W), np.int64)
    for k in range(8):
        band[:, edges[k]:edges[k + 1]] = k
    fringe = np.zeros(ppv, bool)
    fringe[0:F] = fringe[F + 2 * N[0]:2 * F + 2 * N[0]] = True
    gray = np.flatnonzero(~fringe)
    stack = np.empty((8, ppv, H, W), np.uint8)
    stack[:, fringe] = rng.integers(100, 121, (8, 2 * F, H, W))
    stack[:, ~fringe] = np.array([0, 10, 200, 254], np.uint8)[rng.integers(0, 4, (8, len(gray), H, W))]
    strong = np.array(([250] + [10] * (F - 1)) * 2, np.uint8)[:, None, None]
    for e in range(8):
        here = band == e
        well = np.where(band % 2 == 0, ~here, here)                          # where this exposure has the large score
        stack[e][fringe] = np.where(well[None], strong, stack[e][fringe])
        n_clipped = np.where(band % 2 == 0, np.where(here, 0, rng.integers(1, 4, (H, W))), np.where(band % 4 == 3, 1, 0))
        order = np.argsort(rng.random((len(gray), H, W)), axis=0)           # per pixel a random order of the Gray planes
        clip = order < n_clipped[None]
        stack[e][gray] = np.where(clip, 255, stack[e][gray])
    stack.setflags(write=False)
    return stack, band


@functools.lru_cache(maxsize=None)
def full_clip(W, H, E=3):
    """(all uint8 [E][72][H][W] of 255, one: the same with 254 in the LAST exposure's Gray plane 11 wherever (row + column // 3) is even)"""
    ppv = 2 * FULL_F + 2 * FULL_N[0] + 2 * FULL_N[1]
    every = np.full((E, ppv, H, W), 255, np.uint8)
    one = every.copy()
    r, c = np.mgrid[0:H, 0:W]
    one[E - 1, FULL_F + 11][(r + c // 3) % 2 == 0] = 254
    every.setflags(write=False), one.setflags(write=False)
    return every, one
