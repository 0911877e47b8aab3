"""CPU test of the exposure fusion's crafted inputs (tests/exposure_cases.py): each generator holds what it is there for, by the
restatement tests/exposure_reference.py alone.  The same inputs run on the device in tests/test_gpu_exposure.py and
tests/test_gpu_exposure_edges.py."""
import hashlib

import numpy as np
import pytest

import exposure_cases as XC
import exposure_reference as XR


def _ppv(F, N):
    return 2 * F + 2 * N[0] + 2 * N[1]


def test_crafted_is_what_the_first_device_tests_were_written_over():
    """the bytes tests/test_gpu_exposure.py has drawn since it exists: the generator moved here unchanged"""
    want = {(67, 9, 28, 1): "f5d4d99aefca83d3", (64, 7, 34, 64343): "afed8ce465203f2e"}
    for args, digest in want.items():
        s = XC._crafted(*args)
        assert s.shape == (8,) + args[2:1:-1] + args[1::-1] and s.dtype == np.uint8 and not s.flags.writeable
        assert set(np.unique(s)) == set(XC.ALPHABET.tolist())
        assert np.array_equal(s[2], s[0]) and np.array_equal(s[6], s[3])
        assert hashlib.sha256(s.tobytes()).hexdigest()[:16] == digest, args
    assert XC._crafted(67, 9, 28, 1) is XC.crafted_from((0, 10, 200, 254, 255), 67, 9, 28, 1)


def test_edge_shapes_hold_the_launch_edges():
    shapes = XC.EDGE_SHAPES
    assert all(W % 4 == 1 for W, _ in shapes), "the last quad of a row holds one window pixel"
    assert any(XC.pitch(W) - W >= 4 and W > 4 for W, _ in shapes), "whole padding quads behind the window's last"
    assert any(XC.pitch(W) - W == 3 for W, _ in shapes), "no quad behind the window's last"
    assert any(H == 1 for _, H in shapes) and any(W == 1 and H > 1 for W, H in shapes) and (1, 1) in shapes
    lanes = [-(-W // 4) * H for W, H in shapes]
    assert sum(n < 64 for n in lanes) >= 3 and any(64 < n < 256 for n in lanes), "less than a wave; more than one wave of one block"
    # the counts are what tells: every pixel of the last column is counted once, so a launch that drops the lone pixel of a quad loses H
    F, N = 3, (6, 5)
    for W, H in shapes:
        for sat in (255, 200):
            _, m, counts = XR.fuse(XC._crafted(W, H, _ppv(F, N), 7)[:3], F, *N, 0, sat)
            assert counts[:3].sum() == W * H and m.shape == (H, W)
    _, m, counts = XR.fuse(XC._crafted(253, 2, _ppv(F, N), 7), F, *N, 0, 200)
    assert (m[:, -1] & 0x80).any() and len(set((m[:, -1] & 7).tolist()) | set((m[:, -2] & 7).tolist())) > 1


@pytest.mark.parametrize("F", [3, 4])
def test_banded_stack_takes_every_exposure_on_whole_quads_and_two_at_every_edge(F):
    (W, H), N = XC.BAND_SHAPE, (6, 5)
    assert W <= 322 and H <= 13
    stack, band = XC.banded(W, H, F, N)
    edges = XC.band_edges(W)
    assert edges[0] == 0 and edges[8] == W and all(e % 4 for e in edges[1:8]) and all(b - a >= 7 for a, b in zip(edges, edges[1:]))
    fused, m, counts = XR.fuse(stack, F, *N, 0, 255)
    assert np.array_equal(m & 7, band), "exposure k is chosen on band k, everywhere"
    assert np.array_equal((m & 0x80) != 0, band % 4 == 3), "chosen and clipped on the bands 3 and 7 alone"
    # strictly: by the clip count on the even bands, against the score; by the score alone on the odd ones
    use = XR.planes_in_use(F, *N, 0)
    n = (stack[:, use] >= 255).sum(axis=1)
    q = np.minimum(XR.score(F, stack[:, 0:F].transpose(1, 0, 2, 3)), XR.score(F, stack[:, F + 2 * N[0]:][:, :F].transpose(1, 0, 2, 3)))
    own_n, own_q = np.take_along_axis(n, band[None], axis=0)[0], np.take_along_axis(q, band[None], axis=0)[0]
    others = np.arange(8)[:, None, None] != band[None]
    even = band % 2 == 0
    assert (np.where(others, n, 99).min(axis=0)[even] > own_n[even]).all() and (np.where(others, q, 10 ** 9).min(axis=0)[even] > own_q[even]).all()
    assert (n == own_n[None])[:, ~even].all() and (np.where(others, q, -1).max(axis=0)[~even] < own_q[~even]).all()
    assert set(own_n[~even].tolist()) == {0, 1}
    # the fast path of pass 2 with every e0: a whole aligned quad of one exposure; the slow path beside it: two exposures in the quad at an edge
    quads = (m & 7)[:, :W // 4 * 4].reshape(H, W // 4, 4)
    whole = (quads == quads[..., :1]).all(axis=-1)
    assert {int(e) for e in quads[..., 0][whole]} == set(range(8))
    for e in edges[1:8]:
        at = quads[:, e // 4]
        assert (at[:, 0] != at[:, 3]).all() and not whole[:, e // 4].any(), e
    assert counts[8] == int((band % 4 == 3).sum()) and all(counts[k] == int((band == k).sum()) for k in range(8))
    assert np.array_equal(fused[use], np.take_along_axis(stack[:, use], band[None, None], axis=0)[0])


def test_full_clip_reaches_the_largest_clip_count():
    W, H = 67, 9
    every, one = XC.full_clip(W, H)
    E, ppv = every.shape[:2]
    F, N = XC.FULL_F, XC.FULL_N
    assert ppv == _ppv(F, N) == 72 == len(XR.planes_in_use(F, *N, 0)), "n = 72: the largest clip count of the key"
    fused, m, counts = XR.fuse(every, F, *N, 0, 255)
    assert (m == 0x80).all() and counts.tolist() == [W * H] + [0] * (E - 1) + [W * H] and (fused == 255).all()
    fused, m, counts = XR.fuse(one, F, *N, 0, 255)
    dented = one[E - 1, F + 11] == 254
    assert 0.4 < dented.mean() < 0.6 and (one != every).sum() == dented.sum(), "one byte of 254 on half the pixels: n = 71 against 72"
    assert np.array_equal(m, np.where(dented, 0x80 | (E - 1), 0x80)) and counts.tolist() == [int((~dented).sum())] + [0] * (E - 2) + [int(dented.sum()), W * H]
    assert np.array_equal(fused[F + 11] == 254, dented) and (np.delete(fused, F + 11, axis=0) == 255).all()
    quads = dented[:, :W // 4 * 4].reshape(H, W // 4, 4)
    assert (quads.any(axis=-1) & ~quads.all(axis=-1)).any(), "both exposures within one quad"


@pytest.mark.parametrize("s", XC.EDGE_SATURATIONS)
def test_saturation_alphabets_clip_and_do_not(s):
    alphabet = XC.saturation_alphabet(s)
    assert all(0 <= b <= 255 for b in alphabet) and {s - 1, s, s + 1} <= set(alphabet)
    assert any(b >= s for b in alphabet) and any(b < s for b in alphabet)
    assert sorted(XC.EDGE_SATURATIONS) == [2, 127, 128, 129, 254], "both sides of the switch of exp_clip_test at 127 / 128, and both ends"
    F, N = 3, (6, 5)
    stack = XC.crafted_from(alphabet, 67, 9, _ppv(F, N), 100 + s)[:4]
    assert set(np.unique(stack)) == set(alphabet)
    _, m, counts = XR.fuse(stack, F, *N, 0, s)
    n = (stack >= s).sum(axis=1)
    assert 0 < n.min() and n.max() < _ppv(F, N) and len(np.unique(n.min(axis=0))) >= 4, "clipped and unclipped bytes at every pixel, clip counts that differ"
    assert counts[4] > 0 and (counts[:4] > 0).sum() >= 3, "several exposures are chosen"
    # the neighbouring saturations decide differently: s is told from s - 1 and s + 1
    for other in (s - 1, s + 1):
        assert not np.array_equal(XR.fuse(stack, F, *N, 0, other)[1], m), other
