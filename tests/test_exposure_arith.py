"""CPU tests of the exposure-fusion arithmetic (3dscan_amd/csrc/sl3d_exposure.h -- the header k_fuse_exposures compiles, free of HIP) and
of the NumPy restatement of the rule (tests/exposure_reference.py).

The header runs through tests/native/exposure_check.cpp, built by g++ twice: plainly, and as the same stand-alone program with
-fsanitize=address,undefined (every check runs on both).
- exp_score against NumPy over every (I0, I1, I2) triple for F = 3 and over 2^20 hashed quadruples for F = 4;
- exp_key: its order is the lexicographic rule (fewer clipped planes, then the larger score, then the smaller e) over all n in 0 .. 72,
  the boundary scores and e in 0 .. 7;
- the packed clip test and the byte comparison the kernel counts and selects with, over every saturation and byte.
The restatement on the three-band scene (96 x 40, N = 7, fringe width 4, F = 3 and 4, noise 0 and +-2): on every lit pixel the map is the
band index, the fused stack is the gain-0.8 capture byte for byte, no pixel is clipped in every exposure."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import exposure_reference as XR

SRC = os.path.join(ROOT, "tests", "native", "exposure_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exposure_" + request.param) / "exposure_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *FLAGS[request.param], SRC, "-o", exe])
    return exe


def _run(exe, tmp_path, what, dtype):
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, what, out], timeout=600)
    return np.fromfile(out, dtype=dtype)


def _hash32(t):
    t = t.astype(np.uint64)
    m = np.uint64(0xffffffff)
    t ^= t >> np.uint64(16)
    t = (t * np.uint64(0x7feb352d)) & m
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x846ca68b)) & m
    t ^= t >> np.uint64(16)
    return t


def test_score_every_triple_three_step(checker, tmp_path):
    got = _run(checker, tmp_path, "score3", np.uint32)
    t = np.arange(1 << 24, dtype=np.int64)
    i0, i1, i2 = t >> 16, (t >> 8) & 255, t & 255
    want = (i0 - i2) ** 2 + (2 * i1 - i0 - i2) ** 2
    assert np.array_equal(got, want)
    assert int(want.max()) == 510 * 510 <= 325125 < 1 << 19 and int(want.min()) == 0   # (the bound 255^2 + 510^2 of the header is not attained)


def test_score_hashed_quadruples_four_step(checker, tmp_path):
    got = _run(checker, tmp_path, "score4", np.uint32)
    h = _hash32(np.arange(1 << 20)).astype(np.int64)
    i0, i1, i2, i3 = h & 255, (h >> 8) & 255, (h >> 16) & 255, h >> 24
    want = (i3 - i1) ** 2 + (i0 - i2) ** 2
    assert got.shape == (1 << 20,) and np.array_equal(got, want)
    assert np.array_equal(want, XR.score(4, [i0, i1, i2, i3])) and want.max() > 120000   # (the restatement's score is this one)


def test_key_order_is_the_lexicographic_rule(checker, tmp_path):
    keys = _run(checker, tmp_path, "keys", np.uint32)
    Q = (0, 1, 325124, 325125)
    triples = [(n, q, e) for n in range(73) for q in Q for e in range(8)]
    assert keys.shape == (len(triples),) and len(set(keys.tolist())) == len(triples)
    assert all(int(k) == ((127 - n) << 22) | (q << 3) | (7 - e) for k, (n, q, e) in zip(keys, triples))   # the formula of the header
    # a larger key <=> fewer clipped planes, then the larger score, then the smaller e: the two total orders are the same order
    by_key = [t for _, t in sorted(zip(keys.tolist(), triples))]
    by_rule = sorted(triples, key=lambda t: (-t[0], t[1], -t[2]))
    assert by_key == by_rule
    assert int(keys.max()) < 1 << 29


def test_packed_clip_test_and_byte_comparison(checker, tmp_path):
    got = _run(checker, tmp_path, "clipped", np.uint8).reshape(256, 256)
    s, x = np.meshgrid(np.arange(1, 257), np.arange(256), indexing="ij")
    assert np.array_equal(got, (x >= s).astype(np.uint8))
    assert not got[255].any() and got[0][1:].all() and not got[0][0]   # 256: nothing ever clips; 1: every byte but 0 does
    assert _run(checker, tmp_path, "equal", np.uint8).all()


@pytest.fixture(scope="module")
def scenes(synth):
    return {(F, noise): XR.three_band_scene(synth, 96, 40, 512, 384, 7, 4, F, noise=noise) for F in (3, 4) for noise in (0, 2)}


@pytest.mark.parametrize("noise", [0, 2])
@pytest.mark.parametrize("F", [3, 4])
def test_restatement_on_the_three_band_scene(scenes, F, noise):
    sc = scenes[(F, noise)]
    lit = sc["lit"]
    assert lit.mean() > 0.5 and all((sc["band"][lit] == b).sum() > 300 for b in range(3))
    fused, emap, counts = XR.fuse(sc["stack"], F, 7, 7, 0, 255)
    assert np.array_equal(emap[lit], sc["band"][lit])          # every lit pixel: its band's exposure, not clipped
    assert np.array_equal(fused, sc["base"])                   # byte for byte the gain-0.8 capture
    assert counts[3] == 0 and int(counts[:3].sum()) == lit.size and not (emap & 0x80).any()
    assert np.array_equal(counts[:3], np.bincount((emap & 7).ravel(), minlength=3))
    # no single exposure is that capture: each differs on the lit pixels of two bands
    for e in range(3):
        same = (sc["stack"][e] == sc["base"]).all(axis=0)
        assert same[lit & (sc["band"] == e)].all() and not same[lit & (sc["band"] != e)].any()
