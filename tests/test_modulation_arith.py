"""CPU test of the fringe-modulation arithmetic (3dscan_amd/csrc/sl3d_modulation.h -- the header k_modulation_select /
k_modulation_gamma compile, free of HIP): gamma of every (I0, I1, I2) triple and the selection test built on it, run through the header
(tests/native/modulation_check.cpp) and compared bit for bit with a NumPy float32 restatement of 3/wrapped_phase.cpp:92-96:
d = I0 - I2, e = 2*I1 - I0 - I2, gamma = sqrtf((float)(3d^2 + e^2)) / (float)(I0 + I1 + I2) (0/0 = NaN), selected iff
(double)gamma > thr strictly on both axes and the mask byte is 1."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "modulation_check.cpp")
N = 1 << 24


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modulation") / "modulation_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", exe])
    return exe


def _run(exe, tmp_path, *args, dtype):
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, *args, out], timeout=600)
    return np.fromfile(out, dtype=dtype)


def numpy_gamma():
    t = np.arange(N, dtype=np.int64)
    i0, i1, i2 = t >> 16, (t >> 8) & 255, t & 255
    d, e = i0 - i2, 2 * i1 - i0 - i2
    t1 = np.sqrt((3 * d * d + e * e).astype(np.float32))
    t2 = (i0 + i1 + i2).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t1 / t2


@pytest.fixture(scope="module")
def gamma_ref():
    g = numpy_gamma()
    assert g.dtype == np.float32
    return g


def test_gamma_every_triple_bit_exact(checker, tmp_path, gamma_ref):
    got = _run(checker, tmp_path, "gamma", dtype=np.float32)
    assert got.shape == (N,)
    nan = np.isnan(gamma_ref)
    assert np.array_equal(np.isnan(got), nan)
    assert int(nan.sum()) == 1 and nan[0]                    # t2 == 0 only for I0 = I1 = I2 = 0
    assert np.array_equal(got[~nan].view(np.uint32), gamma_ref[~nan].view(np.uint32))
    assert np.isfinite(got[1:]).all() and got[1:].min() == 0.0 and got[1:].max() > 1.0


def _attained(gamma_ref):
    """gamma values that occur, widened to double: thresholds AT which the strictness of `>` decides"""
    g = gamma_ref[1:]
    return [float(g[np.argmin(np.abs(g - v))]) for v in (0.01, 0.05, 0.1, 0.3)] + [float(np.max(g)), 0.0]


def test_pass_is_strict_and_in_double(checker, tmp_path, gamma_ref):
    g64 = gamma_ref.astype(np.float64)
    attained = _attained(gamma_ref)
    for thr in [0.01, 0.05, 0.1, 0.3, -1.0] + attained:
        got = _run(checker, tmp_path, "pass", float(thr).hex(), dtype=np.uint8)
        want = (g64 > thr).astype(np.uint8)                  # NaN compares false
        assert np.array_equal(got, want), thr
        assert got[0] == 0                                   # NaN never passes
        if thr in attained:
            at = g64 == thr
            assert at.any() and not got[at].any(), thr       # a pixel AT the threshold is rejected
    # the comparison is in double: a threshold half an ulp below an attained gamma g whose float32 mantissa is even.  The tie rounds to
    # g, so float32(thr) == g: a comparison against (float)thr would reject every pixel AT g, the one in double keeps them all.
    f = gamma_ref[1:]
    near = f[np.argsort(np.abs(f.astype(np.float64) - 0.05))[:1000]]
    g = next(v for v in near if v > 0 and (int(v.view(np.uint32)) & 1) == 0)
    below = np.nextafter(g, np.float32(0))
    thr = (float(g) + float(below)) / 2.0
    assert float(below) < thr < float(g) and np.float32(thr) == g
    got = _run(checker, tmp_path, "pass", thr.hex(), dtype=np.uint8)
    at = gamma_ref == g
    assert np.array_equal(got, (g64 > thr).astype(np.uint8))
    assert at.any() and got[at].all()                        # kept by the double comparison ...
    assert not (gamma_ref[at] > np.float32(thr)).any()        # ... rejected by a float one

def test_select_ands_the_mask_and_both_axes(checker, tmp_path, gamma_ref):
    t = np.arange(N, dtype=np.uint64)
    gh = gamma_ref[(t * np.uint64(2654435761)) & np.uint64(N - 1)].astype(np.float64)
    gv = gamma_ref.astype(np.float64)
    mask1 = (t % np.uint64(3)) == 1
    for thr in (0.01, 0.05, 0.1, 0.3):
        got = _run(checker, tmp_path, "select", float(thr).hex(), dtype=np.uint8)
        want = mask1 & (gv > thr) & (gh > thr)
        assert np.array_equal(got, want.astype(np.uint8)), thr
        assert 0 < int(got.sum()) < int(mask1.sum())
