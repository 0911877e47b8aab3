"""CPU tests of the voxel grid's arithmetic (3dscan_amd/csrc/sl3d_voxel.h -- the header k_voxel_insert, k_voxel_count and k_voxel_scatter
compile, free of HIP) against the NumPy restatement of the rule (tests/voxel_reference.py).

The header runs through tests/native/voxel_check.cpp, built by g++ twice: plainly, and as the same stand-alone program with
-fsanitize=address,undefined (every check runs on both).  Cell index, range test and q over 2^18 hashed float bit patterns (every
exponent: denormals, infinities, NaNs among them), hashed floats of a scan's size and the special inputs -- +-0, denormals, +-inf, NaN,
coordinates exactly on a cell face, quotients within an ulp of an integer (3 * 0.1f over 0.1f), the indices -2^20, 2^20 - 1 and 2^20,
negative coordinates -- for seven leaves; key and hash over hashed and extreme indices; the centroid over hashed cells, sums and counts;
the capacity around every power of two.  Everything bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import voxel_reference as VR

SRC = os.path.join(ROOT, "tests", "native", "voxel_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
LEAVES = (0.5, 0.1, 0.3, 1.0, 3.0, 1e-3, 1e-30)
CELL_OUT = np.dtype([("c", "<f8"), ("q", "<i8"), ("ok", "<i4"), ("pad", "<i4")])
CENTROID_IN = np.dtype([("c", "<f8"), ("S", "<i8"), ("count", "<u4"), ("leaf", "<f4")])


@pytest.fixture(scope="module", params=list(FLAGS))
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxel_" + request.param) / "voxel_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *FLAGS[request.param], SRC, "-o", exe])
    return exe


def _run(exe, tmp_path, what, data, dtype):
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    subprocess.check_call([exe, what, src, out], timeout=600)
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


def _inputs(leaf):
    L = np.float32(leaf)
    bits = _hash32(np.arange(1 << 18)).astype(np.uint32).view(np.float32)                       # every kind of float
    scan = ((_hash32(np.arange(1 << 18) + (1 << 20)).astype(np.float64) / 2.0**32 - 0.5) * 900.0).astype(np.float32)
    k = np.arange(-4096, 4096, dtype=np.float32)
    face = k * L                                                                                 # on a cell face, as float arithmetic gives it
    near = np.concatenate([np.nextafter(face, np.float32(np.inf)), np.nextafter(face, np.float32(-np.inf))])
    edge = np.array([-(1 << 20), (1 << 20) - 1, 1 << 20, -(1 << 20) - 1], dtype=np.float64) * np.float64(L)
    edge = np.concatenate([edge.astype(np.float32), np.nextafter(edge.astype(np.float32), np.float32(0)),
                           np.nextafter(edge.astype(np.float32), np.float32(np.inf)), np.nextafter(edge.astype(np.float32), np.float32(-np.inf))])
    tiny = np.array([1, 2, 0x7fffff, 0x800000, 0x80000001, 0x807fffff], dtype=np.uint32).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 3 * np.float32(0.1), -3 * np.float32(0.1), np.float32(0.1) * 3,
                        np.float32(0.3), np.float32(0.7) + np.float32(0.1) + np.float32(0.1)], dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([bits, scan, face, near, edge, tiny, special]).astype(np.float32)


@pytest.mark.parametrize("leaf", LEAVES)
def test_cell_range_and_q(checker, tmp_path, leaf):
    x = _inputs(leaf)
    got = _run(checker, tmp_path, "cells", np.float32(leaf).tobytes() + x.tobytes(), CELL_OUT)
    c, ok = VR.cell(x, leaf)
    assert got.shape == x.shape
    assert np.array_equal(got["ok"] != 0, ok)
    assert np.array_equal(got["c"].view(np.uint64)[~np.isnan(c)], c.view(np.uint64)[~np.isnan(c)]) and np.isnan(got["c"][np.isnan(c)]).all()
    want_q = np.zeros(len(x), np.int64)
    want_q[ok] = VR.q(x[ok], c[ok], leaf)
    assert np.array_equal(got["q"], want_q)
    assert not ok[~np.isfinite(x)].any()                                   # the range test alone refuses NaN and the infinities
    assert want_q.min() >= -1 and want_q.max() <= 1 << 24                  # what sl3d_voxel.h says of q
    if leaf != 1e-30:
        assert ok.mean() > 0.5 and (c[ok] < 0).any() and (c[ok] == -(1 << 20)).any() and (c[ok] == (1 << 20) - 1).any()
        assert (c[~ok & np.isfinite(x)] == 1 << 20).any()                  # 2^20 is the first index out of range


def test_the_quotient_an_ulp_from_an_integer():
    """3 * 0.1f over 0.1f: the float product is above 3 * (double)0.1f, and the cell is 3"""
    x, leaf = np.float32(0.1) * np.float32(3), np.float32(0.1)
    assert np.float64(x) != 3 * np.float64(leaf)
    c, ok = VR.cell(np.array([x]), leaf)
    assert ok[0] and c[0] == np.floor(np.float64(x) / np.float64(leaf))


def test_key_and_hash(checker, tmp_path):
    h = _hash32(np.arange(3 << 16)).astype(np.int64)
    c = ((h & 0x1fffff) - (1 << 20)).reshape(-1, 3)
    lim = np.array([-(1 << 20), (1 << 20) - 1, 0, -1, 1])
    ext = np.stack(np.meshgrid(lim, lim, lim, indexing="ij"), -1).reshape(-1, 3)
    c = np.concatenate([c, ext]).astype(np.int32)
    got = _run(checker, tmp_path, "keys", c.tobytes(), np.uint64).reshape(-1, 2)
    k = VR.key(c)
    assert np.array_equal(got[:, 0], k) and np.array_equal(got[:, 1], VR.mix(k))
    assert int(k.max()) == (1 << 63) - 1 < VR.EMPTY and len(np.unique(k)) == len(np.unique(c, axis=0))
    assert int(VR.mix(np.array([0], np.uint64))[0]) == 0 and int(VR.mix(np.array([1], np.uint64))[0]) == 0x5692161d100b05e5   # splitmix64's finaliser


def test_centroid(checker, tmp_path):
    n = 1 << 16
    h = _hash32(np.arange(4 * n)).astype(np.int64).reshape(4, n)
    rec = np.zeros(n * len(LEAVES[:6]), CENTROID_IN)
    for j, leaf in enumerate(LEAVES[:6]):
        r = rec[j * n:(j + 1) * n]
        r["c"] = ((h[0] & 0x1fffff) - (1 << 20)).astype(np.float64)
        r["count"] = 1 + (h[1] % np.array([1, 2, 7, 5000, 1 << 31])[h[2] % 5])
        r["S"] = (r["count"].astype(np.int64) * (h[3] % ((1 << 24) + 2) - 1))        # a mean q anywhere in [-1, 2^24]
        r["S"] += h[2] % r["count"].astype(np.int64)
        r["leaf"] = np.float32(leaf)
    got = _run(checker, tmp_path, "centroid", rec.tobytes(), np.float32)
    for j, leaf in enumerate(LEAVES[:6]):
        r = rec[j * n:(j + 1) * n]
        want = VR.centroid(r["c"], leaf, r["S"], r["count"])
        assert np.array_equal(got[j * n:(j + 1) * n].view(np.uint32), want.view(np.uint32)), leaf


def test_table_capacity(checker, tmp_path):
    n = np.unique(np.concatenate([[0, 1, 511, 512, 513, (1 << 31) - 1], *[[1 << e, (1 << e) - 1, (1 << e) + 1] for e in range(1, 31)]])).astype(np.int64)
    got = _run(checker, tmp_path, "capacity", n.tobytes(), np.uint64)
    want = np.array([VR.table_capacity(int(v)) for v in n], dtype=np.uint64)
    assert np.array_equal(got, want)
    assert all(int(c) >= max(1024, 2 * int(v)) and int(c) & (int(c) - 1) == 0 and (int(c) == 1024 or int(c) // 2 < 2 * int(v)) for c, v in zip(want, n))
    assert int(want[-1]) == 1 << 32
